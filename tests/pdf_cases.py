"""The PDF corpus of tests/test_pdf_host.py and tests/test_gpu_pdf.py, from a builder that knows nothing of model/pdf.py: objects are
assembled by hand, Group 4 and LZW strips come out of Pillow's TIFF writer, JPEGs from Pillow, Flate streams from zlib over rows
filtered in NumPy.  Every case keeps the pixels its pages must show (for lossless streams the array it started from, for DCT
Pillow's decode of the same JPEG bytes), put on the page by tests/pdf_ref.py, or the words the refusal must contain.

corpus() -> {name: Case}: Case.pdf (bytes), Case.pages (per page a (H, W, 3) B,G,R array, or a str the refusal reason must contain),
Case.error (None, or a str PdfError's text must contain), Case.codes (per page the orientation codes of its images, where the case
pins them), Case.host_only (True where the issue leaves the images to the host)."""
import functools
import io
import struct
import zlib

import numpy as np
from PIL import Image

import pdf_ref as R

SIZES = ((1, 1), (33, 31), (64, 64), (65, 129), (70, 131))          # (h, w)


class Case:
    def __init__(self, pdf, pages, error=None, codes=None, host_only=False):
        self.pdf, self.pages, self.error, self.codes, self.host_only = pdf, pages, error, codes, host_only


# ---- pixels ---------------------------------------------------------------------------------------------------------------------------------
def gray_image(h, w, seed):
    rng = np.random.RandomState(seed)
    a = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5) + rng.randint(0, 40, (h, w))) % 256
    return a.astype(np.uint8)


def rgb_image(h, w, seed):
    return np.stack([gray_image(h, w, seed + k) for k in range(3)], axis=2)


def bilevel_image(h, w, seed):
    """True = white paper, with rules and blobs of ink."""
    rng = np.random.RandomState(seed)
    a = np.ones((h, w), bool)
    a[h // 3, :] = False
    a[:, w // 4] = False
    a &= rng.rand(h, w) > 0.08
    return a


def bgr(a):
    """(h, w) gray, bool or (h, w, 3) R,G,B -> (h, w, 3) B,G,R uint8."""
    if a.dtype == bool:
        a = a.astype(np.uint8) * 255
    if a.ndim == 2:
        return np.ascontiguousarray(np.repeat(a[:, :, None], 3, axis=2))
    return np.ascontiguousarray(a[:, :, ::-1])


# ---- streams --------------------------------------------------------------------------------------------------------------------------------
def tiff_strip(im, compression, tiffinfo):
    """The single strip of Pillow's TIFF of an image."""
    b = io.BytesIO()
    info = dict(tiffinfo)
    info[278] = im.size[1]
    im.save(b, "TIFF", compression=compression, tiffinfo=info)
    data = b.getvalue()
    order = "<" if data[:2] == b"II" else ">"
    ifd, = struct.unpack_from(order + "I", data, 4)
    n, = struct.unpack_from(order + "H", data, ifd)
    tags = {}
    for k in range(n):
        tag, typ, count = struct.unpack_from(order + "HHI", data, ifd + 2 + 12 * k)
        tags[tag] = struct.unpack_from(order + ("H" if typ == 3 else "I"), data, ifd + 10 + 12 * k)[0]
        assert count == 1 or tag not in (273, 279)
    return data[tags[273]:tags[273] + tags[279]]


def g4(white, black_is_1):
    """The Group 4 strip of a bool image (True = white).  black_is_1: white pixels are coded as the decoder's 0 bits... which a PDF
    shows white only under /BlackIs1 true; otherwise they are coded as white runs, PDF's default."""
    im = Image.fromarray(white)                                       # mode "1", 1 = white
    return tiff_strip(im, "group4", {262: 1 if black_is_1 else 0})


def lzw(rows_u8):
    """TIFF LZW (= PDF LZWDecode with EarlyChange 1) of a 2-D uint8 array of row bytes."""
    return tiff_strip(Image.fromarray(rows_u8), "tiff_lzw", {})


def jpeg(a, quality=90):
    """(bytes, the (h, w, 3) B,G,R pixels Pillow decodes from them)."""
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality)
    with Image.open(io.BytesIO(b.getvalue())) as im:
        return b.getvalue(), np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def row_bytes(a, bits):
    """The rows of an image as PDF stores them: (h, bytes per row) uint8; a: (h, w) or (h, w, 3) samples."""
    flat = a.reshape(a.shape[0], -1)
    return np.packbits(flat.astype(bool), axis=1) if bits == 1 else flat.astype(np.uint8)


def png_rows(rows, bpp, predictor):
    """Rows with a PNG filter byte in front: predictor 10 None, 11 Sub, 12 Up, 15 the three in turn."""
    h = rows.shape[0]
    r = rows.astype(np.int64)
    left = np.zeros_like(r)
    left[:, bpp:] = r[:, :-bpp] if bpp < r.shape[1] else 0
    up = np.zeros_like(r)
    up[1:] = r[:-1]
    out = np.zeros((h, rows.shape[1] + 1), np.uint8)
    for y in range(h):
        ft = {10: 0, 11: 1, 12: 2}.get(predictor, y % 3)
        out[y, 0] = ft
        out[y, 1:] = (r[y] - (0 if ft == 0 else left[y] if ft == 1 else up[y])) & 255
    return out.tobytes()


def tiff_predicted(rows, bpp):
    """TIFF predictor 2 on 8-bit samples: every sample minus the one bpp bytes before it."""
    r = rows.astype(np.int64)
    out = r.copy()
    out[:, bpp:] = r[:, bpp:] - r[:, :-bpp]
    return (out & 255).astype(np.uint8)


def ascii85(data):
    import base64
    return base64.a85encode(data) + b"~>"


# ---- the builder ----------------------------------------------------------------------------------------------------------------------------
class Builder:
    """Objects by number; finish() lays the file out with a classic table, or with an object stream and a cross-reference stream."""

    def __init__(self):
        self.objs = {}
        self.next = 1

    def reserve(self):
        self.next += 1
        return self.next - 1

    def put(self, body, num=None):
        num = self.reserve() if num is None else num
        self.objs[num] = body if isinstance(body, bytes) else body.encode("latin-1")
        return num

    def stream(self, d, data, num=None):
        return self.put(("<< %s /Length %d >>\nstream\n" % (d, len(data))).encode("latin-1") + data + b"\nendstream", num)

    def finish(self, root, xref="table", trailer_extra="", header=b"%PDF-1.4\n%\xe2\xe3\xcf\xd3\n"):
        out = bytearray(header)
        if xref == "table":
            offsets = {}
            for num in sorted(self.objs):
                offsets[num] = len(out)
                out += b"%d 0 obj\n" % num + self.objs[num] + b"\nendobj\n"
            at = len(out)
            out += b"xref\n0 %d\n0000000000 65535 f \n" % self.next
            for num in range(1, self.next):
                out += b"%010d 00000 n \n" % offsets[num] if num in offsets else b"0000000000 00000 f \n"
            out += ("trailer\n<< /Size %d /Root %d 0 R %s >>\nstartxref\n%d\n%%%%EOF\n" % (self.next, root, trailer_extra, at)).encode("latin-1")
            return bytes(out)
        # PDF 1.5: every object that is no stream goes into one object stream
        plain = [n for n in sorted(self.objs) if not self.objs[n].rstrip().endswith(b"endstream")]
        head, body = b"", b""
        for n in plain:
            head += b"%d %d " % (n, len(body))
            body += self.objs[n] + b"\n"
        holder = self.reserve()
        payload = zlib.compress(head + body)
        self.objs[holder] = ("<< /Type /ObjStm /N %d /First %d /Filter /FlateDecode /Length %d >>\nstream\n" % (
            len(plain), len(head), len(payload))).encode("latin-1") + payload + b"\nendstream"
        offsets = {}
        for num in sorted(self.objs):
            if num in plain:
                continue
            offsets[num] = len(out)
            out += b"%d 0 obj\n" % num + self.objs[num] + b"\nendobj\n"
        xnum = self.reserve()
        at = len(out)
        rows = np.zeros((self.next, 7), np.uint8)                     # W [1 4 2]
        for num in range(self.next):
            if num in plain:
                rec = struct.pack(">BIH", 2, holder, plain.index(num))
            elif num in offsets or num == xnum:
                rec = struct.pack(">BIH", 1, at if num == xnum else offsets[num], 0)
            else:
                rec = struct.pack(">BIH", 0, 0, 65535 if num == 0 else 0)
            rows[num] = np.frombuffer(rec, np.uint8)
        payload = zlib.compress(png_rows(rows, 1, 12))
        out += ("%d 0 obj\n<< /Type /XRef /Size %d /W [1 4 2] /Root %d 0 R /Filter /FlateDecode /DecodeParms << /Predictor 12 /Columns 7 >> "
                "/Length %d %s >>\nstream\n" % (xnum, self.next, root, len(payload), trailer_extra)).encode("latin-1")
        out += payload + b"\nendstream\nendobj\n"
        out += b"startxref\n%d\n%%%%EOF\n" % at
        return bytes(out)


def num(v):
    s = "%.6f" % v
    return s.rstrip("0").rstrip(".")


def image_dict(w, h, rest):
    return "/Type /XObject /Subtype /Image /Width %d /Height %d %s" % (w, h, rest)


def simple(pages, xref="table", trailer_extra="", inherit=None, pages_extra=""):
    """A file of `pages`: each a dict with media (x0, y0, x1, y1; None: inherited), rotate (None: absent), contents (a list of
    bytes), images {name: (dict text, data, aux)}, aux a list of (dict text, data) streams whose numbers replace {0}, {1}, ... in
    the dict text; resources_extra and page_extra (text).  inherit: (media, rotate) on the /Pages node."""
    b = Builder()
    catalog, tree = b.reserve(), b.reserve()
    kids = []
    for p in pages:
        page = b.reserve()
        names = []
        for name, (d, data, aux) in p.get("images", {}).items():
            nums = [b.stream(ad, adata) for ad, adata in aux]
            names.append("/%s %d 0 R" % (name, b.stream(d.format(*nums), data)))
        for name, (d, data) in p.get("forms", {}).items():
            names.append("/%s %d 0 R" % (name, b.stream(d, data)))
        contents = [b.stream(d, data) for d, data in p["contents"]]
        text = "<< /Type /Page /Parent %d 0 R " % tree
        if p.get("media") is not None:
            text += "/MediaBox [%s] " % " ".join(num(v) for v in p["media"])
        if p.get("rotate") is not None:
            text += "/Rotate %d " % p["rotate"]
        text += "/Resources << /XObject << %s >> %s >> " % (" ".join(names), p.get("resources_extra", ""))
        text += "/Contents %s " % ("%d 0 R" % contents[0] if len(contents) == 1 else "[%s]" % " ".join("%d 0 R" % c for c in contents))
        b.put(text + p.get("page_extra", "") + ">>", page)
        kids.append(page)
    b.put("<< /Type /Catalog /Pages %d 0 R >>" % tree, catalog)
    text = "<< /Type /Pages /Count %d /Kids [%s] " % (len(kids), " ".join("%d 0 R" % k for k in kids))
    if inherit:
        text += "/MediaBox [%s] /Rotate %d " % (" ".join(num(v) for v in inherit[0]), inherit[1])
    b.put(text + pages_extra + ">>", tree)
    return b.finish(catalog, xref, trailer_extra), b


def upright(w, h):
    return (w, 0, 0, h, 0, 0)


def draw(name, ctm):
    return ("q %s cm /%s Do Q\n" % (" ".join(num(v) for v in ctm), name)).encode("latin-1")


def one(d, data, shown, w, h, aux=(), rotate=None, media=None, ctm=None):
    """A one-page file showing one image: `shown` its (h, w, 3) B,G,R pixels; the CTM upright at one pixel per point by default."""
    ctm = upright(w, h) if ctm is None else ctm
    media = (0, 0, w, h) if media is None else media
    page = {"media": media, "rotate": rotate, "contents": [("", draw("Im0", ctm))], "images": {"Im0": (image_dict(w, h, d), data, list(aux))}}
    return Case(simple([page])[0], [R.render(media, rotate or 0, [(shown, ctm)])])


CTMS = {                                                             # orientation code -> CTM of a w x h image at one pixel per point
    1: lambda w, h: (w, 0, 0, h, 0, 0), 2: lambda w, h: (-w, 0, 0, h, w, 0), 3: lambda w, h: (-w, 0, 0, -h, w, h),
    4: lambda w, h: (w, 0, 0, -h, 0, h), 5: lambda w, h: (0, -w, -h, 0, h, w), 6: lambda w, h: (0, -w, h, 0, 0, w),
    7: lambda w, h: (0, w, h, 0, 0, 0), 8: lambda w, h: (0, w, -h, 0, h, 0),
}


def flate(rows):
    return zlib.compress(rows.tobytes() if isinstance(rows, np.ndarray) else rows)


def raw_gray(h, w, seed):
    """The plain refusal carrier: an unfiltered 8-bit gray image."""
    a = gray_image(h, w, seed)
    return "/ColorSpace /DeviceGray /BitsPerComponent 8", a.tobytes(), bgr(a)


@functools.lru_cache(maxsize=None)
def corpus():
    c = {}
    H1, W1 = SIZES[1]
    H2, W2 = SIZES[2]
    H3, W3 = SIZES[3]
    H4, W4 = SIZES[4]

    # ---- every accepted kind of stream ------------------------------------------------------------------------------------------------
    g, want = jpeg(gray_image(H4, W4, 1))
    c["dct_gray"] = one("/ColorSpace /DeviceGray /BitsPerComponent 8 /Filter /DCTDecode", g, want, W4, H4)
    g, want = jpeg(rgb_image(H3, W3, 2))
    c["dct_rgb_calrgb"] = one("/ColorSpace [/CalRGB << /WhitePoint [0.95 1 1.09] >>] /BitsPerComponent 8 /Filter [/DCTDecode]", g, want, W3, H3)
    g, want = jpeg(rgb_image(H1, W1, 3))
    c["dct_rgb_ascii85"] = one("/ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter [/ASCII85Decode /DCTDecode] /DecodeParms [null null]",
                               ascii85(g), want, W1, H1)
    g, want = jpeg(gray_image(1, 1, 4))
    c["dct_gray_1x1"] = one("/ColorSpace /DeviceGray /BitsPerComponent 8 /Filter /DCTDecode", g, want, 1, 1)
    g, want = jpeg(gray_image(H2, W2, 5))
    c["dct_gray_decode_reversed"] = one("/ColorSpace /DeviceGray /BitsPerComponent 8 /Filter /DCTDecode /Decode [1 0]", g, 255 - want, W2, H2)

    for name, (h, w), black_is_1, extra, flip in (
            ("g4_blackis1", SIZES[4], True, "/ColorSpace /DeviceGray", False),
            ("g4_default", SIZES[3], False, "/ColorSpace /DeviceGray", False),
            ("g4_decode_reversed", SIZES[1], False, "/ColorSpace /DeviceGray /Decode [1 0]", True),
            ("g4_image_mask", SIZES[2], True, "/ImageMask true", False),
            ("g4_image_mask_reversed", SIZES[1], True, "/ImageMask true /Decode [1 0]", True),
            ("g4_1x1", SIZES[0], True, "/ColorSpace [/CalGray << /WhitePoint [0.95 1 1.09] >>]", False),
            ("g4_indexed_bw", SIZES[1], True, "/ColorSpace [/Indexed /DeviceGray 1 <00FF>]", False)):
        white = bilevel_image(h, w, 10 + len(c))
        parms = "/K -1 /Columns %d /Rows %d /BlackIs1 %s" % (w, h, "true" if black_is_1 else "false")
        d = "%s /BitsPerComponent 1 /Filter /CCITTFaxDecode /DecodeParms << %s >>" % (extra, parms)
        if name == "g4_default":                                     # filter and parms as arrays, as Pillow writes them
            d = "%s /BitsPerComponent 1 /Filter [/CCITTFaxDecode] /DecodeParms [<< %s >>]" % (extra, parms)
        c[name] = one(d, g4(white, black_is_1), bgr(white ^ flip), w, h)

    a = gray_image(H4, W4, 20)
    c["flate_png15_gray"] = one("/ColorSpace /DeviceGray /BitsPerComponent 8 /Filter /FlateDecode /DecodeParms << /Predictor 15 /Columns %d >>" % W4,
                                flate(png_rows(row_bytes(a, 8), 1, 15)), bgr(a), W4, H4)
    a = rgb_image(H3, W3, 21)
    c["flate_png15_rgb_icc"] = one(
        "/ColorSpace [/ICCBased {0} 0 R] /BitsPerComponent 8 /Filter /FlateDecode /DecodeParms << /Predictor 15 /Colors 3 /Columns %d >>" % W3,
        flate(png_rows(row_bytes(a, 8), 3, 15)), bgr(a), W3, H3, aux=[("/N 3", b"not a profile anyone reads")])
    a = rgb_image(H1, W1, 22)
    c["flate_png11_rgb"] = one("/ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter [/FlateDecode] /DecodeParms [<< /Predictor 11 /Colors 3 "
                               "/BitsPerComponent 8 /Columns %d >>]" % W1, flate(png_rows(row_bytes(a, 8), 3, 11)), bgr(a), W1, H1)
    white = bilevel_image(H2, W2, 23)
    c["flate_png12_gray1"] = one("/ColorSpace /DeviceGray /BitsPerComponent 1 /Filter /FlateDecode /DecodeParms << /Predictor 12 "
                                 "/BitsPerComponent 1 /Columns %d >>" % W2, flate(png_rows(row_bytes(white, 1), 1, 12)), bgr(white), W2, H2)
    idx = gray_image(H1, W1, 24) % 7
    pal = np.array([[255, 255, 255], [0, 0, 0], [200, 30, 30], [30, 200, 30], [30, 30, 200], [250, 250, 0], [90, 90, 90]], np.uint8)
    c["flate_png10_indexed_string"] = one(
        "/ColorSpace [/Indexed /DeviceRGB 6 <%s>] /BitsPerComponent 8 /Filter /FlateDecode /DecodeParms << /Predictor 10 /Columns %d >>"
        % (pal.tobytes().hex(), W1), flate(png_rows(row_bytes(idx, 8), 1, 10)), bgr(pal[idx]), W1, H1)
    idx = gray_image(H3, W3, 25) % 7
    c["flate_indexed_stream"] = one("/ColorSpace [/Indexed /DeviceRGB 6 {0} 0 R] /BitsPerComponent 8 /Filter /FlateDecode",
                                    flate(row_bytes(idx, 8)), bgr(pal[idx]), W3, H3, aux=[("/Filter /FlateDecode", zlib.compress(pal.tobytes()))])
    a = gray_image(H1, W1, 26)
    c["flate_gray"] = one("/ColorSpace /DeviceGray /BitsPerComponent 8 /Filter /FlateDecode", flate(row_bytes(a, 8)), bgr(a), W1, H1)
    a = rgb_image(H4, W4, 27)
    c["flate_rgb_hex"] = one("/ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter [/ASCIIHexDecode /FlateDecode]",
                             flate(row_bytes(a, 8)).hex().encode("ascii") + b">", bgr(a), W4, H4)
    white = bilevel_image(H3, W3, 28)
    c["flate_gray1"] = one("/ColorSpace /DeviceGray /BitsPerComponent 1 /Filter /FlateDecode", flate(row_bytes(white, 1)), bgr(white), W3, H3)
    a = rgb_image(H2, W2, 29)
    c["flate_tiff2_rgb"] = one("/ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /FlateDecode /DecodeParms << /Predictor 2 /Colors 3 /Columns %d >>" % W2,
                               flate(tiff_predicted(row_bytes(a, 8), 3)), bgr(a), W2, H2)
    a = gray_image(H1, W1, 30)
    c["flate_tiff2_gray_reversed"] = one("/ColorSpace /DeviceGray /BitsPerComponent 8 /Decode [1 0] /Filter /FlateDecode /DecodeParms << /Predictor 2 "
                                         "/Columns %d >>" % W1, flate(tiff_predicted(row_bytes(a, 8), 1)), bgr(255 - a), W1, H1)
    a = gray_image(H4, W4, 31)
    c["lzw_gray"] = one("/ColorSpace /DeviceGray /BitsPerComponent 8 /Filter /LZWDecode", lzw(row_bytes(a, 8)), bgr(a), W4, H4)
    a = rgb_image(H1, W1, 32)
    c["lzw_tiff2_rgb"] = one("/ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /LZWDecode /DecodeParms << /Predictor 2 /Colors 3 /Columns %d "
                             "/EarlyChange 1 >>" % W1, lzw(tiff_predicted(row_bytes(a, 8), 3)), bgr(a), W1, H1)
    a = gray_image(H2, W2, 33)
    c["raw_gray"] = one("/ColorSpace /DeviceGray /BitsPerComponent 8", a.tobytes(), bgr(a), W2, H2)
    a = rgb_image(1, 1, 34)
    c["raw_rgb_1x1"] = one("/ColorSpace /DeviceRGB /BitsPerComponent 8", a.tobytes(), bgr(a), 1, 1)
    a = rgb_image(H3, W3, 35)
    c["raw_rgb"] = one("/ColorSpace /DeviceRGB /BitsPerComponent 8", a.tobytes(), bgr(a), W3, H3)
    white = bilevel_image(H1, W1, 36)
    c["raw_gray1_mask"] = one("/ImageMask true", row_bytes(white, 1).tobytes(), bgr(white), W1, H1)
    a4 = gray_image(H1, W1, 37) >> 4                                # 4-bit gray: wrapped, and left to the host
    packed = (a4[:, 0::2] << 4 | np.pad(a4, ((0, 0), (0, W1 % 2)))[:, 1::2]).astype(np.uint8)
    c["flate_png10_gray4_host"] = one("/ColorSpace /DeviceGray /BitsPerComponent 4 /Filter /FlateDecode /DecodeParms << /Predictor 10 "
                                      "/BitsPerComponent 4 /Columns %d >>" % W1, flate(png_rows(packed, 1, 10)), bgr((a4 * 17).astype(np.uint8)), W1, H1)
    c["flate_png10_gray4_host"].host_only = True

    # ---- geometry -------------------------------------------------------------------------------------------------------------------------
    for code in range(1, 9):
        h, w = SIZES[1 + code % 4]
        a = rgb_image(h, w, 40 + code)
        ow, oh = (h, w) if code >= 5 else (w, h)
        c["orientation_%d" % code] = one("/ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /FlateDecode", flate(row_bytes(a, 8)), bgr(a), w, h,
                                         ctm=CTMS[code](w, h), media=(0, 0, ow, oh))
        c["orientation_%d" % code].codes = [[code]]
    for rotate in (0, 90, 180, 270, -90):
        a = rgb_image(H3, W3, 50 + rotate % 7)
        c["rotate_%d" % rotate] = one("/ColorSpace /DeviceRGB /BitsPerComponent 8", a.tobytes(), bgr(a), W3, H3, rotate=rotate)
    a = gray_image(H1, W1, 56)
    c["rotate_90_of_orientation_7_inverted"] = one("/ColorSpace /DeviceGray /BitsPerComponent 8 /Decode [1 0]", a.tobytes(), bgr(255 - a), W1, H1,
                                                   ctm=CTMS[7](W1, H1), media=(0, 0, H1, W1), rotate=90)
    # five strips of 64, 64, 64, 64 and 7 rows at 300 dpi
    white = bilevel_image(263, 131, 57)
    unit = 72.0 / 300.0
    images, content, draws = {}, b"", []
    for k, row in enumerate(range(0, 263, 64)):
        rows = min(64, 263 - row)
        part = white[row:row + rows]
        images["S%d" % k] = (image_dict(131, rows, "/ColorSpace /DeviceGray /BitsPerComponent 1 /Filter /CCITTFaxDecode /DecodeParms << /K -1 "
                                        "/Columns 131 /Rows %d >>" % rows), g4(part, False), [])
        ctm = (131 * unit, 0, 0, rows * unit, 0, (263 - row - rows) * unit)
        content += draw("S%d" % k, ctm)
        draws.append((bgr(part), ctm))
    media = (0, 0, 131 * unit, 263 * unit)
    c["five_strips"] = Case(simple([{"media": media, "contents": [("", content)], "images": images}])[0], [R.render(media, 0, draws)])
    assert np.array_equal(c["five_strips"].pages[0], bgr(white))
    # an image hanging over each of the four MediaBox edges, on a MediaBox that is not at the origin; the first sets the scale
    media = (10, 20, 10 + 131, 20 + 140)
    images, content, draws = {}, b"", []
    for k, (x, y) in enumerate(((40, 60), (-12, 70), (131 - 20, 40), (40, 140 - 15), (50, -9))):
        a = rgb_image(H1, W1, 60 + k)
        images["I%d" % k] = (image_dict(W1, H1, "/ColorSpace /DeviceRGB /BitsPerComponent 8"), a.tobytes(), [])
        ctm = (W1, 0, 0, H1, 10 + x, 20 + y)
        content += draw("I%d" % k, ctm)
        draws.append((bgr(a), ctm))
    c["over_the_edges"] = Case(simple([{"media": media, "contents": [("", content)], "images": images}])[0], [R.render(media, 0, draws)])
    # inherited MediaBox and Rotate, contents as an array of three streams (one Flate, one ASCIIHex, one ASCII85), a marked-content pair
    a = gray_image(H1, W1, 66)
    d, data, shown = raw_gray(H1, W1, 66)
    ctm = upright(W1, H1)
    parts = [("/Filter /FlateDecode", zlib.compress(b"/Artifact BMC q 0 g 0 G\n")),
             ("/Filter /ASCIIHexDecode", ("%s cm" % " ".join(num(v) for v in ctm)).encode().hex().encode() + b">"),
             ("/Filter [/ASCII85Decode]", ascii85(b" /Im0 Do Q EMC\n"))]
    page = {"media": None, "contents": parts, "images": {"Im0": (image_dict(W1, H1, d), data, [])}}
    c["inherited_contents_array"] = Case(simple([page], inherit=((0, 0, W1, H1), 270))[0], [R.render((0, 0, W1, H1), 270, [(shown, ctm)])])
    # PDF 1.5: object stream and cross-reference stream; two pages
    pages, want = [], []
    for k, (h, w) in enumerate((SIZES[1], SIZES[3])):
        d, data, shown = raw_gray(h, w, 70 + k)
        pages.append({"media": (0, 0, w, h), "rotate": 90 * k, "contents": [("", draw("Im0", upright(w, h)))], "images": {"Im0": (image_dict(w, h, d), data, [])}})
        want.append(R.render((0, 0, w, h), 90 * k, [(shown, upright(w, h))]))
    c["xref_stream"] = Case(simple(pages, xref="stream")[0], want)
    # an incremental update: the page object replaced by one with /Rotate 180, a second table with /Prev; /Length indirect
    d, data, shown = raw_gray(H1, W1, 72)
    b = Builder()
    catalog, tree, page, content, image, length = (b.reserve() for _ in range(6))
    text = draw("Im0", upright(W1, H1))
    b.put("<< /Type /Catalog /Pages %d 0 R >>" % tree, catalog)
    b.put("<< /Type /Pages /Count 1 /Kids [%d 0 R] >>" % page, tree)
    body = "<< /Type /Page /Parent %d 0 R /MediaBox [0 0 %d %d] /Resources << /XObject << /Im0 %d 0 R >> >> /Contents %d 0 R %%s>>" % (tree, W1, H1, image, content)
    b.put(body % "", page)
    b.put(b"<< /Length %d 0 R >>\nstream\n" % length + text + b"\nendstream", content)
    b.put("%d" % len(text), length)
    b.stream(image_dict(W1, H1, d), data, image)
    first = b.finish(catalog)
    prev = int(first[first.rindex(b"startxref") + 9:].split()[0])
    update = b"%d 0 obj\n" % page + (body % "/Rotate 180 ").encode("latin-1") + b"\nendobj\n"
    at = len(first) + len(update)
    update += b"xref\n%d 1\n%010d 00000 n \n" % (page, len(first))
    update += ("trailer\n<< /Size %d /Root %d 0 R /Prev %d >>\nstartxref\n%d\n%%%%EOF\n" % (b.next, catalog, prev, at)).encode("latin-1")
    c["prev_chain_indirect_length"] = Case(first + update, [R.render((0, 0, W1, H1), 180, [(shown, upright(W1, H1))])])

    # ---- Pillow's own PDFs ------------------------------------------------------------------------------------------------------------
    def pillow_pdf(ims, **kw):
        f = io.BytesIO()
        ims[0].save(f, "PDF", save_all=len(ims) > 1, append_images=ims[1:], **kw)
        return f.getvalue()

    white = bilevel_image(H4, W4, 80)
    c["pillow_1"] = Case(pillow_pdf([Image.fromarray(white)], resolution=300.0), [bgr(white)])
    a = gray_image(H4, W4, 81)
    pdf = pillow_pdf([Image.fromarray(a)], resolution=300.0)
    c["pillow_L"] = Case(pdf, [pillow_jpeg_pixels(pdf)[0]])
    a = rgb_image(H4, W4, 82)
    pdf = pillow_pdf([Image.fromarray(a)])
    c["pillow_RGB"] = Case(pdf, [pillow_jpeg_pixels(pdf)[0]])
    ims = [Image.fromarray(bilevel_image(H3, W3, 83)), Image.fromarray(gray_image(H1, W1, 84)), Image.fromarray(rgb_image(H2, W2, 85))]
    pdf = pillow_pdf(ims, resolution=150.0)
    jp = pillow_jpeg_pixels(pdf)
    c["pillow_three_pages"] = Case(pdf, [bgr(bilevel_image(H3, W3, 83)), jp[0], jp[1]])

    # ---- refusals -------------------------------------------------------------------------------------------------------------------------
    d, data, shown = raw_gray(H1, W1, 90)
    up = upright(W1, H1)

    def refused(reason, content=None, image=None, **kw):
        page = {"media": (0, 0, W1, H1), "contents": [("", draw("Im0", up) if content is None else content)],
                "images": {"Im0": image or (image_dict(W1, H1, d), data, [])}}
        page.update(kw)
        return Case(simple([page])[0], [reason])

    c["refuse_text"] = refused("operator BT", draw("Im0", up) + b"BT /F1 12 Tf (scanned) Tj ET\n")
    c["refuse_path"] = refused("operator re", b"0 0 10 10 re f\n" + draw("Im0", up))
    c["refuse_inline_image"] = refused("inline image", draw("Im0", up) + b"q 1 0 0 1 0 0 cm BI /W 1 /H 1 /BPC 8 /CS /G ID x EI Q\n")
    c["refuse_form"] = refused("form", draw("Im0", up) + b"/Fm0 Do\n", forms={"Fm0": ("/Type /XObject /Subtype /Form /BBox [0 0 1 1]", b"q Q")})
    c["refuse_gs"] = refused("gs", b"/GS0 gs\n" + draw("Im0", up), resources_extra="/ExtGState << /GS0 << /ca 0.5 >> >>")
    c["refuse_smask"] = refused("SMask", image=(image_dict(W1, H1, d + " /SMask {0} 0 R"), data,
                                                [(image_dict(W1, H1, "/ColorSpace /DeviceGray /BitsPerComponent 8"), data)]))
    cmyk = np.zeros((H1, W1, 4), np.uint8)
    c["refuse_cmyk"] = refused("DeviceCMYK", image=(image_dict(W1, H1, "/ColorSpace /DeviceCMYK /BitsPerComponent 8"), cmyk.tobytes(), []))
    c["refuse_jbig2"] = refused("JBIG2", image=(image_dict(W1, H1, "/ColorSpace /DeviceGray /BitsPerComponent 1 /Filter /JBIG2Decode"), b"\0" * 16, []))
    c["refuse_jpx"] = refused("JPX", image=(image_dict(W1, H1, "/ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /JPXDecode"), b"\0" * 16, []))
    strip = g4(bilevel_image(H1, W1, 91), False)
    ccitt = "/ColorSpace /DeviceGray /BitsPerComponent 1 /Filter /CCITTFaxDecode /DecodeParms << %s /Columns %d /Rows %d >>"
    c["refuse_k0"] = refused("K = 0", image=(image_dict(W1, H1, ccitt % ("/K 0", W1, H1)), strip, []))
    c["refuse_byte_align"] = refused("EncodedByteAlign", image=(image_dict(W1, H1, ccitt % ("/K -1 /EncodedByteAlign true", W1, H1)), strip, []))
    c["refuse_overlap"] = refused("overlap", draw("Im0", up) + draw("Im0", (W1, 0, 0, H1, 5, 5)), media=(0, 0, 2 * W1, 2 * H1))
    c["refuse_resolution"] = refused("resolution", draw("Im0", up) + draw("Im0", (W1 / 2.0, 0, 0, H1 / 2.0, W1, H1)), media=(0, 0, 2 * W1, 2 * H1))
    c["refuse_skew"] = refused("skewed", draw("Im0", (W1, 3, 2, H1, 0, 0)))
    # a refused page beside a good one does not fail the file
    good = {"media": (0, 0, W1, H1), "contents": [("", draw("Im0", up))], "images": {"Im0": (image_dict(W1, H1, d), data, [])}}
    bad = dict(good, contents=[("", b"BT ET\n" + draw("Im0", up))])
    c["refuse_one_page_of_two"] = Case(simple([bad, good])[0], ["operator BT", shown])
    # whole files
    c["error_encrypt"] = Case(simple([good], trailer_extra="/Encrypt << /Filter /Standard /V 1 /R 2 /O (x) /U (y) /P -4 >>")[0], [], error="Encrypt")
    b = Builder()
    catalog, tree = b.reserve(), b.reserve()
    b.put("<< /Type /Catalog /Pages %d 0 R >>" % tree, catalog)
    b.put("<< /Type /Pages /Count 1 /Kids [%d 0 R] >>" % tree, tree)
    c["error_cyclic_kids"] = Case(b.finish(catalog), [], error="Kids")
    pdf = simple([good])[0]
    at = int(pdf[pdf.rindex(b"startxref") + 9:].split()[0])
    c["error_cyclic_prev"] = Case(pdf.replace(b"trailer\n<< ", b"trailer\n<< /Prev %d " % at), [], error="Prev")
    return c


@functools.lru_cache(maxsize=None)
def compose_grid():
    """The compose step's grid: all eight orientations x invert x the five sizes x five offsets (inside, and hanging over the left,
    top, right and bottom edge by up to 3 pixels), every item on a page of its own, two pixels larger than the oriented image each
    way.  -> (pages [(H, W)], items [(S, code, invert, page, x, y, crop_x, crop_y, crop_w, crop_h)])."""
    pages, items = [], []
    for h, w in SIZES:
        S = np.ascontiguousarray(rgb_image(h, w, 100 + h)[:, :, ::-1])
        for code in range(1, 9):
            oh, ow = (w, h) if code >= 5 else (h, w)
            H, W = oh + 2, ow + 2
            kx, ky = min(3, ow - 1), min(3, oh - 1)
            for invert in (0, 1):
                for left, top in ((1, 1), (-kx, 1), (1, -ky), (W - ow + kx, 1), (1, H - oh + ky)):
                    x, y, cx, cy = max(left, 0), max(top, 0), max(-left, 0), max(-top, 0)
                    cw, ch = min(left + ow, W) - x, min(top + oh, H) - y
                    items.append((S, code, invert, len(pages), x, y, cx, cy, cw, ch))
                    pages.append((H, W))
    small, square, dot = (np.ascontiguousarray(rgb_image(h, w, 120 + h)[:, :, ::-1]) for h, w in SIZES[1:3] + SIZES[:1])
    # a page that three items of different sizes leave partly uncovered, then one that two items cover exactly (no fill)
    items += [(small, 6, 0, len(pages), 0, 0, 0, 0, 33, 31), (square, 3, 1, len(pages), 40, 10, 0, 0, 64, 64), (dot, 1, 0, len(pages), 149, 99, 0, 0, 1, 1)]
    pages.append((100, 150))
    items += [(small, 1, 0, len(pages), 0, 0, 0, 0, 31, 33), (small, 2, 1, len(pages), 31, 0, 0, 0, 31, 33)]
    pages.append((33, 62))
    return pages, items


def pillow_jpeg_pixels(pdf):
    """Pillow's decode of every JPEG embedded in a PDF it wrote, in file order, as B,G,R."""
    out, pos = [], 0
    while True:
        at = pdf.find(b"\xff\xd8\xff", pos)
        if at < 0:
            return out
        end = pdf.index(b"endstream", at)
        with Image.open(io.BytesIO(pdf[at:end])) as im:
            out.append(np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1]))
        pos = end
