"""Reference helper of the TIFF tests (no test here): a small TIFF writer that wraps given strip bytes into one IFD (either byte order,
SHORT or LONG fields, any photometric / fill order / predictor / rows per strip, extra tags), pure-Python PackBits and TIFF-LZW
encoders and decoders (the LZW decoder counts Clear codes, KwKwK codes and width changes), and a corpus builder over Pillow's writer."""
import io
import struct
import warnings
import zlib

import numpy as np
from PIL import Image

SHORT, LONG = 3, 4
COMPRESSIONS = {"raw": 1, "packbits": 32773, "tiff_lzw": 5, "tiff_adobe_deflate": 8, "group4": 4}
LAYOUTS = ("1", "L", "P", "RGB")
WIDTHS, HEIGHTS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65), (1, 2, 5, 9)


def pillow_bgr(data):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with Image.open(io.BytesIO(data)) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


# ---- the writer -------------------------------------------------------------------------------------------------------------------------
def write_tiff(strips, width, height, rows_per_strip, compression=1, bits=(8,), photometric=1, samples=None, fill_order=None, predictor=None,
               colormap=None, big_endian=False, long_fields=False, extra=(), omit=()):
    """One classic TIFF: header, the strips, the out-of-line values, the IFD.  strips: list of bytes.  Dimensions, offsets and byte
    counts are LONG if long_fields else SHORT (offsets and counts that do not fit a SHORT are LONG anyway); arrays of more than 4
    bytes go by offset, as the specification says.  extra: (tag, type, values) triples (they replace a standard tag of the same
    number); omit: tags to leave out."""
    e = ">" if big_endian else "<"
    dim = LONG if long_fields else SHORT
    samples = len(bits) if samples is None else samples
    out = bytearray((b"MM" if big_endian else b"II") + struct.pack(e + "HI", 42, 0))
    offsets = []
    for s in strips:
        if len(out) & 1:
            out += b"\0"
        offsets.append(len(out))
        out += s
    big = long_fields or max(offsets + [len(s) for s in strips] + [0]) > 65535
    tags = {256: (dim, [width]), 257: (dim, [height]), 258: (SHORT, list(bits)), 259: (SHORT, [compression]), 262: (SHORT, [photometric]),
            273: (LONG if big else SHORT, offsets), 277: (SHORT, [samples]), 278: (dim, [rows_per_strip]),
            279: (LONG if big else SHORT, [len(s) for s in strips])}
    if fill_order is not None:
        tags[266] = (SHORT, [fill_order])
    if predictor is not None:
        tags[317] = (SHORT, [predictor])
    if colormap is not None:
        tags[320] = (SHORT, list(colormap))
    for tag, typ, values in extra:
        tags[tag] = (typ, list(values))
    for tag in omit:
        tags.pop(tag, None)
    entries = []
    for tag in sorted(tags):
        typ, values = tags[tag]
        fmt = {1: "B", 2: "B", SHORT: "H", LONG: "I"}[typ]
        raw = struct.pack(e + fmt * len(values), *values)
        if len(raw) <= 4:
            field = raw.ljust(4, b"\0")
        else:
            if len(out) & 1:
                out += b"\0"
            field = struct.pack(e + "I", len(out))
            out += raw
        entries.append(struct.pack(e + "HHI", tag, typ, len(values)) + field)
    if len(out) & 1:
        out += b"\0"
    struct.pack_into(e + "I", out, 4, len(out))
    out += struct.pack(e + "H", len(entries)) + b"".join(entries) + struct.pack(e + "I", 0)
    return bytes(out)


def read_fields(data):
    """{tag: (type, [values])} of the first IFD of a file the writers here (or Pillow) wrote, and the byte order mark."""
    e = ">" if data[:2] == b"MM" else "<"
    ifd, = struct.unpack_from(e + "I", data, 4)
    n, = struct.unpack_from(e + "H", data, ifd)
    fields = {}
    for k in range(n):
        tag, typ, count = struct.unpack_from(e + "HHI", data, ifd + 2 + 12 * k)
        size = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 7: 1}.get(typ, 1) * count
        at = ifd + 2 + 12 * k + 8
        if size > 4:
            at, = struct.unpack_from(e + "I", data, at)
        fmt = {1: "B", 3: "H", 4: "I"}.get(typ)
        fields[tag] = (typ, list(struct.unpack_from(e + fmt * count, data, at)) if fmt else data[at:at + size])
    return fields


def rewrap(data, big_endian=False, long_fields=False, extra=(), omit=()):
    """The strips and the pixel tags of a file (Pillow's) in a new file of another byte order or field width."""
    f = read_fields(data)
    one = lambda tag, absent=None: f[tag][1][0] if tag in f else absent  # noqa: E731
    strips = [data[o:o + c] for o, c in zip(f[273][1], f[279][1])]
    return write_tiff(strips, one(256), one(257), one(278, one(257)), compression=one(259, 1), bits=tuple(f[258][1]) if 258 in f else (1,),
                      photometric=one(262), samples=one(277, 1), fill_order=one(266), predictor=one(317),
                      colormap=f[320][1] if 320 in f else None, big_endian=big_endian, long_fields=long_fields, extra=extra, omit=omit)


# ---- PackBits ---------------------------------------------------------------------------------------------------------------------------
def packbits_encode(data):
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        j = i
        while j + 1 < n and data[j + 1] == data[i] and j - i < 127:
            j += 1
        if j > i:
            out += bytes([257 - (j - i + 1), data[i]])
            i = j + 1
            continue
        j = i
        while j < n and j - i < 128 and not (j + 2 < n and data[j] == data[j + 1] == data[j + 2]):
            j += 1
        out += bytes([j - i - 1]) + bytes(data[i:j])
        i = j
    return bytes(out)


def packbits_decode(data, want):
    out, i = bytearray(), 0
    while len(out) < want:
        n = data[i]
        i += 1
        if n == 128:
            continue
        if n > 128:
            out += bytes([data[i]]) * (257 - n)
            i += 1
        else:
            out += data[i:i + n + 1]
            i += n + 1
    assert len(out) == want
    return bytes(out)


# ---- TIFF-LZW (MSB first, early change) ----------------------------------------------------------------------------------------------------
class _BitsOut:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, width):
        self.acc = (self.acc << width) | code
        self.n += width
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 255)
        return bytes(self.out)


def lzw_encode(data, eoi=True):
    """What libtiff's encoder writes: Clear first, a Clear when entry 4093 has been made, the width raised one code early."""
    w = _BitsOut()
    table, nxt, width = {}, 258, 9
    w.put(256, 9)
    omega = b""
    for k in range(len(data)):
        ch = data[k:k + 1]
        if not omega or omega + ch in table:
            omega = omega + ch
            continue
        w.put(table[omega] if len(omega) > 1 else omega[0], width)
        table[omega + ch] = nxt
        nxt += 1
        omega = ch
        if nxt == 4094:
            w.put(256, width)
            table, nxt, width = {}, 258, 9
        elif nxt >= (1 << width):
            width += 1
    if omega:
        w.put(table[omega] if len(omega) > 1 else omega[0], width)
        nxt += 1
        if nxt >= (1 << width) and width < 12:
            width += 1
    if eoi:
        w.put(257, width)
    return w.done()


def lzw_decode(data, want):
    """(bytes, stats) with stats = {"clears", "kwkwk", "widths": set of the widths codes were read at}."""
    stats = {"clears": 0, "kwkwk": 0, "widths": set()}
    out = bytearray()
    bit, width, table, prev = 0, 9, [], None
    while len(out) < want:
        assert bit + width <= 8 * len(data), "the strip ends before its rows are full"
        code = (int.from_bytes(data[bit >> 3:(bit >> 3) + 3].ljust(3, b"\0"), "big") >> (24 - width - (bit & 7))) & ((1 << width) - 1)
        stats["widths"].add(width)
        bit += width
        if code == 257:
            break
        if code == 256:
            stats["clears"] += 1
            table, width, prev = [], 9, None
            continue
        assert stats["clears"], "a code before the first Clear"
        if prev is None:
            assert code < 256
            s = bytes([code])
        else:
            if code < 256:
                s = bytes([code])
            elif code - 258 < len(table):
                s = table[code - 258]
            else:
                assert code - 258 == len(table), "code above the next free one"
                stats["kwkwk"] += 1
                s = prev + prev[:1]
            table.append(prev + s[:1])
            if 258 + len(table) > (1 << width) - 2 and width < 12:
                width += 1
        out += s
        prev = s
    assert len(out) == want
    return bytes(out), stats


# ---- pages and the corpus -----------------------------------------------------------------------------------------------------------------
def random_image(rng, mode, w, h, density=0.5):
    if mode == "1":
        return Image.fromarray(rng.random_sample((h, w)) < density)
    if mode == "L":
        return Image.fromarray(rng.randint(0, 256, (h, w)).astype(np.uint8))
    if mode == "P":
        im = Image.fromarray(rng.randint(0, 256, (h, w)).astype(np.uint8)).convert("P")
        im.putpalette(rng.randint(0, 256, 768).astype(np.uint8).tobytes())
        return im
    return Image.fromarray((rng.randint(0, 6, (h, w, 3)) * 50).astype(np.uint8))


def pillow_tiff(im, compression, tiffinfo=None):
    """Pillow's file of an image; tiffinfo by tag number: 262 photometric, 266 fill order, 278 rows per strip, 317 predictor."""
    b = io.BytesIO()
    im.save(b, "TIFF", compression=compression, tiffinfo=dict(tiffinfo or {}))
    return b.getvalue()


def rows_per_strip_values(h):
    return (1, 2, 3, h, h + 7)


def applies(compression, mode, predictor):
    if compression == "group4" and mode != "1":
        return False
    if predictor == 2 and (compression not in ("tiff_lzw", "tiff_adobe_deflate") or mode in ("1", "P")):
        return False                                                     # libtiff applies a predictor under LZW and Deflate only
    return True


def corpus(compression, seed=0):
    """[(label, file bytes)] of one compression kind: every layout it applies to x WIDTHS x HEIGHTS x rows per strip 1, 2, 3, height,
    height + 7, with photometric 0 / 1, fill order 1 / 2, predictor 1 / 2, byte order and field width taking turns so that every
    value meets every layout, width and strip size.  Written by Pillow, then wrapped again by write_tiff."""
    rng = np.random.RandomState(seed)
    files, k = [], 0
    for mode in LAYOUTS:
        if not applies(compression, mode, 1):
            continue
        for w in WIDTHS:
            for h in HEIGHTS:
                im = random_image(rng, mode, w, h)
                for rps in rows_per_strip_values(h):
                    k += 1
                    info = {278: rps}
                    if mode in ("1", "L"):
                        info[262] = (k // 2) & 1
                    if mode == "1" and k % 3 == 0:
                        info[266] = 2
                    if applies(compression, mode, 2) and k % 2:
                        info[317] = 2
                    data = rewrap(pillow_tiff(im, compression, info), big_endian=bool((k // 3) & 1), long_fields=bool((k // 5) & 1))
                    files.append(("%s %s %dx%d rps %d %r %s" % (compression, mode, w, h, rps, info, data[:2].decode()), data))
    return files


def sample_tiffs(jpeg_path):
    """{kind: file} of the golden sample page as the benchmark's kinds (tools/bench_decode_tiff.py)."""
    with Image.open(jpeg_path) as im:
        rgb = im.convert("RGB")
    gray = rgb.convert("L")
    bw = gray.point(lambda v: 255 if v > 128 else 0).convert("1")
    return {
        "g4": pillow_tiff(bw, "group4"),
        "g4_one_strip": pillow_tiff(bw, "group4", {278: bw.size[1]}),
        "packbits_bilevel": pillow_tiff(bw, "packbits"),
        "lzw_gray": pillow_tiff(gray, "tiff_lzw"),
        "lzw_rgb_predictor": pillow_tiff(rgb, "tiff_lzw", {317: 2}),
        "deflate_rgb": pillow_tiff(rgb, "tiff_adobe_deflate"),
        "raw_rgb": pillow_tiff(rgb, "raw"),
    }


def zlib_strip(raw):
    return zlib.compress(raw, 6)
