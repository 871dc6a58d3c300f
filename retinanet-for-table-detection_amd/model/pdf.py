"""Scanned PDFs, read on the device: the reference starts from PDFs (convertPdfsToImages rasterises them,
PDFCSVtoImageCSV maps PDF ground truth to image coordinates); an image-only page is already one of the streams page_io decodes.
This module is the container (a PDF object parser, host, Python), the rules for what a page may look like, the step that puts the
decoded images onto the page (csrc/rtn_compose.hip) and the way from a detection box back to PDF points.  There is no rasteriser
and no new decoder: every image stream is wrapped as a file held in memory and goes through page_io._decode_datas.

The parser reads the header, classic cross-reference tables, cross-reference streams and object streams (PDF 1.5), /Prev chains and
hybrid /XRefStm sections, indirect /Length, the page tree with inherited /MediaBox, /Rotate and /Resources, /Contents as one stream
or an array, and the filters FlateDecode, ASCIIHexDecode and ASCII85Decode on content streams.  Every failure is PdfError (a
ValueError) with a reason; /Prev, /Kids and indirect chains are walked with visited sets.  A file whose trailer has /Encrypt is
refused as a whole.

A page is taken only if it is image-only: its content holds nothing but q, Q, cm, Do on image XObjects, the colour operators g G
rg RG and the marked-content operators BMC BDC EMC MP DP.  Any other operator (text, paths, shading, inline images, Do on a form,
gs) refuses the page, with the operator named; a refused page is reported (PdfPage.refused) and does not fail the file.

An image has /BitsPerComponent 1 or 8 (2, 4 and 16 are wrapped too and left to whoever takes the file); /ColorSpace DeviceGray or
DeviceRGB, CalGray, CalRGB or ICCBased with N = 1 or 3 TAKEN AS THE DEVICE SPACES (no colour management), or Indexed over one of
those with the lookup as a string or a stream; /ImageMask true while the fill colour is black (a 1-bit gray image on white);
/Decode default or fully reversed.  /SMask, /Mask, DeviceCMYK, JBIG2Decode, JPXDecode, /EncodedByteAlign true and CCITTFaxDecode
with K >= 0 refuse the page.  ASCIIHexDecode, ASCII85Decode or FlateDecode in front of the last filter are undone on the host.

  PDF stream                                   file in memory
  DCTDecode                                    the JPEG as it is
  CCITTFaxDecode, K < 0                        one-strip Group 4 TIFF; photometric from BlackIs1, /Decode and the colour space
  FlateDecode, predictor >= 10                 PNG (IHDR, PLTE from the Indexed lookup, the stream as one IDAT, IEND; CRCs made here)
  FlateDecode / LZWDecode, predictor 1 or 2    one-strip TIFF, compression 8 / 5 (LZW with EarlyChange 1 only)
  unfiltered                                   one-strip TIFF, compression 1

Page geometry.  Image space is the unit square with the image's first row at y = 1.  The concatenated CTM [a b c d e f] of each Do
must be a quarter turn and / or a mirror: |b|, |c| <= 1e-6 max(|a|, |d|), or the same with the roles swapped; it maps to one of the
eight TIFF / EXIF orientation codes.  The page's scale (sx, sy, pixels per point) comes from the first painted image: its oriented
pixel width and height over its extent in points.  The canvas is W = round(mediabox_w sx) by H = round(mediabox_h sy) pixels with
row 0 at the top of the MediaBox (round: half up).  Every image's destination rectangle comes from rounding both of its corners at
the page's scale and must have exactly the image's oriented pixel size ("image resolution differs from the page's" otherwise).
Rectangles are clipped to the canvas; two images whose clipped rectangles overlap refuse the page (layered / MRC scans); uncovered
canvas is 255.  /Rotate (any multiple of 90, negative ones too) then turns the canvas clockwise.  /CropBox and /UserUnit are
IGNORED: the page is its MediaBox at 1/72 inch per unit."""
import base64
import ctypes as C
import io
import math
import os
import re
import struct
import zlib
from collections import namedtuple

import numpy as np
import torch

from . import _rt, page_io

L = _rt.L

PDF_G4_MIN_DEFAULT = 16


def pdf_g4_min():
    """RTN_PDF_G4_MIN: the fewest Group 4 images of more than 64 rows in one strip (the normal form inside a PDF) in one call for
    which those are decoded on the device, one serial decoder per image (rtn_tiff_inspect_flags with RTN_TIFF_ALLOW_G4_ONE_STRIP);
    0 leaves them all to Pillow.  The default, 16, is the batch at which that decoder first beat Pillow on one thread on
    sample-sized pages (profiles/tiff_decode_bench.txt; measured again through this module in
    profiles/pdf_read_bench.txt)."""
    try:
        return max(0, int(os.environ.get("RTN_PDF_G4_MIN", "") or PDF_G4_MIN_DEFAULT))
    except ValueError:
        return PDF_G4_MIN_DEFAULT


class PdfError(ValueError):
    """A PDF this module cannot read, with the reason."""


class _Refused(Exception):
    """A page this module does not take, with the reason (becomes PdfPage.refused)."""


# ---- objects ------------------------------------------------------------------------------------------------------------------------------
class Name(str):
    pass


class Ref(namedtuple("Ref", "num gen")):
    pass


class Stream:
    def __init__(self, d, raw):
        self.d, self.raw = d, raw


class _Op(str):
    """A keyword of a content stream or of the file structure (obj, R, stream, q, cm, ...)."""


_WS = b"\x00\t\n\x0c\r "
_MAX_DEPTH = 64
_MAX_INFLATE = 1 << 28            # bytes one host-side inflate may give (content, object and cross-reference streams)
_NUM = re.compile(rb"[+-]?(\d+\.?\d*|\.\d+)")
_SKIP = re.compile(rb"[\x00\t\n\x0c\r ]*(?:%[^\r\n]*[\x00\t\n\x0c\r ]*)*")
_WORD = re.compile(rb"[^\x00\t\n\x0c\r ()<>\[\]{}/%]*")


class _Lexer:
    def __init__(self, data, pos=0):
        self.d, self.p = data, pos

    def skip(self):
        self.p = _SKIP.match(self.d, self.p).end()               # white space and % comments to the end of their lines

    def token(self):
        """The next object or keyword; None at the end of the data."""
        self.skip()
        d, n, p = self.d, len(self.d), self.p
        if p >= n:
            return None
        c = d[p]
        if c == 0x2f:                                            # /Name
            self.p = q = _WORD.match(d, p + 1).end()
            raw = d[p + 1:q]
            if b"#" in raw:
                raw = re.sub(rb"#([0-9A-Fa-f]{2})", lambda m: bytes([int(m.group(1), 16)]), raw)
            return Name(raw.decode("latin-1"))
        if c == 0x28:
            return self._literal()
        if c == 0x3c:
            if d[p + 1:p + 2] == b"<":
                self.p = p + 2
                return _Op("<<")
            q = d.find(b">", p)
            if q < 0:
                raise PdfError("a hex string without its end")
            self.p = q + 1
            return _hex(d[p + 1:q])
        if c == 0x3e:
            if d[p + 1:p + 2] == b">":
                self.p = p + 2
                return _Op(">>")
            raise PdfError("a stray '>' at byte %d" % p)
        if c in b"[]{}":
            self.p = p + 1
            return _Op(chr(c))
        if c == 0x29:
            raise PdfError("a stray ')' at byte %d" % p)
        self.p = q = _WORD.match(d, p).end()
        word = d[p:q]
        if _NUM.fullmatch(word):
            try:
                return int(word) if word.lstrip(b"+-").isdigit() else float(word)
            except ValueError:
                raise PdfError("a bad number %r" % word[:20])
        return _Op(word.decode("latin-1"))

    def _literal(self):
        d, n = self.d, len(self.d)
        p, depth, out = self.p + 1, 1, bytearray()
        esc = {0x6e: 10, 0x72: 13, 0x74: 9, 0x62: 8, 0x66: 12}
        while p < n:
            c = d[p]
            if c == 0x5c and p + 1 < n:
                e = d[p + 1]
                if e in esc:
                    out.append(esc[e])
                    p += 2
                elif 0x30 <= e <= 0x37:
                    q = p + 1
                    while q < min(p + 4, n) and 0x30 <= d[q] <= 0x37:
                        q += 1
                    out.append(int(d[p + 1:q], 8) & 255)
                    p = q
                elif e in b"\r\n":
                    p += 3 if d[p + 1:p + 3] == b"\r\n" else 2
                else:
                    out.append(e)
                    p += 2
                continue
            if c == 0x28:
                depth += 1
            elif c == 0x29:
                depth -= 1
                if depth == 0:
                    self.p = p + 1
                    return bytes(out)
            out.append(c)
            p += 1
        raise PdfError("a string without its end")

    def obj(self, depth=0):
        """The next object: arrays and dictionaries built, `n g R` folded into a Ref; a keyword comes back as an _Op."""
        t = self.token()
        if t is None:
            raise PdfError("the data ends inside an object")
        if not isinstance(t, _Op):
            return t
        if depth > _MAX_DEPTH:
            raise PdfError("objects nested deeper than %d" % _MAX_DEPTH)
        if t == "[":
            out = []
            while True:
                v = self.obj(depth + 1)
                if isinstance(v, _Op):
                    if v == "]":
                        return out
                    if v == "R" and len(out) >= 2 and _is_int(out[-1]) and _is_int(out[-2]):
                        gen, num = out.pop(), out.pop()
                        out.append(Ref(num, gen))
                        continue
                    raise PdfError("%r inside an array" % str(v)[:20])
                out.append(v)
        if t == "<<":
            items = []
            while True:
                v = self.obj(depth + 1)
                if isinstance(v, _Op):
                    if v == ">>":
                        break
                    if v == "R" and len(items) >= 2 and _is_int(items[-1]) and _is_int(items[-2]):
                        gen, num = items.pop(), items.pop()
                        items.append(Ref(num, gen))
                        continue
                    raise PdfError("%r inside a dictionary" % str(v)[:20])
                items.append(v)
            if len(items) % 2:
                raise PdfError("a dictionary with a key and no value")
            out = {}
            for k, v in zip(items[0::2], items[1::2]):
                if not isinstance(k, Name):
                    raise PdfError("a dictionary key that is no name")
                out[str(k)] = v
            return out
        if t == "true":
            return True
        if t == "false":
            return False
        if t == "null":
            return None
        return t


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _is_num(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def _hex(raw):
    s = bytes(c for c in raw if c not in _WS)
    if len(s) % 2:
        s += b"0"
    try:
        return bytes.fromhex(s.decode("ascii"))
    except (ValueError, UnicodeDecodeError):
        raise PdfError("a hex string with other characters")


# ---- host-side stream filters -------------------------------------------------------------------------------------------------------------
def _inflate(data, limit=_MAX_INFLATE):
    try:
        z = zlib.decompressobj()
        out = z.decompress(data, limit)
        if z.unconsumed_tail:
            raise PdfError("a Flate stream of more than %d bytes" % limit)
        return out
    except zlib.error as e:
        raise PdfError("a broken Flate stream: %s" % e)


def _unpredict(data, parms):
    """The rows of a host-decoded Flate stream with /Predictor >= 10 (cross-reference and object streams use it)."""
    pred = parms.get("Predictor", 1)
    if pred in (None, 1):
        return data
    if not _is_int(pred) or pred < 10:
        raise PdfError("predictor %r on a stream decoded on the host" % (pred,))
    colors, bits, cols = parms.get("Colors", 1), parms.get("BitsPerComponent", 8), parms.get("Columns", 1)
    if not (_is_int(colors) and _is_int(bits) and _is_int(cols) and 1 <= colors <= 4 and bits == 8 and 1 <= cols <= 1 << 20):
        raise PdfError("predictor parameters of a stream decoded on the host")
    bpp, row = colors, colors * cols
    n = len(data) // (row + 1)
    a = np.frombuffer(data[:n * (row + 1)], np.uint8).reshape(n, row + 1)
    out = np.zeros((n, row), np.uint8)
    prev = np.zeros(row, np.int64)
    for y in range(n):
        ft, cur = int(a[y, 0]), a[y, 1:].astype(np.int64)
        if ft == 0:
            pass
        elif ft == 2:
            cur = (cur + prev) & 255
        elif ft in (1, 3, 4):
            for x in range(row):
                left = cur[x - bpp] if x >= bpp else 0
                up = prev[x]
                ul = prev[x - bpp] if x >= bpp else 0
                if ft == 1:
                    add = left
                elif ft == 3:
                    add = (left + up) >> 1
                else:
                    pa, pb, pc = abs(up - ul), abs(left - ul), abs(left + up - 2 * ul)
                    add = left if pa <= pb and pa <= pc else (up if pb <= pc else ul)
                cur[x] = (cur[x] + add) & 255
        else:
            raise PdfError("row filter %d in a predicted stream" % ft)
        out[y] = cur
        prev = cur
    return out.tobytes()


def _filters(doc, d):
    """[(filter name, parms dict)] of a stream dictionary; names and parms given alone or as arrays."""
    f = doc.resolve(d.get("Filter"))
    p = doc.resolve(d.get("DecodeParms", d.get("DP")))
    if f is None:
        return []
    fs = [doc.resolve(x) for x in f] if isinstance(f, list) else [f]
    ps = [doc.resolve(x) for x in p] if isinstance(p, list) else [p] * len(fs)
    if len(ps) != len(fs):
        raise PdfError("%d /DecodeParms for %d filters" % (len(ps), len(fs)))
    out = []
    for name, parms in zip(fs, ps):
        if not isinstance(name, Name):
            raise PdfError("a /Filter that is no name")
        if parms is not None and not isinstance(parms, dict):
            raise PdfError("/DecodeParms that is no dictionary")
        out.append((str(name), {k: doc.resolve(v) for k, v in (parms or {}).items()}))
    return out


def _undo(name, parms, data):
    """One of the three filters undone on the host."""
    if name in ("FlateDecode", "Fl"):
        return _unpredict(_inflate(data), parms)
    if name in ("ASCIIHexDecode", "AHx"):
        end = data.find(b">")
        return _hex(data if end < 0 else data[:end])
    if name in ("ASCII85Decode", "A85"):
        end = data.find(b"~>")
        body = bytes(c for c in (data if end < 0 else data[:end]) if c not in _WS)
        try:
            return base64.a85decode(body)
        except ValueError as e:
            raise PdfError("a broken ASCII85 stream: %s" % e)
    raise PdfError("filter /%s on a stream decoded on the host" % name)


# ---- the file -------------------------------------------------------------------------------------------------------------------------------
class _Doc:
    def __init__(self, data):
        if not isinstance(data, (bytes, bytearray, memoryview)):
            raise PdfError("bytes expected, got %s" % type(data).__name__)
        self.data = data = bytes(data)
        if b"%PDF-" not in data[:1024]:
            raise PdfError("no %PDF- header")
        self.xref, self.cache, self.loading = {}, {}, set()
        self.trailer = None
        self._read_xrefs()
        if self.trailer is None:
            raise PdfError("no trailer")
        if self.trailer.get("Encrypt") is not None:
            raise PdfError("the file is encrypted (/Encrypt)")

    # -- cross-reference ----------------------------------------------------------------------------------------------------------------
    def _read_xrefs(self):
        data = self.data
        at = data.rfind(b"startxref", max(0, len(data) - 2048))
        if at < 0:
            raise PdfError("no startxref in the last 2048 bytes")
        pos = _Lexer(data, at + 9).token()
        seen, queue = set(), [pos]
        while queue:
            pos = queue.pop(0)
            if not _is_int(pos) or not 0 <= pos < len(data):
                raise PdfError("a cross-reference section outside the file")
            if pos in seen:
                raise PdfError("the /Prev chain loops")
            seen.add(pos)
            lx = _Lexer(data, pos)
            lx.skip()
            if data[lx.p:lx.p + 4] == b"xref":
                lx.p += 4
                trailer = self._xref_table(lx)
            else:
                trailer = self._xref_stream(lx)
            if self.trailer is None:
                self.trailer = trailer
            for key in ("XRefStm", "Prev"):
                if trailer.get(key) is not None:
                    queue.append(trailer[key])

    def _xref_table(self, lx):
        data = self.data
        while True:
            t = lx.token()
            if isinstance(t, _Op) and t == "trailer":
                break
            count = lx.token()
            if not (_is_int(t) and _is_int(count) and t >= 0 and 0 <= count <= (len(data) - lx.p) // 18 + 1):
                raise PdfError("a broken cross-reference table")
            for k in range(count):
                off, gen, kind = lx.token(), lx.token(), lx.token()
                if not (_is_int(off) and _is_int(gen) and isinstance(kind, _Op) and kind in ("n", "f")):
                    raise PdfError("a broken cross-reference entry")
                if kind == "n" and t + k not in self.xref:
                    self.xref[t + k] = (1, off, gen)
        trailer = lx.obj()
        if not isinstance(trailer, dict):
            raise PdfError("the trailer is no dictionary")
        return trailer

    def _xref_stream(self, lx):
        st = self._object_at(lx, None)
        if not isinstance(st, Stream) or st.d.get("Type") != "XRef":
            raise PdfError("startxref points at neither a table nor a cross-reference stream")
        d = st.d
        w, size = d.get("W"), d.get("Size")
        if not (isinstance(w, list) and len(w) == 3 and all(_is_int(x) and 0 <= x <= 8 for x in w) and _is_int(size) and sum(w) > 0):
            raise PdfError("a broken cross-reference stream dictionary")
        index = d.get("Index", [0, size])
        if not (isinstance(index, list) and len(index) % 2 == 0 and all(_is_int(x) and x >= 0 for x in index)):
            raise PdfError("a broken /Index")
        body = self.stream_bytes(st)
        step, pos = sum(w), 0
        for first, count in zip(index[0::2], index[1::2]):
            for k in range(count):
                if pos + step > len(body):
                    raise PdfError("a cross-reference stream shorter than its /Index")
                f = []
                for width in w:
                    f.append(int.from_bytes(body[pos:pos + width], "big") if width else None)
                    pos += width
                kind = 1 if f[0] is None else f[0]
                if first + k in self.xref:
                    continue
                if kind == 1:
                    self.xref[first + k] = (1, f[1] or 0, f[2] or 0)
                elif kind == 2:
                    self.xref[first + k] = (2, f[1] or 0, f[2] or 0)
        return d

    # -- objects ------------------------------------------------------------------------------------------------------------------------
    def _object_at(self, lx, want):
        """The indirect object that begins at the lexer's position (`want`: its number, or None for any)."""
        num, gen, kw = lx.token(), lx.token(), lx.token()
        if not (_is_int(num) and _is_int(gen) and isinstance(kw, _Op) and kw == "obj"):
            raise PdfError("no object where the cross-reference says one is")
        if want is not None and num != want:
            raise PdfError("object %d where %d is expected" % (num, want))
        v = lx.obj()
        if isinstance(v, _Op):
            raise PdfError("object %d holds the keyword %r" % (num, str(v)[:20]))
        if not isinstance(v, dict):
            return v
        save = lx.p
        kw = lx.token()
        if not (isinstance(kw, _Op) and kw == "stream"):
            lx.p = save
            return v
        data, p = self.data, lx.p
        if data[p:p + 2] == b"\r\n":
            p += 2
        elif data[p:p + 1] in (b"\n", b"\r"):
            p += 1
        length = self.resolve(v.get("Length"))
        if _is_int(length) and 0 <= length <= len(data) - p and data[p + length:p + length + 20].lstrip(_WS).startswith(b"endstream"):
            raw = data[p:p + length]
        else:
            end = data.find(b"endstream", p)
            if end < 0:
                raise PdfError("stream %d without endstream" % num)
            raw = data[p:end]
            if raw.endswith(b"\r\n"):
                raw = raw[:-2]
            elif raw.endswith((b"\n", b"\r")):
                raw = raw[:-1]
        return Stream(v, raw)

    def get(self, num):
        if num in self.cache:
            return self.cache[num]
        entry = self.xref.get(num)
        if entry is None:
            return None                                          # a reference to an object the file does not have is null
        if num in self.loading:
            raise PdfError("object %d needs itself" % num)
        self.loading.add(num)
        try:
            kind, a, b = entry
            if kind == 1:
                if not 0 <= a < len(self.data):
                    raise PdfError("object %d lies outside the file" % num)
                v = self._object_at(_Lexer(self.data, a), num)
            else:
                v = self._from_object_stream(num, a, b)
        finally:
            self.loading.discard(num)
        self.cache[num] = v
        return v

    def _from_object_stream(self, num, holder, index):
        entry = self.xref.get(holder)
        if entry is None or entry[0] != 1:
            raise PdfError("object stream %d is not a plain object" % holder)
        st = self.get(holder)
        if not isinstance(st, Stream) or st.d.get("Type") != "ObjStm":
            raise PdfError("object %d is no object stream" % holder)
        if not hasattr(st, "table"):
            n, first = self.resolve(st.d.get("N")), self.resolve(st.d.get("First"))
            body = self.stream_bytes(st)
            if not (_is_int(n) and _is_int(first) and 0 <= n <= len(body) and 0 <= first <= len(body)):
                raise PdfError("a broken object stream dictionary")
            lx = _Lexer(body[:first])
            table = []
            for _ in range(n):
                k, off = lx.token(), lx.token()
                if not (_is_int(k) and _is_int(off) and 0 <= off <= len(body) - first):
                    raise PdfError("a broken object stream table")
                table.append((k, first + off))
            st.table, st.body = table, body
        if not 0 <= index < len(st.table) or st.table[index][0] != num:
            raise PdfError("object %d is not where its object stream says" % num)
        v = _Lexer(st.body, st.table[index][1]).obj()
        if isinstance(v, _Op):
            raise PdfError("object %d holds a keyword" % num)
        return v

    def resolve(self, v):
        seen = set()
        while isinstance(v, Ref):
            if v.num in seen:
                raise PdfError("an indirect chain loops at object %d" % v.num)
            seen.add(v.num)
            v = self.get(v.num)
        return v

    def stream_bytes(self, st):
        """A stream decoded on the host: Flate (with a PNG predictor), ASCIIHex, ASCII85."""
        data = st.raw
        for name, parms in _filters(self, st.d):
            data = _undo(name, parms, data)
        return data

    # -- pages ----------------------------------------------------------------------------------------------------------------------------
    def pages(self):
        """[(page dictionary, inherited MediaBox, Rotate, Resources)] in page order."""
        root = self.resolve(self.trailer.get("Root"))
        if not isinstance(root, dict):
            raise PdfError("no /Root")
        top = self.resolve(root.get("Pages"))
        if not isinstance(top, dict):
            raise PdfError("no /Pages")
        out, seen = [], set()
        stack = [(root.get("Pages"), {})]
        while stack:
            ref, inherited = stack.pop()
            if isinstance(ref, Ref):
                if ref.num in seen:
                    raise PdfError("the page tree loops at object %d (/Kids)" % ref.num)
                seen.add(ref.num)
            node = self.resolve(ref)
            if not isinstance(node, dict):
                raise PdfError("a page tree node that is no dictionary")
            inh = dict(inherited)
            for key in ("MediaBox", "Rotate", "Resources"):
                if key in node:
                    inh[key] = node[key]
            kids = self.resolve(node.get("Kids"))
            if node.get("Type") == "Pages" or (kids is not None and node.get("Type") != "Page"):
                if not isinstance(kids, list):
                    raise PdfError("a /Pages node without /Kids")
                if len(out) + len(stack) + len(kids) > 1 << 20:
                    raise PdfError("more than 1048576 pages")
                stack.extend((k, inh) for k in reversed(kids))
            else:
                out.append((node, inh))
        return out


# ---- what a page holds ----------------------------------------------------------------------------------------------------------------------
PdfImage = namedtuple("PdfImage", "filter width height bits orientation rect crop invert route")
PdfImage.__doc__ = """An image of a page: the last filter's name ("" for none), the stored sides, bits per component, the orientation
code of its CTM and the page's /Rotate together, rect = (x, y, w, h) of its clipped destination rectangle on the page as read (after
/Rotate), crop = (x, y) of that rectangle's top-left in the oriented image (0, 0 unless the MediaBox cuts it), invert, and route:
"device" or "host" once read (None from pdf_inspect)."""


class PdfPage:
    """A page of a PdfInfo: index, pixel width and height after /Rotate, sx and sy (pixels per point), rotate (0, 90, 180, 270),
    media_box (x0, y0, x1, y1), refused (None or the reason) and images (PdfImage)."""

    def __init__(self, index):
        self.index, self.width, self.height, self.sx, self.sy, self.rotate = index, 0, 0, 0.0, 0.0, 0
        self.media_box, self.refused, self.images = None, None, []
        self._items = []

    def __repr__(self):
        return "PdfPage(%d, %dx%d, refused=%r, %d images)" % (self.index, self.width, self.height, self.refused, len(self.images))


class PdfInfo:
    """pdf_inspect's result: pages (PdfPage, in page order)."""

    def __init__(self, pages):
        self.pages = pages


_CONTENT_OPS = {"q", "Q", "cm", "Do", "g", "G", "rg", "RG", "BMC", "BDC", "EMC", "MP", "DP"}
_Item = namedtuple("_Item", "file filter w h bits orientation invert box g4_one_strip")     # box: (xmin, ymin, xmax, ymax) in points


def _mul(m, n):
    """The matrix of `m` applied first, then `n` (PDF's row-vector order)."""
    a, b, c, d, e, f = m
    A, B, Cc, D, E, F = n
    return (a * A + b * Cc, a * B + b * D, c * A + d * Cc, c * B + d * D, e * A + f * Cc + E, e * B + f * D + F)


def _round(v):
    return int(math.floor(v + 0.5))


def _orientation(m):
    """(code, (xmin, ymin, xmax, ymax)) of a Do under the CTM m, or _Refused."""
    a, b, c, d, e, f = m
    if not all(math.isfinite(v) for v in m):
        raise _Refused("a CTM that is not finite")
    if max(abs(b), abs(c)) <= 1e-6 * max(abs(a), abs(d)) and a != 0 and d != 0:
        code = (1 if a > 0 else 2) if d > 0 else (4 if a > 0 else 3)
        xs, ys = (e, e + a), (f, f + d)
    elif max(abs(a), abs(d)) <= 1e-6 * max(abs(b), abs(c)) and b != 0 and c != 0:
        code = (5 if c < 0 else 6) if b < 0 else (8 if c < 0 else 7)
        xs, ys = (e, e + c), (f, f + b)
    else:
        raise _Refused("a skewed CTM [%g %g %g %g]: only quarter turns and mirrors are taken" % (a, b, c, d))
    return code, (min(xs), min(ys), max(xs), max(ys))


def _colour_space(doc, cs, resources, depth=0):
    """("gray" | "rgb", None) or ("indexed", (base, hival, lookup bytes)), or _Refused."""
    cs = doc.resolve(cs)
    if isinstance(cs, Name) and cs not in ("DeviceGray", "DeviceRGB", "DeviceCMYK", "Pattern") and depth == 0:
        named = doc.resolve((doc.resolve(resources.get("ColorSpace")) or {}).get(str(cs))) if isinstance(resources, dict) else None
        if named is not None:
            return _colour_space(doc, named, resources, 1)
    if isinstance(cs, Name):
        if cs == "DeviceGray":
            return "gray", None
        if cs == "DeviceRGB":
            return "rgb", None
        raise _Refused("colour space /%s" % cs)
    if not (isinstance(cs, list) and cs and isinstance(doc.resolve(cs[0]), Name)):
        raise _Refused("a colour space that is neither a name nor an array")
    kind = str(doc.resolve(cs[0]))
    if kind == "CalGray":
        return "gray", None
    if kind == "CalRGB":
        return "rgb", None
    if kind == "ICCBased" and len(cs) >= 2:
        st = doc.resolve(cs[1])
        n = doc.resolve(st.d.get("N")) if isinstance(st, Stream) else None
        if n in (1, 3):
            return ("gray" if n == 1 else "rgb"), None
        raise _Refused("an ICCBased colour space with N = %r%s" % (n, " (CMYK)" if n == 4 else ""))
    if kind == "Indexed" and len(cs) == 4 and depth < 2:
        base, extra = _colour_space(doc, cs[1], resources, 2)
        hival, lookup = doc.resolve(cs[2]), doc.resolve(cs[3])
        if base == "indexed" or not _is_int(hival) or not 0 <= hival <= 255:
            raise _Refused("a broken Indexed colour space")
        if isinstance(lookup, Stream):
            lookup = doc.stream_bytes(lookup)
        if not isinstance(lookup, bytes):
            raise _Refused("an Indexed lookup that is neither a string nor a stream")
        per = 1 if base == "gray" else 3
        if len(lookup) < per * (hival + 1):
            raise _Refused("an Indexed lookup shorter than hival says")
        return "indexed", (base, hival, lookup[:per * (hival + 1)])
    raise _Refused("colour space /%s" % kind)


def _tiff_file(w, h, bits, samples, compression, photometric, strip, predictor=1, colormap=None):
    """A little-endian one-strip TIFF around `strip`."""
    tags = [(256, 4, 1, w), (257, 4, 1, h), (258, 3, samples, None), (259, 3, 1, compression), (262, 3, 1, photometric),
            (273, 4, 1, None), (277, 3, 1, samples), (278, 4, 1, h), (279, 4, 1, len(strip)), (284, 3, 1, 1)]
    if predictor != 1:
        tags.append((317, 3, 1, predictor))
    if colormap is not None:
        tags.append((320, 3, len(colormap), None))
    ifd_bytes = 2 + 12 * len(tags) + 4
    extra = bytearray()
    pos = 8 + ifd_bytes
    bits_at = cmap_at = 0
    if samples > 2:
        bits_at = pos
        extra += struct.pack("<%dH" % samples, *([bits] * samples))
    if colormap is not None:
        cmap_at = pos + len(extra)
        extra += struct.pack("<%dH" % len(colormap), *colormap)
    if len(extra) % 2:
        extra += b"\0"
    strip_at = pos + len(extra)
    out = bytearray(b"II*\0" + struct.pack("<I", 8) + struct.pack("<H", len(tags)))
    for tag, typ, count, value in tags:
        if tag == 258:
            value = bits_at if samples > 2 else (bits | bits << 16 if samples == 2 else bits)
        elif tag == 273:
            value = strip_at
        elif tag == 320:
            value = cmap_at
        out += struct.pack("<HHI", tag, typ, count)
        out += struct.pack("<HH", value & 0xffff, value >> 16) if typ == 3 and count <= 2 else struct.pack("<I", value)
    out += struct.pack("<I", 0) + extra + strip
    return bytes(out)


def _png_chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)


def _png_file(w, h, bits, colour_type, idat, plte=None):
    out = page_io.PNG_SIGNATURE + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bits, colour_type, 0, 0, 0))
    if plte is not None:
        out += _png_chunk(b"PLTE", plte)
    return out + _png_chunk(b"IDAT", idat) + _png_chunk(b"IEND", b"")


def _palette_rgb(base, lookup, bits, reverse):
    """The Indexed lookup as 2^bits R,G,B triples (entries past hival black), reversed for a reversed /Decode."""
    a = np.frombuffer(lookup, np.uint8)
    rgb = np.repeat(a[:, None], 3, axis=1) if base == "gray" else a.reshape(-1, 3)
    full = np.zeros((1 << bits, 3), np.uint8)
    n = min(len(rgb), 1 << bits)
    full[:n] = rgb[:n]
    return full[::-1].copy() if reverse else full


def _image_item(doc, st, resources, fill_black):
    """The file in memory of one image XObject and what the page needs to know of it: an _Item without its box and orientation."""
    d = {k: doc.resolve(v) for k, v in st.d.items() if k not in ("ColorSpace",)}
    w, h = d.get("Width"), d.get("Height")
    if not (_is_int(w) and _is_int(h) and 1 <= w <= 65535 and 1 <= h <= 65535):
        raise _Refused("an image with sides %r x %r" % (w, h))
    if d.get("SMask") is not None:
        raise _Refused("an image with /SMask (soft mask)")
    if d.get("Mask") is not None:
        raise _Refused("an image with /Mask")
    mask = d.get("ImageMask") is True
    bits = 1 if mask and d.get("BitsPerComponent") is None else d.get("BitsPerComponent")
    filters = _filters(doc, st.d)
    names = [n for n, _ in filters]
    for bad, why in (("JBIG2Decode", "JBIG2"), ("JPXDecode", "JPEG 2000 (JPXDecode)")):
        if bad in names:
            raise _Refused("an image coded as %s" % why)
    if mask:
        if bits != 1:
            raise _Refused("an image mask of %r bits" % (bits,))
        if not fill_black:
            raise _Refused("an image mask painted in a colour other than black")
        space, extra = "gray", None
    else:
        if st.d.get("ColorSpace") is None:
            raise _Refused("an image without /ColorSpace")
        space, extra = _colour_space(doc, st.d.get("ColorSpace"), resources)
    if bits not in (1, 2, 4, 8, 16):
        raise _Refused("an image of %r bits per component" % (bits,))
    comps = 3 if space == "rgb" else 1
    dec = d.get("Decode")
    default = [0, (1 << bits) - 1] if space == "indexed" else [0, 1] * comps
    reverse = False
    if dec is not None:
        if not (isinstance(dec, list) and all(_is_num(doc.resolve(v)) for v in dec)):
            raise _Refused("a broken /Decode")
        dec = [float(doc.resolve(v)) for v in dec]
        if dec == [float(v) for v in default]:
            reverse = False
        elif dec == [float(v) for pair in zip(default[1::2], default[0::2]) for v in pair]:
            reverse = True
        else:
            raise _Refused("a /Decode that is neither the default nor fully reversed")
    data = st.raw
    while len(filters) > 1 or (filters and filters[0][0] in ("ASCIIHexDecode", "AHx", "ASCII85Decode", "A85")):
        name, parms = filters[0]
        if name not in ("ASCIIHexDecode", "AHx", "ASCII85Decode", "A85", "FlateDecode", "Fl"):
            raise _Refused("filter /%s in front of another" % name)
        data = _undo(name, parms, data)
        filters = filters[1:]
    name, parms = filters[0] if filters else ("", {})
    name = {"DCT": "DCTDecode", "CCF": "CCITTFaxDecode", "Fl": "FlateDecode", "LZW": "LZWDecode"}.get(name, name)
    invert, one_strip = False, False
    if name == "DCTDecode":
        if space == "indexed" or bits != 8:
            raise _Refused("a DCT image that is not 8-bit gray or R,G,B")
        file, invert = data, reverse
    elif name == "CCITTFaxDecode":
        k = parms.get("K", 0)
        if not _is_num(k) or k >= 0:
            raise _Refused("CCITTFaxDecode with K = %r (Group 3): only K < 0 (Group 4) is taken" % (k,))
        if parms.get("EncodedByteAlign") is True:
            raise _Refused("CCITTFaxDecode with /EncodedByteAlign true")
        if bits != 1 or parms.get("Columns", 1728) != w:
            raise _Refused("a CCITT image whose /Columns or bits disagree with the image")
        white_is_one = parms.get("BlackIs1") is not True            # the decoder's bit for a white run
        if space == "indexed":
            base, _hival, lookup = extra
            pal = _palette_rgb(base, lookup, 1, reverse)
            if pal[0].tolist() == [0, 0, 0] and pal[1].tolist() == [255, 255, 255]:
                pass
            elif pal[1].tolist() == [0, 0, 0] and pal[0].tolist() == [255, 255, 255]:
                white_is_one = not white_is_one
            else:
                raise _Refused("a CCITT image over a palette that is not black and white")
        elif reverse:
            white_is_one = not white_is_one
        # a TIFF Group 4 decoder gives 0 for a white run: WhiteIsZero (0) shows those white, BlackIsZero (1) black
        file = _tiff_file(w, h, 1, 1, 4, 0 if white_is_one else 1, data)
        one_strip = h > 64
    elif name in ("FlateDecode", "LZWDecode", ""):
        pred = parms.get("Predictor", 1)
        if not _is_int(pred) or not (pred in (1, 2) or 10 <= pred <= 15):
            raise _Refused("predictor %r" % (pred,))
        if pred != 1 and (parms.get("Colors", 1) != comps or parms.get("BitsPerComponent", 8) != bits or parms.get("Columns", 1) != w):
            raise _Refused("predictor parameters that disagree with the image")
        if name == "LZWDecode" and parms.get("EarlyChange", 1) != 1:
            raise _Refused("LZWDecode with /EarlyChange 0")
        if space == "indexed":
            base, _hival, lookup = extra
            pal = _palette_rgb(base, lookup, bits, reverse)
        else:
            invert = reverse
        if pred >= 10:
            if name != "FlateDecode":
                raise _Refused("a PNG predictor under /%s" % (name or "no filter"))
            file = _png_file(w, h, bits, {"gray": 0, "rgb": 2, "indexed": 3}[space], data, pal.tobytes() if space == "indexed" else None)
        else:
            compression = {"FlateDecode": 8, "LZWDecode": 5, "": 1}[name]
            if space == "indexed" and bits == 1:
                bw = [pal[0].tolist(), pal[1].tolist()]
                if bw == [[0, 0, 0], [255, 255, 255]]:
                    file = _tiff_file(w, h, 1, 1, compression, 1, data, pred)
                elif bw == [[255, 255, 255], [0, 0, 0]]:
                    file = _tiff_file(w, h, 1, 1, compression, 0, data, pred)
                else:
                    raise _Refused("a 1-bit Indexed image over a palette that is not black and white")
            elif space == "indexed":
                cmap = [int(v) * 257 for ch in range(3) for v in pal[:, ch]]
                file = _tiff_file(w, h, bits, 1, compression, 3, data, pred, cmap)
            else:
                file = _tiff_file(w, h, bits, comps, compression, 1 if comps == 1 else 2, data, pred)
    else:
        raise _Refused("an image behind filter /%s" % name)
    return _Item(file, name, w, h, bits, 0, invert, None, one_strip)


def _page_items(doc, node, inherited):
    """The _Items of one page in paint order, or _Refused."""
    resources = doc.resolve(inherited.get("Resources")) or {}
    if not isinstance(resources, dict):
        raise _Refused("/Resources that is no dictionary")
    contents = doc.resolve(node.get("Contents"))
    parts = contents if isinstance(contents, list) else [contents]
    body = []
    for part in parts:
        part = doc.resolve(part)
        if part is None:
            continue
        if not isinstance(part, Stream):
            raise _Refused("/Contents that is no stream")
        body.append(doc.stream_bytes(part))
    lx = _Lexer(b"\n".join(body))
    xobjects = doc.resolve(resources.get("XObject")) or {}
    ctm, stack, fill_black, operands, items = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0), [], True, [], []
    while True:
        lx.skip()
        if lx.p >= len(lx.d):
            break
        t = lx.obj()
        if not isinstance(t, _Op):
            operands.append(t)
            if len(operands) > 64:
                raise _Refused("more than 64 operands before an operator")
            continue
        op = str(t)
        if op not in _CONTENT_OPS:
            what = "an inline image (BI)" if op == "BI" else ("the graphics state operator gs" if op == "gs" else "operator %s" % op[:16])
            raise _Refused("the page is not image-only: %s" % what)
        if op == "q":
            if len(stack) >= 256:
                raise _Refused("q nested deeper than 256")
            stack.append((ctm, fill_black))
        elif op == "Q":
            if stack:
                ctm, fill_black = stack.pop()
        elif op == "cm":
            if len(operands) != 6 or not all(_is_num(v) for v in operands):
                raise _Refused("cm without six numbers")
            ctm = _mul(tuple(float(v) for v in operands), ctm)
        elif op in ("g", "rg"):
            if len(operands) != (1 if op == "g" else 3) or not all(_is_num(v) for v in operands):
                raise _Refused("%s without its numbers" % op)
            fill_black = all(float(v) == 0.0 for v in operands)
        elif op == "Do":
            if len(operands) != 1 or not isinstance(operands[0], Name):
                raise _Refused("Do without a name")
            st = doc.resolve(xobjects.get(str(operands[0]))) if isinstance(xobjects, dict) else None
            if not isinstance(st, Stream):
                raise _Refused("Do on /%s, which is no XObject of the page" % operands[0])
            sub = doc.resolve(st.d.get("Subtype"))
            if sub != "Image":
                raise _Refused("the page is not image-only: Do on a %s XObject" % ("form" if sub == "Form" else "/%s" % sub))
            code, box = _orientation(ctm)
            if len(items) >= 65536:
                raise _Refused("more than 65536 images on a page")
            items.append(_image_item(doc, st, resources, fill_black)._replace(orientation=code, box=box))
        operands = []
    return items


# orientation code after the canvas is turned clockwise by 90: code -> code
_TURN = {1: 6, 2: 7, 3: 8, 4: 5, 5: 2, 6: 3, 7: 4, 8: 1}


def _layout(page, items, media_box, rotate):
    """Fills page (sizes, scale, images) and page._items: per image (item, code, x, y, crop_x, crop_y, crop_w, crop_h) on the page
    as read (after /Rotate); _Refused where the geometry rules say so."""
    x0, y0, x1, y1 = media_box
    if not items:
        raise _Refused("the page paints no image")
    first = items[0]
    ow, oh = (first.h, first.w) if first.orientation >= 5 else (first.w, first.h)
    ext_w, ext_h = first.box[2] - first.box[0], first.box[3] - first.box[1]
    if not (ext_w > 0 and ext_h > 0):
        raise _Refused("an image of no extent")
    sx, sy = ow / ext_w, oh / ext_h
    W, H = _round((x1 - x0) * sx), _round((y1 - y0) * sy)
    if not (1 <= W <= 65535 and 1 <= H <= 65535):
        raise _Refused("a canvas of %d x %d pixels" % (W, H))
    placed = []
    for it in items:
        ow, oh = (it.h, it.w) if it.orientation >= 5 else (it.w, it.h)
        left, right = _round((it.box[0] - x0) * sx), _round((it.box[2] - x0) * sx)
        top, bottom = _round((y1 - it.box[3]) * sy), _round((y1 - it.box[1]) * sy)
        if right - left != ow or bottom - top != oh:
            raise _Refused("image resolution differs from the page's (%d x %d pixels into %d x %d)" % (ow, oh, right - left, bottom - top))
        code = it.orientation
        cw, ch = W, H
        for _ in range(rotate // 90):                            # a quarter turn clockwise of the canvas cw x ch
            left, top, ow, oh = ch - (top + oh), left, oh, ow
            cw, ch = ch, cw
            code = _TURN[code]
        cx, cy = max(0, -left), max(0, -top)
        w = min(left + ow, cw) - max(left, 0)
        h = min(top + oh, ch) - max(top, 0)
        if w <= 0 or h <= 0:
            continue                                             # wholly outside the MediaBox
        placed.append((it, code, max(left, 0), max(top, 0), cx, cy, w, h))
    for i, a in enumerate(placed):
        for b in placed[:i]:
            if a[2] < b[2] + b[6] and b[2] < a[2] + a[6] and a[3] < b[3] + b[7] and b[3] < a[3] + a[7]:
                raise _Refused("two images overlap (a layered / MRC scan)")
    page.width, page.height = (H, W) if rotate in (90, 270) else (W, H)
    page.sx, page.sy, page._items = sx, sy, placed
    page.images = [PdfImage(it.filter, it.w, it.h, it.bits, code, (x, y, w, h), (cx, cy), it.invert, None) for it, code, x, y, cx, cy, w, h in placed]


def _inspect(data, wanted=None):
    try:
        doc = _Doc(data)
        nodes = doc.pages()
    except PdfError:
        raise
    except RecursionError:
        raise PdfError("objects nested too deep")
    except (struct.error, IndexError, KeyError, TypeError, AttributeError, OverflowError, MemoryError, UnicodeError, ValueError) as e:
        raise PdfError("a malformed file: %s: %s" % (type(e).__name__, e))
    pages = []
    for index, (node, inherited) in enumerate(nodes):
        page = PdfPage(index)
        pages.append(page)
        if wanted is not None and index not in wanted:
            page.refused = "not asked for"
            continue
        try:
            box = doc.resolve(inherited.get("MediaBox"))
            if not (isinstance(box, list) and len(box) == 4 and all(_is_num(doc.resolve(v)) for v in box)):
                raise _Refused("no /MediaBox of four numbers")
            box = [float(doc.resolve(v)) for v in box]
            box = (min(box[0], box[2]), min(box[1], box[3]), max(box[0], box[2]), max(box[1], box[3]))
            if not (box[2] > box[0] and box[3] > box[1]):
                raise _Refused("an empty /MediaBox")
            rotate = doc.resolve(inherited.get("Rotate", 0))
            if not _is_int(rotate) or rotate % 90:
                raise _Refused("/Rotate %r is no multiple of 90" % (rotate,))
            page.media_box, page.rotate = box, rotate % 360
            _layout(page, _page_items(doc, node, inherited), box, page.rotate)
        except (_Refused, PdfError) as e:
            page.refused = str(e)
        except RecursionError:
            page.refused = "objects nested too deep"
        except (struct.error, IndexError, KeyError, TypeError, AttributeError, OverflowError, MemoryError, UnicodeError, ValueError) as e:
            page.refused = "a malformed page: %s: %s" % (type(e).__name__, e)
        if page.refused is not None:
            page.images, page._items = [], []
    return PdfInfo(pages)


def pdf_inspect(data):
    """Parse a PDF held in memory (host only; nothing is decoded) -> PdfInfo: per page its index, pixel width and height after
    /Rotate, sx, sy, rotate, media_box and refused (None, or why the page is not taken), and per image the filter, sides, bits,
    orientation code and destination rectangle.  PdfError (a ValueError) with the reason for a file that cannot be read at all:
    no header or trailer, broken cross-reference, /Encrypt, a looping /Prev or /Kids chain."""
    return _inspect(data)


def memory_files(data):
    """The files held in memory that read_pdf_pages would hand to the decoders for the accepted pages of a PDF: per page a list of
    bytes (JPEG, PNG or TIFF), None for a refused page.  Host only."""
    return [None if p.refused is not None else [it[0].file for it in p._items] for p in _inspect(data).pages]


def _compose_table(jobs, address, sizes):
    """The arguments of rtn_page_compose / rtn_page_compose_host behind the handle: jobs [(canvas, [(image, code, invert, x, y,
    crop_x, crop_y, w, h)])]; address(a) the address of a buffer, sizes(a) its (h, w)."""
    n_items = sum(len(items) for _c, items in jobs)
    table = (L.ComposeItem * max(n_items, 1))()
    k = 0
    for p, (_canvas, items) in enumerate(jobs):
        for img, code, invert, x, y, cx, cy, w, h in items:
            e = table[k]
            (e.h, e.w), e.src, e.orientation, e.invert = sizes(img), address(img), code, int(bool(invert))
            e.page, e.x, e.y, e.crop_x, e.crop_y, e.crop_w, e.crop_h = p, x, y, cx, cy, w, h
            k += 1
    n = len(jobs)
    ptrs = (C.c_void_p * max(n, 1))(*[address(c) for c, _ in jobs])
    widths = np.ascontiguousarray([sizes(c)[1] for c, _ in jobs], np.int32)
    heights = np.ascontiguousarray([sizes(c)[0] for c, _ in jobs], np.int32)
    return [n_items, table, n, ptrs, widths.ctypes.data, heights.ctypes.data], (table, ptrs, widths, heights)


def read_pdf_pages_host(src):
    """The host route, for comparison and for machines without a GPU: the pages of a scanned PDF (a path or bytes) as NumPy uint8
    (H,W,3) B,G,R arrays, None for a refused page, with the same bytes as read_pdf_pages: every file in memory through Pillow on
    this thread, the pages put together by the CPU twin rtn_page_compose_host."""
    info = _inspect(_as_bytes(src))
    out = []
    for page in info.pages:
        if page.refused is not None:
            out.append(None)
            continue
        try:
            images = [page_io._pillow_bgr(io.BytesIO(placed[0].file)) for placed in page._items]
        except Exception as e:                                   # whatever Pillow raises for a file it does not take
            page.refused = "Pillow does not take an image's file (%s: %s)" % (type(e).__name__, e)
            out.append(None)
            continue
        if any(img.shape[:2] != (placed[0].h, placed[0].w) for img, placed in zip(images, page._items)):
            page.refused = "an image decodes to other sides than its dictionary says"
            out.append(None)
            continue
        canvas = np.empty((page.height, page.width, 3), np.uint8)
        job = (canvas, [(img, code, it.invert, x, y, cx, cy, w, h) for img, (it, code, x, y, cx, cy, w, h) in zip(images, page._items)])
        args, keep = _compose_table([job], lambda a: a.ctypes.data, lambda a: a.shape[:2])
        rc = L.lib.rtn_page_compose_host(*args)
        if rc != 0:
            raise L.RtnError(rc, L.lib.rtn_last_error(None).decode("utf-8", "replace"))
        out.append(canvas)
    return out


# ---- reading --------------------------------------------------------------------------------------------------------------------------------
def _compose(dev, handle, jobs):
    """One rtn_page_compose over `jobs` (see _compose_table) on the handle's stream."""
    args, _keep = _compose_table(jobs, lambda t: t.data_ptr(), lambda t: (int(t.shape[0]), int(t.shape[1])))
    wsb = int(L.lib.rtn_page_compose_workspace_bytes(args[0], args[2]))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    handle.check(L.lib.rtn_page_compose(handle.raw, *args, ws.data_ptr(), wsb))


def _g4_formats(allow):
    """page_io's formats, the TIFF inspector taking one-strip Group 4 when `allow`."""
    if not allow:
        return None

    def inspect(h, data, n, info, blob, capacity):
        return L.lib.rtn_tiff_inspect_flags(h, data, n, L.RTN_TIFF_ALLOW_G4_ONE_STRIP, info, blob, capacity)
    return tuple(f._replace(inspect=inspect) if f.name == "tiff" else f for f in page_io._ALL_FORMATS)


def _as_bytes(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    with open(src, "rb") as f:
        return f.read()


def read_pdfs_pages(srcs, pages=None, device=None, return_info=False):
    """read_pdf_pages for several files (paths or bytes) in ONE device batch: every image stream of every accepted page of every
    file goes through page_io._decode_datas in one call, so each device decoder runs at most once (RTN_TIFF_MIN, RTN_PNG_STREAM_MIN
    and RTN_PNG_LAYOUT_MIN apply as they are, Pillow is the per-file fallback; Group 4 images of more than 64 rows in one strip
    are taken by the device from RTN_PDF_G4_MIN of them on, pdf_g4_min()), then one rtn_page_compose puts the images of the pages
    that need it onto their canvases.  A page that is one upright image covering its canvas, not inverted, is the decoder's tensor
    and launches nothing.  `pages`: None for all, or a list of page indices (from 0) per file (None for all of that file).
    Returns a list per file of CUDA uint8 (H,W,3) B,G,R tensors, None for a refused page (or one not asked for); with
    return_info=True (pages, infos), infos the PdfInfo of every file, its images' route set to "device" or "host".  PdfError for a
    file that cannot be read."""
    srcs = list(srcs)
    if pages is None:
        pages = [None] * len(srcs)
    pages = list(pages)
    if len(pages) != len(srcs):
        raise ValueError("%d page lists for %d files" % (len(pages), len(srcs)))
    infos = [_inspect(_as_bytes(s), None if want is None else set(int(v) for v in want)) for s, want in zip(srcs, pages)]
    files, owners = [], []
    for f, info in enumerate(infos):
        for page in info.pages:
            for k, placed in enumerate(page._items):
                files.append(placed[0].file)
                owners.append((f, page.index, k))
    failed = {}

    def host_decode(i):
        try:
            return page_io._pillow_bgr(io.BytesIO(files[i]))
        except Exception as e:                                   # whatever Pillow raises for a file it does not take
            failed[i] = "%s: %s" % (type(e).__name__, e)
            return np.zeros((1, 1, 3), np.uint8)

    out = [[None] * len(info.pages) for info in infos]
    if not files:
        return (out, infos) if return_info else out
    one_strip = sum(1 for info in infos for p in info.pages for placed in p._items if placed[0].g4_one_strip)
    allow = 1 <= pdf_g4_min() <= one_strip
    with page_io._reader(device) as (dev, h):
        stream = torch.cuda.current_stream(dev)
        images, words = page_io._decode_datas(files, host_decode, dev, h, stream, formats=_g4_formats(allow))
        at = {owner: i for i, owner in enumerate(owners)}
        jobs, job_pages = [], []
        for f, info in enumerate(infos):
            for page in info.pages:
                if page.refused is not None:
                    continue
                mine = [at[(f, page.index, k)] for k in range(len(page._items))]
                for i, placed in zip(mine, page._items):
                    it = placed[0]
                    if i in failed:
                        page.refused = "neither a device inspector nor Pillow takes an image's file (%s)" % failed[i]
                    elif tuple(images[i].shape) != (it.h, it.w, 3):
                        page.refused = "an image decodes to %d x %d pixels, its dictionary says %d x %d" % (
                            images[i].shape[1], images[i].shape[0], it.w, it.h)
                if page.refused is not None:
                    page.images, page._items = [], []
                    continue
                page.images = [im._replace(route="device" if words[i] == 0 else "host") for im, i in zip(page.images, mine)]
                if len(mine) == 1:
                    it, code, x, y, cx, cy, w, hh = page._items[0]
                    if code == 1 and not it.invert and (x, y, cx, cy) == (0, 0, 0, 0) and (w, hh) == (page.width, page.height) == (it.w, it.h):
                        out[f][page.index] = images[mine[0]]
                        continue
                canvas = torch.empty(page.height, page.width, 3, dtype=torch.uint8, device=dev)
                jobs.append((canvas, [(images[i], code, it.invert, x, y, cx, cy, w, hh)
                                      for i, (it, code, x, y, cx, cy, w, hh) in zip(mine, page._items)]))
                job_pages.append((f, page.index))
        if jobs:
            h.set_stream(stream.cuda_stream)
            with torch.cuda.stream(stream):                       # the images and the workspace are this stream's: freed in its order
                _compose(dev, h, jobs)
            for (f, index), (canvas, _items) in zip(job_pages, jobs):
                out[f][index] = canvas
    return (out, infos) if return_info else out


def read_pdf_pages(src, pages=None, device=None, return_info=False):
    """The pages of a scanned PDF (a path or bytes) as CUDA uint8 (H,W,3) B,G,R tensors, None for a refused page: read_pdfs_pages
    of one file.  `pages`: None for all, or the page indices (from 0) to read.  With return_info=True (pages, PdfInfo)."""
    got = read_pdfs_pages([src], pages=[pages], device=device, return_info=return_info)
    return (got[0][0], got[1][0]) if return_info else got[0]


# ---- boxes ----------------------------------------------------------------------------------------------------------------------------------
def _canvas(page):
    return (page.height, page.width) if page.rotate in (90, 270) else (page.width, page.height)


def pdf_boxes_to_pixels(boxes_pt, page, factor=1.0):
    """Boxes (x1, y1, x2, y2) in PDF points of the unrotated user space, y upwards, as pixel boxes on the page as read (PdfPage;
    `factor`: the enlargement applied after reading, if any): the reference's PDFCSVtoImageCSV, x_px = int(scale x_pt) and y_px =
    h - int(scale y_pt) with the box's upper edge becoming the smaller y, measured from the MediaBox's corner; then /Rotate.  For
    /Rotate 0 and a MediaBox at the origin these are the reference's two formulas bit for bit.  Returns int64 (n, 4)."""
    b = np.asarray(boxes_pt, np.float64).reshape(-1, 4)
    W, H = _canvas(page)
    sx, sy = page.sx * float(factor), page.sy * float(factor)
    W, H = int(np.rint(W * float(factor))), int(np.rint(H * float(factor)))
    x0, y0 = page.media_box[0], page.media_box[1]
    out = np.zeros((len(b), 4), np.int64)
    for i, (x1, y1, x2, y2) in enumerate(b):
        px1, px2 = int(sx * (x1 - x0)), int(sx * (x2 - x0))
        py1, py2 = H - int(sy * (y2 - y0)), H - int(sy * (y1 - y0))
        w, h = W, H
        for _ in range(page.rotate // 90):                       # a quarter turn clockwise: (x, y) -> (h - y, x)
            px1, py1, px2, py2 = h - py2, px1, h - py1, px2
            w, h = h, w
        out[i] = (min(px1, px2), min(py1, py2), max(px1, px2), max(py1, py2))
    return out


def boxes_to_pdf(boxes, page, factor=1.0):
    """The inverse of pdf_boxes_to_pixels: pixel boxes (x1, y1, x2, y2) on the page as read (PdfPage), enlarged by `factor` if the
    page was, as (x1, y1, x2, y2) in points of the unrotated user space, y upwards (y1 < y2), /Rotate undone.  float64 (n, 4)."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4) / float(factor)
    W, H = _canvas(page)
    x0, y0 = page.media_box[0], page.media_box[1]
    out = np.zeros((len(b), 4), np.float64)
    for i, (px1, py1, px2, py2) in enumerate(b):
        w, h = (W, H) if page.rotate % 180 == 0 else (H, W)      # of the page as read
        for _ in range(page.rotate // 90):                       # undo a quarter turn clockwise: (x, y) -> (y, w - x)
            px1, py1, px2, py2 = py1, w - px2, py2, w - px1
            w, h = h, w
        xs, ys = (x0 + px1 / page.sx, x0 + px2 / page.sx), (y0 + (H - py1) / page.sy, y0 + (H - py2) / page.sy)
        out[i] = (min(xs), min(ys), max(xs), max(ys))
    return out


# ---- writing --------------------------------------------------------------------------------------------------------------------------------
def _num(v):
    s = "%.6f" % v
    return s.rstrip("0").rstrip(".") if "." in s else s


def _tiff_strips(data):
    """(width, height, photometric, [(first row, rows, strip bytes)]) of a little-endian strip TIFF, by its own strip table."""
    if data[:4] != b"II*\0":
        raise ValueError("a little-endian TIFF expected")
    ifd, = struct.unpack_from("<I", data, 4)
    n, = struct.unpack_from("<H", data, ifd)
    tags = {}
    for k in range(n):
        tag, typ, count, value = struct.unpack_from("<HHII", data, ifd + 2 + 12 * k)
        size = {1: 1, 3: 2, 4: 4}[typ]
        if count * size <= 4:
            vals = list(struct.unpack_from("<%d%s" % (count, {1: "B", 3: "H", 4: "I"}[typ]), data, ifd + 2 + 12 * k + 8))
        else:
            vals = list(struct.unpack_from("<%d%s" % (count, {1: "B", 3: "H", 4: "I"}[typ]), data, value))
        tags[tag] = vals
    w, h, rps = tags[256][0], tags[257][0], min(tags[278][0], tags[257][0])
    strips = [(k * rps, min(rps, h - k * rps), data[off:off + size]) for k, (off, size) in enumerate(zip(tags[273], tags[279]))]
    return w, h, tags[262][0], strips


def write_pages_pdf(path, pages, tiff=None, quality=95, dpi=300):
    """A scan archive around the device encoders: a PDF 1.4 with a classic cross-reference table, one page per input page (uint8
    (H,W,3) B,G,R or (H,W) gray; CUDA or host), the MediaBox H x W pixels at `dpi`.  By default every page is one DCTDecode image,
    the JPEG of encode_jpeg_bgr at `quality`.  tiff="g4": every page is thresholded and coded by encode_tiff_bgr (bilevel: ink is
    gray < 128; Group 4, 64 rows per strip) and each strip, taken out of the encoded file by its own strip table, is one
    CCITTFaxDecode image XObject (/K -1, /BlackIs1 chosen so that paper is white), stacked by cm; read_pdf_pages decodes such a
    file with one wave per strip.  `path` None returns the bytes."""
    pages = list(pages)
    if tiff not in (None, "g4"):
        raise ValueError("tiff must be None or 'g4', got %r" % (tiff,))
    if not dpi > 0:
        raise ValueError("dpi must be positive")
    dims = [page_io._check_page(i, p) for i, p in enumerate(pages)]
    unit = 72.0 / float(dpi)
    objs = {}                                                    # number -> bytes of the object's body

    def stream(d, data):
        return ("<< %s /Length %d >>\nstream\n" % (d, len(data))).encode("latin-1") + data + b"\nendstream"

    files = page_io.encode_tiff_bgr(pages) if tiff == "g4" else page_io.encode_jpeg_bgr(pages, quality=quality)
    next_num, kids = 3, []
    for (H, W, comps), data in zip(dims, files):
        page_num, content_num = next_num, next_num + 1
        next_num += 2
        wpt, hpt = W * unit, H * unit
        xobjects, content = [], []
        if tiff == "g4":
            w, h, photometric, strips = _tiff_strips(data)
            for k, (row, rows, strip) in enumerate(strips):
                d = ("/Type /XObject /Subtype /Image /Width %d /Height %d /ColorSpace /DeviceGray /BitsPerComponent 1 /Filter /CCITTFaxDecode "
                     "/DecodeParms << /K -1 /Columns %d /Rows %d /BlackIs1 %s >>" % (w, rows, w, rows, "true" if photometric == 1 else "false"))
                objs[next_num] = stream(d, strip)
                xobjects.append("/S%d %d 0 R" % (k, next_num))
                content.append("q %s 0 0 %s 0 %s cm /S%d Do Q" % (_num(wpt), _num(rows * unit), _num(hpt - (row + rows) * unit), k))
                next_num += 1
        else:
            d = ("/Type /XObject /Subtype /Image /Width %d /Height %d /ColorSpace /%s /BitsPerComponent 8 /Filter /DCTDecode"
                 % (W, H, "DeviceGray" if comps == 1 else "DeviceRGB"))
            objs[next_num] = stream(d, data)
            xobjects.append("/Im0 %d 0 R" % next_num)
            content.append("q %s 0 0 %s 0 0 cm /Im0 Do Q" % (_num(wpt), _num(hpt)))
            next_num += 1
        objs[content_num] = stream("", "\n".join(content).encode("latin-1"))
        objs[page_num] = ("<< /Type /Page /Parent 2 0 R /MediaBox [0 0 %s %s] /Resources << /XObject << %s >> >> /Contents %d 0 R >>"
                          % (_num(wpt), _num(hpt), " ".join(xobjects), content_num)).encode("latin-1")
        kids.append(page_num)
    objs[1] = b"<< /Type /Catalog /Pages 2 0 R >>"
    objs[2] = ("<< /Type /Pages /Count %d /Kids [%s] >>" % (len(kids), " ".join("%d 0 R" % k for k in kids))).encode("latin-1")
    out = bytearray(b"%PDF-1.4\n%\xe2\xe3\xcf\xd3\n")
    offsets = {}
    for num in sorted(objs):
        offsets[num] = len(out)
        out += ("%d 0 obj\n" % num).encode("latin-1") + objs[num] + b"\nendobj\n"
    xref_at = len(out)
    out += ("xref\n0 %d\n0000000000 65535 f \n" % next_num).encode("latin-1")
    for num in range(1, next_num):
        out += ("%010d 00000 n \n" % offsets[num]).encode("latin-1")
    out += ("trailer\n<< /Size %d /Root 1 0 R >>\nstartxref\n%d\n%%%%EOF\n" % (next_num, xref_at)).encode("latin-1")
    if path is None:
        return bytes(out)
    with open(path, "wb") as f:
        f.write(out)
    return None
