"""Reference helpers for the stream PNG decoder (csrc/rtn_png_stream.hip): the five PNG row filters done and undone
in NumPy, a file assembler that wraps any zlib stream into a PNG with any IDAT cut points and optional ancillary chunks, and the
list of deflate stream shapes the CPU and GPU tests share.  Uses zlib, struct, NumPy and png_encode_ref alone;
tests/test_png_stream_host.py holds the helper against Pillow and proves it can fail."""
import random
import struct
import zlib

import numpy as np

import png_encode_ref as R

Z_BLOCK = 5                                              # zlib.h (the zlib module exports it only in newer Pythons)


def _paeth(a, b, c, tie_to_c=False):
    """The Paeth predictor on int arrays; tie_to_c=True is the deliberately wrong tie-break the tests use to prove they can fail."""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    if tie_to_c:
        return np.where((pa < pb) & (pa < pc), a, np.where(pb < pc, b, c))
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_page(page_bgr, types):
    """The filtered stream (bytes) of a page with filter type types[y] (0 .. 4) on row y."""
    a = R.rgb_of(page_bgr)
    h, w = a.shape[:2]
    c = 1 if a.ndim == 2 else 3
    rows = a.reshape(h, w * c).astype(np.int32)
    out = np.zeros((h, 1 + w * c), np.uint8)
    zero = np.zeros(w * c, np.int32)
    for y in range(h):
        x, up = rows[y], (rows[y - 1] if y else zero)
        left = np.concatenate([zero[:c], x[:-c]]) if w * c > c else zero[:w * c]
        upleft = np.concatenate([zero[:c], up[:-c]]) if w * c > c else zero[:w * c]
        t = int(types[y])
        pred = [zero, left, up, (left + up) // 2, _paeth(left, up, upleft)][t]
        out[y, 0] = t
        out[y, 1:] = (x - pred) & 255
    return out.tobytes()


def unfilter(stream, w, h, c, wrong_paeth=False):
    """Undo the five filters of a filtered stream -> (h, w*c) uint8; a filter type above 4 is an error."""
    rows = np.frombuffer(stream, np.uint8).reshape(h, 1 + w * c)
    out = np.zeros((h, w * c), np.uint8)
    prev = np.zeros(w * c, np.int32)
    for y in range(h):
        t = int(rows[y, 0])
        assert t <= 4, "filter type %d" % t
        x = rows[y, 1:].astype(np.int32)
        if t == 0:
            cur = x
        elif t == 2:
            cur = (x + prev) & 255
        else:                                             # left-dependent: pixel by pixel, all channels at once
            cur = np.zeros(w * c, np.int32)
            a = np.zeros(c, np.int32)
            cc = np.zeros(c, np.int32)
            for px in range(w):
                b = prev[px * c:(px + 1) * c]
                pred = a if t == 1 else (a + b) // 2 if t == 3 else _paeth(a, b, cc, wrong_paeth)
                a = (x[px * c:(px + 1) * c] + pred) & 255
                cur[px * c:(px + 1) * c] = a
                cc = b
        out[y] = cur
        prev = cur
    return out


def ihdr(w, h, c, depth=8, ctype=None, interlace=0):
    return R._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, (2 if c == 3 else 0) if ctype is None else ctype, 0, 0, interlace))


def assemble(w, h, c, zstream, cuts=None, before=(), after=(), between=None):
    """A PNG file of a w x h page of c components around any zlib stream.  cuts: the offsets at which the stream is cut into IDATs
    (sorted, may repeat: an empty IDAT); before / after: (type, payload) chunks in front of and behind the IDAT run; between: a
    (type, payload) chunk put after the first IDAT (which breaks the run)."""
    out = R.SIGNATURE + ihdr(w, h, c)
    for t, b in before:
        out += R._chunk(t, b)
    edges = [0] + list(cuts or []) + [len(zstream)]
    for k in range(len(edges) - 1):
        out += R._chunk(b"IDAT", zstream[edges[k]:edges[k + 1]])
        if between is not None and k == 0:
            out += R._chunk(*between)
    for t, b in after:
        out += R._chunk(t, b)
    return out + R._chunk(b"IEND", b"")


def zwrap(deflate, raw, adler=None):
    """A zlib stream around raw deflate data for the bytes `raw`."""
    return R.ZLIB_HEADER + deflate + struct.pack(">I", (zlib.adler32(raw) if adler is None else adler) & 0xffffffff)


def every(n, step):
    return list(range(step, n, step))


STREAM_SHAPES = [                                        # (name, level, memLevel, strategy)
    ("l6m1", 6, 1, zlib.Z_DEFAULT_STRATEGY), ("l1m1", 1, 1, zlib.Z_DEFAULT_STRATEGY), ("l6m2", 6, 2, zlib.Z_DEFAULT_STRATEGY),
    ("l6m8", 6, 8, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, 1, zlib.Z_FIXED), ("stored", 0, 8, zlib.Z_DEFAULT_STRATEGY),
    ("rle", 6, 1, zlib.Z_RLE), ("huffman", 6, 1, zlib.Z_HUFFMAN_ONLY),
]


def deflate_shapes(raw, seed=0):
    """[(name, raw deflate data)] of the bytes `raw`: every entry of STREAM_SHAPES, and one stream flushed at random points."""
    out = []
    for name, level, mem, strategy in STREAM_SHAPES:
        co = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
        out.append((name, co.compress(raw) + co.flush()))
    rng = random.Random(seed)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 4)
    pos, data, k = 0, b"", 0
    while pos < len(raw):
        n = rng.randint(1, max(2, len(raw) // 6))
        data += co.compress(raw[pos:pos + n]) + co.flush((zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, Z_BLOCK)[k % 3])
        pos += n
        k += 1
    out.append(("flushes", data + co.flush()))
    for name, d in out:
        assert zlib.decompressobj(-15).decompress(d) == raw, name
    return out
