"""Reference helpers for the PNG pixel layouts (csrc/rtn_png_layout.h, DESIGN §3.4f "Pixel layouts"): a NumPy + zlib writer for any
legal PNG layout (depth, colour type, Adam7, any filter type per row of every pass, palette, tRNS, chosen padding bits), which
Pillow cannot write itself, and a NumPy statement of what Image.open(f).convert("RGB") makes of the samples.  The oracle of every
test is Pillow reading the written bytes back; tests/test_png_layout_host.py holds this helper against Pillow and proves that it
can fail (the lsb_first and low_byte switches are the deliberately wrong variants)."""
import struct
import zlib

import numpy as np

import png_encode_ref as R

SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# every (colour type, depth) pair the layout decoder accepts: all legal pairs but 16-bit gray
ACCEPTED = [(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]      # x0, y0, dx, dy


def passes(w, h, interlace):
    """[(x0, y0, dx, dy, cols, rows)] of the passes that have rows and columns, in stream order."""
    out = []
    for x0, y0, dx, dy in (ADAM7 if interlace else [(0, 0, 1, 1)]):
        cols, rows = (w - x0 + dx - 1) // dx if w > x0 else 0, (h - y0 + dy - 1) // dy if h > y0 else 0
        if cols > 0 and rows > 0:
            out.append((x0, y0, dx, dy, cols, rows))
    return out


def row_bytes(cols, ctype, depth):
    return (cols * SAMPLES[ctype] * depth + 7) // 8


def stream_bytes(w, h, ctype, depth, interlace):
    return sum(rows * (1 + row_bytes(cols, ctype, depth)) for _, _, _, _, cols, rows in passes(w, h, interlace))


def pack(samp, depth, pad_ones=False, lsb_first=False):
    """(rows, cols, ns) samples below 2^depth -> (rows, row bytes) uint8: samples MSB first, 16-bit samples big-endian, the unused
    low bits of a row's last byte zeros or ones.  lsb_first=True is the wrong bit order."""
    rows, cols, ns = samp.shape
    flat = samp.reshape(rows, cols * ns).astype(np.uint32)
    if depth == 8:
        return flat.astype(np.uint8)
    if depth == 16:
        return np.stack([flat >> 8, flat & 255], -1).astype(np.uint8).reshape(rows, cols * ns * 2)
    per = 8 // depth
    n = (cols * ns + per - 1) // per
    padded = np.full((rows, n * per), (1 << depth) - 1 if pad_ones else 0, np.uint32)
    padded[:, :cols * ns] = flat
    out = np.zeros((rows, n), np.uint32)
    for k in range(per):
        out |= padded[:, k::per] << ((depth * k) if lsb_first else (8 - depth * (k + 1)))
    return out.astype(np.uint8)


def filter_rows(data, types, bpp):
    """(rows, rb) reconstructed bytes -> the filtered rows with their type bytes, (rows, 1 + rb)."""
    rows, rb = data.shape
    x = data.astype(np.int32)
    out = np.zeros((rows, 1 + rb), np.uint8)
    zero = np.zeros(rb, np.int32)
    for y in range(rows):
        up = x[y - 1] if y else zero
        left, upleft = zero.copy(), zero.copy()
        left[bpp:], upleft[bpp:] = x[y, :rb - bpp] if rb > bpp else [], up[:rb - bpp] if rb > bpp else []
        t = int(types[y])
        if t == 4:
            p = left + up - upleft
            pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        else:
            pred = [zero, left, up, (left + up) // 2][t]
        out[y, 0] = t
        out[y, 1:] = (x[y] - pred) & 255
    return out


def raw_stream(samp, ctype, depth, interlace=0, filters=0, pad_ones=False, lsb_first=False):
    """The filtered stream of a page of samples (h, w, ns).  filters: one type 0 .. 4 for every row, or a RandomState that draws a
    type per row of every pass.  Returns (bytes, [offset of every pass's first row])."""
    h, w, ns = samp.shape
    assert ns == SAMPLES[ctype] and int(samp.max()) < (1 << depth)
    bpp = max(1, ns * depth // 8)
    out, offs = b"", []
    for x0, y0, dx, dy, cols, rows in passes(w, h, interlace):
        sub = samp[y0::dy, x0::dx]
        assert sub.shape[:2] == (rows, cols)
        types = np.full(rows, filters) if isinstance(filters, int) else filters.randint(0, 5, rows)
        offs.append(len(out))
        out += filter_rows(pack(sub, depth, pad_ones, lsb_first), types, bpp).tobytes()
    assert len(out) == stream_bytes(w, h, ctype, depth, interlace)
    return out, offs


def ihdr(w, h, ctype, depth, interlace=0):
    return R._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))


def wrap(w, h, ctype, depth, interlace, zstream, palette=None, before=(), after=(), plte_after=False, cuts=None):
    """A PNG file around any zlib stream.  palette: (n, 3) R,G,B entries written as PLTE in front of the first IDAT (plte_after:
    behind the last instead); before / after: (type, payload) chunks in front of (behind PLTE) and behind the IDATs."""
    plte = R._chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()) if palette is not None else b""
    out = R.SIGNATURE + ihdr(w, h, ctype, depth, interlace) + (b"" if plte_after else plte)
    for t, b in before:
        out += R._chunk(t, b)
    edges = [0] + list(cuts or []) + [len(zstream)]
    for k in range(len(edges) - 1):
        out += R._chunk(b"IDAT", zstream[edges[k]:edges[k + 1]])
    if plte_after:
        out += plte
    for t, b in after:
        out += R._chunk(t, b)
    return out + R._chunk(b"IEND", b"")


def write(samp, ctype, depth, interlace=0, filters=0, pad_ones=False, palette=None, trns=None, lsb_first=False, level=6):
    """The PNG file of a page of samples (h, w, ns); trns: the payload of a tRNS chunk."""
    raw, _ = raw_stream(samp, ctype, depth, interlace, filters, pad_ones, lsb_first)
    h, w = samp.shape[:2]
    return wrap(w, h, ctype, depth, interlace, zlib.compress(raw, level), palette, before=[(b"tRNS", trns)] if trns is not None else ())


def expected_bgr(samp, ctype, depth, palette=None, low_byte=False):
    """What Image.open(f).convert("RGB") gives, as B,G,R: gray scaled by 255 / (2^depth - 1), the PLTE entry ((0,0,0) past the
    last), the high byte of 16-bit samples, alpha dropped.  low_byte=True is the wrong byte of a 16-bit sample."""
    v = samp.astype(np.int64)
    if depth == 16:
        v = (v & 255) if low_byte else (v >> 8)
    if ctype == 3:
        table = np.zeros((256, 3), np.int64)
        table[:len(palette)] = np.asarray(palette)
        rgb = table[v[:, :, 0]]
    elif ctype in (0, 4):
        g = v[:, :, 0] * (255 // ((1 << depth) - 1)) if depth < 8 else v[:, :, 0]
        rgb = np.stack([g, g, g], -1)
    else:
        rgb = v[:, :, :3]
    return np.ascontiguousarray(rgb[:, :, ::-1].astype(np.uint8))


def random_page(rng, w, h, ctype, depth, smooth=False):
    """Random samples (h, w, ns); smooth: slowly varying, so that the predictors matter."""
    ns = SAMPLES[ctype]
    if smooth and depth >= 8:
        v = np.cumsum(np.cumsum(rng.randint(0, 3 << (depth - 8), (h, w, ns)), axis=0), axis=1) & ((1 << depth) - 1)
    else:
        v = rng.randint(0, 1 << depth, (h, w, ns))
    return v.astype(np.int64)


def random_palette(rng, n):
    return rng.randint(0, 256, (n, 3)).astype(np.uint8)
