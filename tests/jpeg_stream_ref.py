"""Marker-level surgery on baseline JPEG files, for the decoder tests (tests/test_jpeg_decode_host.py, tests/test_gpu_jpeg.py).

split / join take a Pillow-written file apart and put it back together; the variants rearrange, renumber, widen, pad or repeat its
header segments the ways other writers do.  The entropy-coded bytes are never re-encoded, so Pillow's decode of each variant's own
bytes is the expected result.  built() assembles files from chosen coefficients (tests/jpeg_encode_ref.py's scan()) that reach
paths a real FDCT rarely does: ZRL runs, a coefficient at index 63, the largest DC and AC categories, Huffman codes of every
length up to 16 bits, a perfectly periodic stream."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_encode_ref as R  # noqa: E402

SOF0, DHT, SOS, DQT, DRI, APP0, APP1, APP2, APP14, COM = 0xC0, 0xC4, 0xDA, 0xDB, 0xDD, 0xE0, 0xE1, 0xE2, 0xEE, 0xFE


def split(data):
    """(segs, scan): the header segments [(marker, payload)] from after SOI up to and including SOS, and the entropy-coded bytes
    (stuffing and RSTn included) up to, not including, EOI."""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    segs, pos = [], 2
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        segs.append((m, bytes(data[pos + 4:pos + 2 + n])))
        pos += 2 + n
        if m == SOS:
            return segs, bytes(data[pos:-2])


def join(segs, scan, fill=0, tail=b""):
    """SOI, the segments, the scan, EOI, tail.  fill: that many extra 0xFF bytes before every header marker, and one (if fill) before
    each RSTn and before EOI."""
    out = bytearray(b"\xff\xd8")
    for m, payload in segs:
        out += b"\xff" * fill + bytes([0xFF, m]) + struct.pack(">H", len(payload) + 2) + payload
    if fill:
        padded, i = bytearray(), 0
        while i < len(scan):
            if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
                padded += b"\xff"
            padded += scan[i:i + 2] if scan[i] == 0xFF else scan[i:i + 1]
            i += 2 if scan[i] == 0xFF else 1
        scan = bytes(padded) + b"\xff"
    return bytes(out) + scan + b"\xff\xd9" + tail


def _tables(payload, dqt):
    """the tables of one DQT or DHT payload: [(first byte, rest)]"""
    out, q = [], 0
    while q < len(payload):
        n = (64 * (1 + (payload[q] >> 4))) if dqt else 16 + sum(payload[q + 1:q + 17])
        out.append((payload[q], payload[q + 1:q + 1 + n]))
        q += 1 + n
    return out


def _map_segs(segs, marker, fn):
    return [(m, fn(p) if m == marker else p) for m, p in segs]


def _first(segs, marker):
    return next(i for i, (m, _) in enumerate(segs) if m == marker)


def _widen(scale):
    def fn(p):
        out = b""
        for head, body in _tables(p, True):
            assert head >> 4 == 0
            out += bytes([0x10 | head]) + b"".join(struct.pack(">H", v * scale) for v in body)
        return out
    return fn


def _component_ids(segs, ids):
    def sof(p):
        b = bytearray(p)
        for c in range(p[5]):
            b[6 + 3 * c] = ids[c]
        return bytes(b)

    def sos(p):
        b = bytearray(p)
        for c in range(p[0]):
            b[1 + 2 * c] = ids[c]
        return bytes(b)
    return _map_segs(_map_segs(segs, SOF0, sof), SOS, sos)


def _without(segs, marker):
    return [(m, p) for m, p in segs if m != marker]


def _adobe(transform):
    return (APP14, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, transform))


def _renumber(segs):
    qmap, hmap = {0: 2, 1: 3}, {0: 3, 1: 2}

    def dqt(p):
        return b"".join(bytes([(h & 0xF0) | qmap[h & 15]]) + body for h, body in _tables(p, True))

    def dht(p):
        return b"".join(bytes([(h & 0xF0) | hmap[h & 15]]) + body for h, body in _tables(p, False))

    def sof(p):
        b = bytearray(p)
        for c in range(p[5]):
            b[8 + 3 * c] = qmap[b[8 + 3 * c]]
        return bytes(b)

    def sos(p):
        b = bytearray(p)
        for c in range(p[0]):
            v = b[2 + 2 * c]
            b[2 + 2 * c] = (hmap[v >> 4] << 4) | hmap[v & 15]
        return bytes(b)
    for marker, fn in ((DQT, dqt), (DHT, dht), (SOF0, sof), (SOS, sos)):
        segs = _map_segs(segs, marker, fn)
    return segs


def _merged(segs):
    for marker in (DQT, DHT):
        whole = b"".join(p for m, p in segs if m == marker)
        at = _first(segs, marker)
        segs = [(m, whole if i == at else p) for i, (m, p) in enumerate(segs) if m != marker or i == at]
    return segs


def _filler(n, seed):
    return b"junk" + np.random.RandomState(seed).randint(0, 256, n - 4).astype(np.uint8).tobytes()


def variants(data):
    """{name: bytes} of every header variant of one Pillow-written baseline file (gray or YCbCr)."""
    segs, scan = split(data)
    has_dri = any(m == DRI for m, _ in segs)
    out = {}
    out["merged"] = join(_merged(segs), scan)
    out["dqt16"] = join(_map_segs(segs, DQT, _widen(1)), scan)
    out["dqt16x40"] = join(_map_segs(segs, DQT, _widen(40)), scan)
    out["fill"] = join(segs, scan, fill=2)
    out["trailing"] = join(segs, scan, tail=b"\x00" * 7 + b"\xff\xd9" + b"text after the end of the image")
    out["renum"] = join(_renumber(segs), scan)
    out["ids012"] = join(_component_ids(segs, (0, 1, 2)), scan)
    bare = _without(segs, APP0)
    out["nojfif789"] = join(_component_ids(bare, (7, 8, 9)), scan)
    out["nojfifRGBids"] = join(_component_ids(bare, (ord("R"), ord("G"), ord("B"))), scan)
    for t in (0, 1, 2):
        out["adobe%d" % t] = join([_adobe(t)] + bare, scan)
    at = _first(segs, APP0) + 1
    out["jfif+adobe0"] = join(segs[:at] + [_adobe(0)] + segs[at:], scan)
    out["bigapp"] = join(segs[:at] + [(APP1, _filler(60000, 1)), (COM, b"a comment"), (APP2, _filler(65533, 2))] + segs[at:], scan)
    at = _first(segs, DQT)
    junk = bytes([0]) + np.random.RandomState(3).randint(1, 256, 64).astype(np.uint8).tobytes()
    out["redefine"] = join(segs[:at] + [(DQT, junk)] + segs[at:], scan)
    real = next((p for m, p in segs if m == DRI), struct.pack(">H", 0))
    wrong = struct.pack(">H", struct.unpack(">H", real)[0] + 5)
    rest = segs if has_dri else segs[:-1] + [(DRI, real)] + segs[-1:]
    out["dri-twice"] = join(rest[:at] + [(DRI, wrong)] + rest[at:], scan)
    if not has_dri:
        out["dri-huge"] = join(segs[:-1] + [(DRI, struct.pack(">H", 65535))] + segs[-1:], scan)
    if segs[_first(segs, SOF0)][1][5] == 1:
        for hv in (0x22, 0x21, 0x12, 0x44):
            out["gray_samp%02x" % hv] = gray_samp(data, hv)
    return out


REFUSED = {"nojfifRGBids": "RGB JPEG (component ids R, G, B)", "adobe0": "Adobe RGB JPEG (transform 0)"}    # 3-component files only


def gray_samp(data, hv):
    """A 1-component file with sampling factors hv in its frame header (a single-component scan is never interleaved, so they change
    nothing)."""
    segs, scan = split(data)

    def sof(p):
        assert p[5] == 1
        return p[:7] + bytes([hv]) + p[8:]
    return join(_map_segs(segs, SOF0, sof), scan)


# ---- files built from chosen coefficients -----------------------------------------------------------------------------------------
def _dht(cls, ident, bits, vals):
    return (DHT, bytes([cls << 4 | ident]) + bytes(bits) + bytes(vals))


def assemble(coefs, w, h, components, subsampling, huff=None):
    """A baseline file of the given frame whose blocks (scan order, padding blocks included, zig-zag order) are coefs; both
    quantisation tables are all ones, so a coefficient is its dequantised value.  huff: see jpeg_encode_ref.scan."""
    hm, vm = (1, 1) if components == 1 or subsampling == 0 else ((2, 1) if subsampling == 1 else (2, 2))
    nblocks = -(-w // (8 * hm)) * -(-h // (8 * vm)) * (hm * vm + 2 if components == 3 else 1)
    assert len(coefs) == nblocks, (len(coefs), nblocks)
    tabs = huff if huff is not None else list(zip(R.HUFF_BITS, R.HUFF_VALS))
    segs = [(APP0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for t in range(2 if components == 3 else 1):
        segs.append((DQT, bytes([t]) + bytes([1] * 64)))
    frame = struct.pack(">BHHB", 8, h, w, components)
    for c in range(components):
        frame += bytes([c + 1, (hm << 4 | vm) if c == 0 else 0x11, 0 if c == 0 else 1])
    segs.append((SOF0, frame))
    for t in range(4 if components == 3 else 2):
        segs.append(_dht(t & 1, t >> 1, *tabs[t]))
    sos = bytes([components]) + b"".join(bytes([c + 1, 0x00 if c == 0 else 0x11]) for c in range(components)) + b"\x00\x3f\x00"
    segs.append((SOS, sos))
    return join(segs, R.scan(np.asarray(coefs), components, subsampling, huff))


def long_code_tables():
    """Four (bits, vals): DC codes of 1 .. 12 bits (one each, the longest for the smallest categories) and AC codes of 2 .. 16 bits,
    with codes at every length from 10 to 16, for all 162 AC symbols."""
    dc = ([1] * 12 + [0] * 4, list(range(11, -1, -1)))
    ac_bits = [0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 4, 8, 16, 32, 40, 52]
    syms = [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 11)]
    order = list(np.random.RandomState(7).permutation(len(syms)))
    ac = (ac_bits, [syms[i] for i in order])
    assert sum(ac_bits) == len(syms) == 162
    return [dc, ac, dc, ac]


def _value(size, negative):
    v = (1 << size) - 1 - (size * 37) % (1 << (size - 1))               # somewhere in the category's range
    return -v if negative else v


def built():
    """{name: (bytes, W, H)} of the coefficient-built files."""
    out = {}
    rng = np.random.RandomState(11)

    def blocks(n):
        return np.zeros((n, 64), np.int64)

    # AC runs needing one, two and three ZRL; a coefficient at index 63 (no EOB); 4:2:0 and gray
    for name, comps, ss, (w, h) in (("zrl63-420", 3, 2, (45, 61)), ("zrl63-gray", 1, 0, (45, 61))):
        n = -(-w // 16) * -(-h // 16) * 6 if comps == 3 else -(-w // 8) * -(-h // 8)
        b = blocks(n)
        for j in range(n):
            b[j, 0] = int(rng.randint(-60, 61))
            kind = j % 5
            if kind < 3:
                b[j, 1 + 16 * (kind + 1) + int(rng.randint(0, 14 - 2 * kind))] = int(rng.randint(1, 40)) * (1 if j & 1 else -1)
            if kind >= 2:
                b[j, 63] = int(rng.randint(1, 30)) * (-1 if j & 2 else 1)
            if kind == 4:
                b[j, 20] = -7
                b[j, 47] = 3                                          # 26 zeros between: one ZRL inside a block that has no EOB
        out[name] = (assemble(b, w, h, comps, ss), w, h)
    # DC differences of category 11 in both signs (4:2:2: three predictors), AC values of category 10 (4:4:4)
    w, h = 45, 61
    n = -(-w // 16) * -(-h // 8) * 4
    b = blocks(n)
    for j in range(n):
        b[j, 0] = (1023 if (j // 4 + j) & 1 else -1023) if j % 7 else int(rng.randint(-5, 6))
    out["dc11-422"] = (assemble(b, w, h, 3, 1), w, h)
    n = -(-w // 8) * -(-h // 8) * 3
    b = blocks(n)
    for j in range(n):
        b[j, 0] = int(rng.randint(-40, 41))
        b[j, 1 + j % 63] = int(rng.randint(512, 1024)) * (1 if j & 1 else -1)
    out["ac10-444"] = (assemble(b, w, h, 3, 0), w, h)
    # every AC symbol once and DC categories 0 .. 8 in both signs (the 12- to 4-bit DC codes), with Huffman codes of every length up
    # to 16 bits; the DC values stay small enough for the largest AC values to leave the IDCT inside its exact range
    tabs = long_code_tables()
    syms = tabs[1][1]
    for name, comps, ss, (w, h) in (("longcodes-gray", 1, 0, (112, 96)), ("longcodes-420", 3, 2, (96, 80))):
        n = -(-w // 16) * -(-h // 16) * 6 if comps == 3 else -(-w // 8) * -(-h // 8)
        assert n >= len(syms)
        b = blocks(n)
        dc = [0, 0, 0]
        comp = [0, 0, 0, 0, 1, 2] if comps == 3 else [0]
        for j in range(n):
            s = syms[j % len(syms)]
            run, size = s >> 4, s & 15
            if size:
                b[j, 1 + run] = _value(size, j & 1)
            elif run == 15:
                b[j, 1 + 16 + j % 40] = 5
            c = comp[j % len(comp)]
            cat = (j // len(comp)) % 9                                 # the DC difference's category, alternating signs
            diff = 0 if cat == 0 else _value(cat, dc[c] > 0)
            dc[c] += diff
            b[j, 0] = dc[c]
        out[name] = (assemble(b, w, h, comps, ss, tabs), w, h)
    # an all-zero page: every block is "DC 0, EOB", a periodic stream in which a wrong guess never resynchronises by itself.  With the
    # standard tables a luma block takes 6 bits and a chroma block 4: an MCU is 32 bits at 4:2:0 (a thread's range on a page this
    # small, so every guess is right), 20 at 4:2:2, 14 at 4:4:4 and 6 on a gray page
    w, h = 333, 250
    out["allzero-420"] = (assemble(blocks(-(-w // 16) * -(-h // 16) * 6), w, h, 3, 2), w, h)
    out["allzero-422"] = (assemble(blocks(-(-w // 16) * -(-h // 8) * 4), w, h, 3, 1), w, h)
    out["allzero-444"] = (assemble(blocks(-(-w // 8) * -(-h // 8) * 3), w, h, 3, 0), w, h)
    out["allzero-gray"] = (assemble(blocks(-(-w // 8) * -(-h // 8)), w, h, 1, 0), w, h)
    return out
