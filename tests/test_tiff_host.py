"""CPU tests of the host half of the TIFF decoder (csrc/rtn_tiff_decode.h): the reference helper tests/tiff_ref.py
against Pillow, what rtn_tiff_inspect accepts and refuses, and the CPU twin rtn_tiff_decode_host (the device's PackBits, LZW, Group 4,
Deflate and pixel functions behind a context that checks every position) against Pillow on the full grid of compressions, layouts,
sizes and strip heights, on the Group 4 / LZW / PackBits corner cases and on damaged streams.  The same host code is a stand-alone
program for sanitizer builds (tools/tiff_fuzz.cpp).  No kernel is launched here."""
import ctypes as C
import io
import os
import struct
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_ref as T  # noqa: E402

TF_SHORT, TF_OVER = 1 << 18, 1 << 19


def inspect(pkg, data, with_blob=True, capacity=None, guard=0):
    """(rc, info, reason, blob array) of rtn_tiff_inspect; `guard` bytes of 0xA5 follow the capacity."""
    L = pkg._lib
    info = L.TiffInfo()
    cap = L.lib.rtn_tiff_blob_bound(len(data)) if capacity is None else capacity
    blob = np.full(cap + guard, 0xa5, np.uint8)
    rc = L.lib.rtn_tiff_inspect(None, data, len(data), C.byref(info), blob.ctypes.data if with_blob else None, cap)
    return rc, info, L.lib.rtn_last_error(None).decode(), blob


def twin(pkg, data, guard=64):
    """(status, (H,W,3) page or None) of the host twin over one file; the guard bytes around the page must stay."""
    L = pkg._lib
    rc, info, why, blob = inspect(pkg, data)
    assert rc == 0, why
    n = info.height * info.width * 3
    out = np.full(n + 2 * guard, 0xa5, np.uint8)
    st = C.c_int32(-1)
    rc = L.lib.rtn_tiff_decode_host(blob.ctypes.data, out.ctypes.data + guard, n, C.byref(st))
    assert rc == 0, L.lib.rtn_last_error(None)
    assert (out[:guard] == 0xa5).all() and (out[guard + n:] == 0xa5).all()
    if st.value:
        assert (out == 0xa5).all()                                       # a flagged page is not written
        return st.value, None
    return 0, out[guard:guard + n].reshape(info.height, info.width, 3)


def same_as_pillow(pkg, data, label=""):
    st, page = twin(pkg, data)
    assert st == 0, (label, hex(st))
    assert np.array_equal(page, T.pillow_bgr(data)), label


def gray_file(rows, w, rps, encode, compression, **kw):
    """A gray (or, with bits=(1,), bilevel) file of the byte rows `rows`, each strip encoded by `encode`."""
    strips = [encode(b"".join(rows[y:y + rps])) for y in range(0, len(rows), rps)]
    return T.write_tiff(strips, w, len(rows), rps, compression=compression, **kw)


# ---- the reference helper ---------------------------------------------------------------------------------------------------------------
def test_entry_points_exist(pkg):
    """Fails without the feature."""
    for name in ("rtn_tiff_blob_bound", "rtn_tiff_inspect", "rtn_tiff_decode_workspace_bytes", "rtn_tiff_decode", "rtn_tiff_decode_host"):
        assert hasattr(pkg._lib.lib, name)
    import importlib
    PIO = importlib.import_module("retinanet-for-table-detection_amd.model.page_io")
    assert PIO.tiff_min() >= 0 and callable(PIO.tiff_inspect) and callable(PIO.decode_tiff_bgr)
    assert [f.name for f in PIO._ALL_FORMATS] == ["jpeg", "png", "png_stream", "png_layout", "tiff"]


def test_helper_agrees_with_pillow():
    rng = np.random.RandomState(1)
    for w, h, rps in ((1, 1, 1), (17, 5, 2), (65, 9, 3), (300, 40, 40), (64, 7, 50)):
        a = (np.cumsum(rng.randint(0, 3, (h, w)), axis=1) & 255).astype(np.uint8)
        a[h // 2] = 7                                                    # a long repeat run
        rows = [r.tobytes() for r in a]
        want = np.repeat(a[:, :, None], 3, axis=2)
        for be in (False, True):
            for long_fields in (False, True):
                for encode, comp in ((bytes, 1), (T.packbits_encode, 32773), (T.lzw_encode, 5), (T.zlib_strip, 8)):
                    data = gray_file(rows, w, min(rps, h) if rps <= h else rps, encode, comp, big_endian=be, long_fields=long_fields)
                    assert np.array_equal(T.pillow_bgr(data), want), (w, h, rps, comp, be)
        raw = b"".join(rows)
        assert T.packbits_decode(T.packbits_encode(raw), len(raw)) == raw
        assert T.lzw_decode(T.lzw_encode(raw), len(raw))[0] == raw
        im = Image.fromarray(a)
        for comp, decode in (("packbits", T.packbits_decode), ("tiff_lzw", lambda s, n: T.lzw_decode(s, n)[0])):
            data = T.pillow_tiff(im, comp)
            f = T.read_fields(data)
            strips = [data[o:o + c] for o, c in zip(f[273][1], f[279][1])]
            assert len(strips) == 1 and decode(strips[0], len(raw)) == raw   # the helper's decoders read Pillow's strips
        assert T.pillow_bgr(T.rewrap(T.pillow_tiff(im, "tiff_lzw"), big_endian=True, long_fields=True)).tolist() == want.tolist()


# ---- the inspector ------------------------------------------------------------------------------------------------------------------------
def test_inspector_accepts(pkg):
    rng = np.random.RandomState(2)
    for comp, number in T.COMPRESSIONS.items():
        for mode in T.LAYOUTS:
            if not T.applies(comp, mode, 1):
                continue
            im = T.random_image(rng, mode, 33, 9)
            for be in (False, True):
                data = T.rewrap(T.pillow_tiff(im, comp, {278: 4}), big_endian=be, long_fields=be,
                                extra=[(296, T.SHORT, [2]), (305, 2, b"scanner\0")])     # resolution unit, software: ignored
                rc, info, why, blob = inspect(pkg, data)
                assert rc == 0, (comp, mode, why)
                assert (info.width, info.height, info.strips, info.compression) == (33, 9, 3, number)
                assert (info.components, info.bits) == (3 if mode == "RGB" else 1, 1 if mode == "1" else 8)
                assert info.blob_bytes % 16 == 0 and 0 < info.blob_bytes <= pkg._lib.lib.rtn_tiff_blob_bound(len(data))
                rc2, info2, _, _ = inspect(pkg, data, with_blob=False)
                assert rc2 == 0 and info2.blob_bytes == info.blob_bytes
    data = T.rewrap(T.pillow_tiff(T.random_image(rng, "L", 8, 4), "tiff_adobe_deflate"), extra=[(259, T.SHORT, [32946])])
    rc, info, why, _ = inspect(pkg, data)
    assert rc == 0 and info.compression == 8, why
    same_as_pillow(pkg, data)


def refused_files():
    rng = np.random.RandomState(3)
    gray = T.random_image(rng, "L", 16, 8)
    rgb = T.random_image(rng, "RGB", 16, 8)
    bw = T.random_image(rng, "1", 16, 8)
    base = T.pillow_tiff(gray, "raw")
    rows = [bytes(16)] * 8
    cases = [
        ("tiles", T.rewrap(base, extra=[(322, T.SHORT, [16]), (323, T.SHORT, [16])])),
        ("BigTIFF", base[:2] + struct.pack("<H", 43) + base[4:]),
        ("Group 3", T.rewrap(T.pillow_tiff(bw, "group3"))),
        ("JPEG", T.rewrap(base, extra=[(259, T.SHORT, [7])])),
        ("old-style LZW", T.write_tiff([b"\x00\x01" + bytes(30)], 16, 8, 8, compression=5)),
        ("2-bit", T.write_tiff([bytes(32)], 16, 8, 8, bits=(2,))),
        ("4-bit", T.write_tiff([bytes(64)], 16, 8, 8, bits=(4,))),
        ("16-bit", T.write_tiff([bytes(256)], 16, 8, 8, bits=(16,))),
        ("CMYK", T.write_tiff([bytes(512)], 16, 8, 8, bits=(8, 8, 8, 8), photometric=5)),
        ("ExtraSamples", T.write_tiff([bytes(512)], 16, 8, 8, bits=(8, 8, 8, 8), photometric=2, extra=[(338, T.SHORT, [2])])),
        ("PhotometricInterpretation 6", T.rewrap(T.pillow_tiff(rgb, "raw"), extra=[(262, T.SHORT, [6])])),
        ("PhotometricInterpretation 8", T.rewrap(T.pillow_tiff(rgb, "raw"), extra=[(262, T.SHORT, [8])])),
        ("ExtraSamples", T.rewrap(base, extra=[(338, T.SHORT, [1])])),
        ("PlanarConfiguration 2", T.rewrap(T.pillow_tiff(rgb, "raw"), extra=[(284, T.SHORT, [2])])),
        ("T6Options", T.rewrap(T.pillow_tiff(bw, "group4"), extra=[(293, T.LONG, [2])])),
        ("Orientation 3", T.rewrap(base, extra=[(274, T.SHORT, [3])])),
        ("Predictor 2", T.rewrap(T.pillow_tiff(bw, "tiff_lzw"), extra=[(317, T.SHORT, [2])])),
        ("Predictor 2", T.rewrap(base, extra=[(317, T.SHORT, [2])])),
        ("FillOrder 2", T.rewrap(base, extra=[(266, T.SHORT, [2])])),
        ("ColorMap", T.rewrap(T.pillow_tiff(T.random_image(rng, "P", 16, 8), "raw"), omit=[320])),
        ("IFD lies outside", base[:4] + struct.pack("<I", len(base) + 10) + base[8:]),
        ("outside the file", T.rewrap(base, extra=[(273, T.LONG, [len(base) * 2])])),
        ("outside the file", T.rewrap(base, extra=[(279, T.LONG, [len(base) * 2])])),
        ("outside the file", T.rewrap(base, extra=[(258, T.SHORT, [8, 8, 8]), (277, T.SHORT, [3]), (262, T.SHORT, [2])])[:-40]),
        ("bytes for", T.write_tiff([b"".join(rows)[:-1]], 16, 8, 8)),
        ("overlap", T.write_tiff([bytes(1)] * 3, 1, 3, 1, compression=32773, extra=[(273, T.SHORT, [8, 8, 8]), (279, T.SHORT, [60, 60, 60])])),
        ("strip offsets", T.rewrap(base, extra=[(278, T.SHORT, [3])])),
        ("not a TIFF", b"\x89PNG\r\n\x1a\n" + bytes(40)),
        ("single strip", T.pillow_tiff(T.random_image(rng, "1", 16, 80), "group4", {278: 80})),
    ]
    return cases


def test_inspector_refuses(pkg, monkeypatch):
    monkeypatch.delenv("RTN_TIFF_G4_ONE_STRIP", raising=False)
    for reason, data in refused_files():
        rc, info, why, blob = inspect(pkg, data, guard=16)
        assert rc != 0 and reason in why, (reason, why)
        assert info.blob_bytes == 0 and info.width == 0
        assert (blob == 0xa5).all(), reason                               # a refused file writes nothing
    monkeypatch.setenv("RTN_TIFF_G4_ONE_STRIP", "1")
    data = refused_files()[-1][1]
    rc, info, why, _ = inspect(pkg, data)
    assert rc == 0 and info.strips == 1, why
    same_as_pillow(pkg, data)


def test_inspector_writes_nothing_past_its_capacity(pkg):
    rng = np.random.RandomState(4)
    for comp in T.COMPRESSIONS:
        mode = "1" if comp == "group4" else "P"
        data = T.pillow_tiff(T.random_image(rng, mode, 37, 11), comp, {278: 3})
        rc, info, why, _ = inspect(pkg, data, with_blob=False)
        assert rc == 0, why
        rc, info2, why, blob = inspect(pkg, data, capacity=info.blob_bytes, guard=64)
        assert rc == 0 and info2.blob_bytes == info.blob_bytes and (blob[info.blob_bytes:] == 0xa5).all()
        rc, info3, why, blob = inspect(pkg, data, capacity=info.blob_bytes - 1, guard=64)
        assert rc != 0 and "blob_capacity" in why and (blob == 0xa5).all() and info3.blob_bytes == 0
        for cut in list(range(0, 16)) + [len(data) // 2, len(data) - 1]:  # a prefix never gets past the inspector's checks
            rc, _, _, blob = inspect(pkg, data[:cut], capacity=pkg._lib.lib.rtn_tiff_blob_bound(cut), guard=16)
            assert rc != 0 and (blob == 0xa5).all(), cut


# ---- the twin against Pillow ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compression", list(T.COMPRESSIONS))
def test_twin_grid(pkg, compression):
    files = T.corpus(compression)
    layouts = sum(T.applies(compression, m, 1) for m in T.LAYOUTS)
    assert len(files) == layouts * len(T.WIDTHS) * len(T.HEIGHTS) * 5
    marks = set()
    for label, data in files:
        same_as_pillow(pkg, data, label)
        f = T.read_fields(data)
        marks.add((data[:2], f[262][1][0], f.get(266, (0, [1]))[1][0], f.get(317, (0, [1]))[1][0]))
    assert {m[0] for m in marks} == {b"II", b"MM"}
    if compression in ("tiff_lzw", "tiff_adobe_deflate"):
        assert {m[3] for m in marks} == {1, 2}
    assert {0, 1} <= {m[1] for m in marks} and {m[2] for m in marks} == {1, 2}


def g4(a, info=None):
    return T.pillow_tiff(Image.fromarray(a), "group4", info)


def test_group4_modes_and_long_runs(pkg, monkeypatch):
    monkeypatch.setenv("RTN_TIFF_G4_ONE_STRIP", "1")
    # every vertical mode: the run of row 2 k + 1 starts d = -3 .. 3 pixels from the one above it (T.6 codes |d| <= 3 vertically)
    a = np.zeros((14, 40), bool)
    for k, d in enumerate(range(-3, 4)):
        a[2 * k, 10:20] = True
        a[2 * k + 1, 10 + d:20 + (d if d % 2 else 0)] = True
    same_as_pillow(pkg, g4(a), "vertical")
    # pass mode: the row above has a run the coded row lacks; horizontal: a run far from every change above
    a = np.zeros((4, 60), bool)
    a[0, 5:9] = a[0, 30:34] = True
    a[1, 30:34] = True
    a[2, 50:58] = True
    a[3, 2:3] = a[3, 20:21] = a[3, 50:60] = True
    same_as_pillow(pkg, g4(a), "pass and horizontal")
    # extended make-up codes (a white run of 1792 or more), repeated make-up (above 2560), black make-up codes
    for w, x in ((3000, 2990), (5300, 5290)):
        a = np.zeros((3, w), bool)
        a[0, x] = True
        a[1, 100:w - 100] = True                                         # a black run of thousands
        a[2, :70] = a[2, 200:200 + 64] = True
        for rps in (1, 3):
            same_as_pillow(pkg, g4(a, {278: rps}), "%d rps %d" % (w, rps))
    # all white, all black, rows ending in each colour, strips of one row, either photometric and fill order
    rng = np.random.RandomState(5)
    for a in (np.zeros((5, 33), bool), np.ones((5, 33), bool), np.tri(9, 17, dtype=bool), ~np.tri(9, 17, dtype=bool), rng.random_sample((9, 70)) < 0.3):
        for info in ({}, {278: 1}, {262: 0}, {266: 2, 278: 2}):
            same_as_pillow(pkg, g4(a, info), str(info))
    # every run length 0 .. 2623 of either colour, in strips of one row (so every change is coded horizontally)
    w = 2700
    a = np.zeros((2 * 42, w), bool)
    for k in range(42):
        x = 0
        for j in range(64):
            n = (k * 64 + j) % 2624
            if x + n + 1 > w:
                break
            a[2 * k, x + n] = True                                       # white run n, then one black pixel
            x += n + 1
        a[2 * k + 1] = ~a[2 * k]
    same_as_pillow(pkg, g4(a, {278: 1}), "run lengths")


def test_group4_with_and_without_eofb(pkg):
    a = np.random.RandomState(6).random_sample((6, 50)) < 0.4
    data = g4(a, {278: 3})
    f = T.read_fields(data)
    strips = [data[o:o + c] for o, c in zip(f[273][1], f[279][1])]
    eofb = [s for s in strips if "000000000001000000000001" in bin(int.from_bytes(s, "big"))[2:].zfill(8 * len(s))]
    assert len(eofb) == len(strips)                                      # libtiff ends every strip with EOFB
    want = T.pillow_bgr(data)
    for cut in (0, 3):                                                   # without EOFB: the last three bytes hold it
        bare = T.write_tiff([s[:len(s) - cut] for s in strips], 50, 6, 3, compression=4, bits=(1,), photometric=f[262][1][0])
        st, page = twin(pkg, bare)
        assert st == 0 and np.array_equal(page, want), cut


def test_lzw_noise_strip_and_no_eoi(pkg):
    rng = np.random.RandomState(7)
    w, h = 128, 160
    a = rng.randint(0, 256, (h, w)).astype(np.uint8)
    a[80, :100] = 97                                                     # "aaaa...": the code being defined (KwKwK)
    raw = a.tobytes()
    strip = T.lzw_encode(raw)
    back, stats = T.lzw_decode(strip, len(raw))
    assert back == raw
    assert stats["clears"] >= 3 and stats["widths"] == {9, 10, 11, 12} and stats["kwkwk"] >= 1, stats
    want = np.repeat(a[:, :, None], 3, axis=2)
    for s in (strip, T.lzw_encode(raw, eoi=False)):
        data = T.write_tiff([s], w, h, h, compression=5)
        assert np.array_equal(T.pillow_bgr(data), want)
        st, page = twin(pkg, data)
        assert st == 0 and np.array_equal(page, want)
    pil = T.pillow_tiff(Image.fromarray(a), "tiff_lzw", {278: h})     # libtiff's own encoding of the same strip
    f = T.read_fields(pil)
    _, stats = T.lzw_decode(pil[f[273][1][0]:f[273][1][0] + f[279][1][0]], len(raw))
    assert stats["clears"] >= 3 and stats["widths"] == {9, 10, 11, 12}
    same_as_pillow(pkg, pil)


def test_packbits_hand_packed_runs(pkg):
    w, h = 40, 8                                                         # 320 bytes in one strip
    parts = [
        (b"\x00\x11", b"\x11"),                                          # literal run of 1
        (b"\x00\x12", b"\x12"),
        (bytes([255, 7, 128]), b"\x07\x07"),                            # repeat run of 2 (-1), then the no-op -128
        (bytes([129, 9]), b"\x09" * 128),                                # repeat run of 128: crosses rows 0 .. 3
        (bytes([127]) + bytes(range(128)), bytes(range(128))),           # literal run of 128: crosses rows 3 .. 6
        (bytes([128, 128, 0, 1]), b"\x01"),                              # no-ops, then a repeat "run" of 1 (0 = one literal)
        (bytes([257 - 59, 200]), b"\xc8" * 59),
    ]
    strip, raw = b"".join(p[0] for p in parts), b"".join(p[1] for p in parts)
    assert len(raw) == w * h and T.packbits_decode(strip, w * h) == raw
    data = T.write_tiff([strip], w, h, h, compression=32773)
    want = np.repeat(np.frombuffer(raw, np.uint8).reshape(h, w)[:, :, None], 3, axis=2)
    assert np.array_equal(T.pillow_bgr(data), want)
    st, page = twin(pkg, data)
    assert st == 0 and np.array_equal(page, want)
    st, _ = twin(pkg, T.write_tiff([strip[:-1]], w, h, h, compression=32773))
    assert st & TF_SHORT
    st, _ = twin(pkg, T.write_tiff([strip[:-2] + bytes([257 - 60, 200])], w, h, h, compression=32773))
    assert st & TF_OVER


def damaged_files(seed=8, flips=6):
    """[(label, bytes)]: the valid files of every compression with bytes of their strip data changed, and with strips cut short."""
    rng = np.random.RandomState(seed)
    out = []
    for comp in ("packbits", "tiff_lzw", "tiff_adobe_deflate", "group4"):
        for mode in ("1", "RGB"):
            if not T.applies(comp, mode, 1):
                continue
            im = T.random_image(rng, mode, 150, 23, density=0.2)
            if mode == "RGB":
                im = Image.fromarray((np.cumsum(rng.randint(0, 2, (23, 150, 3)), axis=1) & 255).astype(np.uint8))
            data = T.pillow_tiff(im, comp, {278: 8})
            f = T.read_fields(data)
            for k in range(flips):
                s = rng.randint(len(f[273][1]))
                o, c = f[273][1][s], f[279][1][s]
                b = bytearray(data)
                b[o + rng.randint(c)] ^= 1 << rng.randint(8)
                if k % 2:
                    b[o + rng.randint(c)] = rng.randint(256)
                out.append(("%s %s flip %d" % (comp, mode, k), bytes(b)))
            strips = [data[o:o + c] for o, c in zip(f[273][1], f[279][1])]
            for cut in (1, 2, len(strips[-1]) // 2):
                cutted = strips[:-1] + [strips[-1][:len(strips[-1]) - cut]]
                out.append(("%s %s cut %d" % (comp, mode, cut), T.write_tiff(
                    cutted, 150, 23, 8, compression=T.COMPRESSIONS[comp], bits=tuple(f[258][1]) if 258 in f else (1,),
                    photometric=f[262][1][0], samples=f[277][1][0] if 277 in f else 1)))
    return out


def pillow_or_none(data, size):
    try:
        page = T.pillow_bgr(data)
    except Exception:
        return None
    return page if page.shape[:2] == size else None


def test_damaged_streams(pkg):
    files = damaged_files()
    assert len(files) >= 50
    flagged = 0
    for label, data in files:
        st, page = twin(pkg, data)                                       # never crashes; the guard bytes are checked inside
        if st == 0:
            want = pillow_or_none(data, page.shape[:2])
            assert want is not None and np.array_equal(page, want), label
        else:
            flagged += 1
    assert flagged >= len(files) // 4
