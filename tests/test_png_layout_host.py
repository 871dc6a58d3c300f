"""CPU tests of the host half of the PNG pixel layouts (csrc/rtn_png_layout.h, the layout inspector of csrc/rtn_png_stream.h; DESIGN
§3.4f "Pixel layouts"): the reference helper tests/png_layout_ref.py against Pillow, what rtn_png_layout_inspect accepts and
refuses, and the CPU twin (rtn_png_stream_inflate_host, then rtn_png_layout_pixels_host, which runs the device's geometry, filter
and expansion functions) against Pillow on the full grid of layouts, sizes and filters.  The same host code is a stand-alone
program for sanitizer builds (tools/png_layout_fuzz.cpp).  No kernel is launched here."""
import ctypes as C
import io
import os
import shutil
import struct
import subprocess
import sys
import warnings
import zlib

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_ref as R  # noqa: E402
import png_layout_ref as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS, HEIGHTS = (1, 2, 3, 5, 7, 8, 9, 17, 65), (1, 2, 5, 8, 9)


def pillow_bgr(data):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                 # Pillow warns about tRNS in palette files
        with Image.open(io.BytesIO(data)) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def inspect(pkg, data, with_blob=True, capacity=None, guard=0, which="layout"):
    """(rc, info, reason, blob array) of rtn_png_layout_inspect (or _stream_); `guard` bytes of 0xA5 follow the capacity."""
    L = pkg._lib
    info = L.PngInfo()
    cap = L.lib.rtn_png_layout_blob_bound(len(data)) if capacity is None else capacity
    blob = np.full(cap + guard, 0xa5, np.uint8)
    fn = getattr(L.lib, "rtn_png_%s_inspect" % which)
    rc = fn(None, data, len(data), C.byref(info), blob.ctypes.data if with_blob else None, cap)
    return rc, info, L.lib.rtn_last_error(None).decode(), blob


def twin(pkg, data, want, guard=64):
    """(status, (H,W,3) page or None) of the two host twins over one file; `want`: the filtered stream's length."""
    L = pkg._lib
    rc, info, why, blob = inspect(pkg, data)
    assert rc == 0, why
    stream = np.full(want + 2 * guard, 0xa5, np.uint8)
    st = C.c_int32(-1)
    rc = L.lib.rtn_png_stream_inflate_host(blob.ctypes.data, 0, stream.ctypes.data + guard, want, C.byref(st))
    assert rc == 0, L.lib.rtn_last_error(None)
    assert (stream[:guard] == 0xa5).all() and (stream[guard + want:] == 0xa5).all()
    if st.value:
        return st.value, None
    n = info.height * info.width * 3
    out = np.full(n + 2 * guard, 0xa5, np.uint8)
    rc = L.lib.rtn_png_layout_pixels_host(blob.ctypes.data, stream.ctypes.data + guard, want, out.ctypes.data + guard, C.byref(st))
    assert rc == 0, L.lib.rtn_last_error(None)
    assert (out[:guard] == 0xa5).all() and (out[guard + n:] == 0xa5).all()
    return st.value, (out[guard:guard + n].reshape(info.height, info.width, 3) if st.value == 0 else None)


# ---- the reference helper ---------------------------------------------------------------------------------------------------------------
def test_helper_agrees_with_pillow():
    rng = np.random.RandomState(1)
    n = 0
    for ctype, depth in P.ACCEPTED:
        for interlace in (0, 1):
            for w, h in ((1, 1), (9, 5), (17, 9)):
                samp = P.random_page(rng, w, h, ctype, depth)
                pal = P.random_palette(rng, max(1, (1 << depth) - 1)) if ctype == 3 else None
                data = P.write(samp, ctype, depth, interlace, rng, pad_ones=True, palette=pal)
                assert np.array_equal(pillow_bgr(data), P.expected_bgr(samp, ctype, depth, pal)), (ctype, depth, interlace, w, h)
                n += 1
    assert n == 14 * 2 * 3


def test_helper_can_fail():
    """A writer that packs sub-byte samples LSB first, and a statement of Pillow's conversion that takes the low byte of a 16-bit
    sample, both disagree with Pillow."""
    rng = np.random.RandomState(2)
    samp = P.random_page(rng, 9, 5, 0, 2)
    assert np.array_equal(pillow_bgr(P.write(samp, 0, 2)), P.expected_bgr(samp, 0, 2))
    assert not np.array_equal(pillow_bgr(P.write(samp, 0, 2, lsb_first=True)), P.expected_bgr(samp, 0, 2))
    samp = P.random_page(rng, 9, 5, 2, 16)
    assert np.array_equal(pillow_bgr(P.write(samp, 2, 16)), P.expected_bgr(samp, 2, 16))
    assert not np.array_equal(pillow_bgr(P.write(samp, 2, 16)), P.expected_bgr(samp, 2, 16, low_byte=True))


# ---- the twin on the full grid -------------------------------------------------------------------------------------------------------------
def test_twin_equals_pillow_on_the_full_grid(pkg):
    """Every accepted (type, depth) pair x interlace x 9 widths x 5 heights x filter 0 .. 4 and a random mix, padding bits ones, a
    palette one entry short of full (so indices past it occur); then every palette length for the palette depths.  No case may be
    skipped: Pillow reads all of these kinds."""
    rng = np.random.RandomState(3)
    ran = 0

    def case(ctype, depth, interlace, w, h, filters, npal):
        samp = P.random_page(rng, w, h, ctype, depth)
        pal = P.random_palette(rng, npal) if ctype == 3 else None
        data = P.write(samp, ctype, depth, interlace, filters, pad_ones=True, palette=pal, level=1)
        st, page = twin(pkg, data, P.stream_bytes(w, h, ctype, depth, interlace))
        assert st == 0, (ctype, depth, interlace, w, h, filters, npal, st)
        assert np.array_equal(page, pillow_bgr(data)), (ctype, depth, interlace, w, h, filters, npal)

    for ctype, depth in P.ACCEPTED:
        for interlace in (0, 1):
            for w in WIDTHS:
                for h in HEIGHTS:
                    for filters in (0, 1, 2, 3, 4, rng):
                        case(ctype, depth, interlace, w, h, filters, max(1, (1 << depth) - 1))
                        ran += 1
    for depth in (1, 2, 4, 8):
        for npal in (1, 2, (1 << depth) - 1, 1 << depth):
            for interlace in (0, 1):
                for w in WIDTHS:
                    for h in HEIGHTS:
                        case(3, depth, interlace, w, h, rng, npal)
                        ran += 1
    assert ran == 14 * 2 * 9 * 5 * 6 + 4 * 4 * 2 * 9 * 5


def test_twin_ignores_trns_and_a_suggested_palette(pkg):
    rng = np.random.RandomState(4)
    for ctype, depth, trns in ((0, 4, b"\x00\x03"), (2, 8, b"\x00\x01\x00\x02\x00\x03"), (3, 2, b"\x00\x80\xff")):
        samp = P.random_page(rng, 9, 5, ctype, depth)
        pal = P.random_palette(rng, 4) if ctype == 3 else None
        data = P.write(samp, ctype, depth, 1, rng, palette=pal, trns=trns)
        st, page = twin(pkg, data, P.stream_bytes(9, 5, ctype, depth, 1))
        assert st == 0 and np.array_equal(page, pillow_bgr(data)), ctype
    samp = P.random_page(rng, 9, 5, 6, 8)
    raw, _ = P.raw_stream(samp, 6, 8)
    data = P.wrap(9, 5, 6, 8, 0, zlib.compress(raw), palette=P.random_palette(rng, 7))
    st, page = twin(pkg, data, len(raw))
    assert st == 0 and np.array_equal(page, pillow_bgr(data))


def test_pixels_host_flags_a_filter_type_above_four(pkg):
    rng = np.random.RandomState(5)
    samp = P.random_page(rng, 17, 9, 0, 1)
    raw, offs = P.raw_stream(samp, 0, 1, 1, rng)
    assert len(offs) == 7
    bad = bytearray(raw)
    bad[offs[2]] = 5                                                     # the first row of pass 3
    data = P.wrap(17, 9, 0, 1, 1, zlib.compress(bytes(bad)))
    assert twin(pkg, data, len(raw)) == (128, None)


# ---- the inspector ----------------------------------------------------------------------------------------------------------------------
def test_inspector_accepts_each_kind(pkg, monkeypatch):
    """The stream length is what rtn_png_stream_inflate_host demands as want_bytes (any other value is RTN_EINVAL) and what the
    workspace is sized from."""
    monkeypatch.setenv("RTN_PNG_SEGMENT", "1024")
    L = pkg._lib
    rng = np.random.RandomState(6)
    for ctype, depth in P.ACCEPTED:
        for interlace in (0, 1):
            w, h = 65, 9
            samp = P.random_page(rng, w, h, ctype, depth)
            pal = P.random_palette(rng, 2) if ctype == 3 else None
            data = P.write(samp, ctype, depth, interlace, rng, palette=pal)
            rc, info, why, blob = inspect(pkg, data)
            assert rc == 0, why
            assert (info.width, info.height, info.components) == (w, h, P.SAMPLES[ctype])
            zbytes = sum(len(b) for k, b in R.parse_chunks(data) if k == b"IDAT")
            assert info.payload_bytes == zbytes and info.chunks == (zbytes - 6 + 1023) // 1024
            assert info.blob_bytes % 16 == 0 and 0 < info.blob_bytes <= L.lib.rtn_png_layout_blob_bound(len(data))
            want = P.stream_bytes(w, h, ctype, depth, interlace)
            assert info.workspace_bytes >= 3 * want
            out, st = np.zeros(want + 1, np.uint8), C.c_int32(-1)
            for wrong in (want - 1, want + 1):
                assert L.lib.rtn_png_stream_inflate_host(blob.ctypes.data, 0, out.ctypes.data, wrong, C.byref(st)) == -1
            assert L.lib.rtn_png_stream_inflate_host(blob.ctypes.data, 0, out.ctypes.data, want, C.byref(st)) == 0 and st.value == 0
            rc2, info2, _, _ = inspect(pkg, data, with_blob=False)
            assert rc2 == 0 and (info2.blob_bytes, info2.workspace_bytes) == (info.blob_bytes, info.workspace_bytes)
    # what the stream inspector takes, the layout inspector takes too
    data = P.write(P.random_page(rng, 9, 5, 2, 8), 2, 8)
    assert inspect(pkg, data)[0] == 0 and inspect(pkg, data, which="stream")[0] == 0


def small_files():
    rng = np.random.RandomState(7)
    pal = P.random_palette(rng, 4)
    samp = P.random_page(rng, 9, 5, 3, 2)
    raw, _ = P.raw_stream(samp, 3, 2)
    z = zlib.compress(raw)
    return rng, pal, samp, z


def test_inspector_refuses(pkg):
    rng, pal, samp, z = small_files()
    assert inspect(pkg, P.wrap(9, 5, 3, 2, 0, z, pal))[0] == 0
    gray16 = P.write(P.random_page(rng, 9, 5, 0, 16), 0, 16)
    assert pillow_bgr(gray16).shape == (5, 9, 3)
    refused = {
        "gray 16": gray16,
        "no PLTE": P.wrap(9, 5, 3, 2, 0, z),
        "PLTE after IDAT": P.wrap(9, 5, 3, 2, 0, z, pal, plte_after=True),
        "too many entries": P.wrap(9, 5, 3, 2, 0, z, P.random_palette(rng, 5)),
        "empty PLTE": P.wrap(9, 5, 3, 2, 0, z, np.zeros((0, 3), np.uint8)),
        "PLTE not a multiple of 3": P.wrap(9, 5, 3, 2, 0, z, before=[(b"PLTE", b"\x01\x02\x03\x04")]),
        "two PLTE": P.wrap(9, 5, 3, 2, 0, z, pal, before=[(b"PLTE", pal.tobytes())]),
        "PLTE in gray": P.wrap(9, 5, 0, 2, 0, z, pal),
        "bKGD": P.wrap(9, 5, 3, 2, 0, z, pal, before=[(b"bKGD", b"\x01")]),
        "unknown ancillary": P.wrap(9, 5, 3, 2, 0, z, pal, before=[(b"abCd", b"x")]),
        "interlace 2": P.wrap(9, 5, 3, 2, 2, z, pal),
    }
    for ctype, depths in ((0, (3, 5, 32)), (2, (1, 2, 4)), (3, (16,)), (4, (1, 2, 4)), (6, (4,)), (1, (8,)), (5, (8,)), (7, (8,))):
        for depth in depths:
            refused["type %d depth %d" % (ctype, depth)] = P.wrap(9, 5, ctype, depth, 0, z, pal)
    bad = bytearray(P.wrap(9, 5, 3, 2, 0, z, pal, before=[(b"tRNS", b"\x00\x80")]))
    bad[bad.index(b"tRNS") + 4] ^= 1                                     # a tRNS chunk with a stale CRC
    refused["tRNS CRC"] = bytes(bad)
    bad = bytearray(P.wrap(9, 5, 3, 2, 0, z, pal))
    bad[bad.index(b"PLTE") + 5] ^= 1
    refused["PLTE CRC"] = bytes(bad)
    for name, data in refused.items():
        rc, info, why, _ = inspect(pkg, data)
        assert rc == -1 and why and info.blob_bytes == 0, name


def test_inspector_refuses_every_truncation(pkg):
    rng, pal, samp, z = small_files()
    data = P.wrap(9, 5, 3, 2, 0, z, pal, before=[(b"tRNS", b"\x00\x80")], after=[(b"tEXt", b"k\x00v")])
    assert inspect(pkg, data)[0] == 0
    for cut in range(len(data)):
        rc, info, why, _ = inspect(pkg, data[:cut])
        assert rc == -1 and why and info.blob_bytes == 0, cut


def test_blob_capacity_is_respected(pkg):
    rng, pal, samp, z = small_files()
    data = P.wrap(9, 5, 3, 2, 0, z, pal)
    rc, info, why, blob = inspect(pkg, data)
    assert rc == 0, why
    need = info.blob_bytes
    assert bytes(pal.tobytes()) in blob[:need].tobytes()
    rc, _, why, blob = inspect(pkg, data, capacity=need - 1, guard=64)
    assert rc == -1 and "capacity" in why
    assert (blob == 0xa5).all()
    rc, _, _, blob = inspect(pkg, data, capacity=need, guard=64)
    assert rc == 0 and (blob[need:] == 0xa5).all() and not (blob[:need] == 0xa5).all()


def test_stream_inspector_still_refuses_the_new_kinds(pkg):
    rng = np.random.RandomState(8)
    n = 0
    for ctype, depth in P.ACCEPTED:
        for interlace in (0, 1):
            if (ctype, depth, interlace) in ((0, 8, 0), (2, 8, 0)):
                continue
            pal = P.random_palette(rng, 2) if ctype == 3 else None
            data = P.write(P.random_page(rng, 9, 5, ctype, depth), ctype, depth, interlace, palette=pal)
            assert inspect(pkg, data)[0] == 0
            rc, info, why, _ = inspect(pkg, data, which="stream")
            assert rc == -1 and why and info.blob_bytes == 0, (ctype, depth, interlace)
            n += 1
    assert n == 26
    data = P.write(P.random_page(rng, 9, 5, 2, 8), 2, 8, trns=b"\x00\x01\x00\x02\x00\x03")
    assert inspect(pkg, data)[0] == 0 and inspect(pkg, data, which="stream")[0] == -1


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------
def test_formats_and_knob(pkg, monkeypatch):
    PIO = __import__("importlib").import_module(pkg.__name__ + ".model.page_io")
    assert [f.name for f in PIO._FORMATS] == ["jpeg", "png", "png_stream"]
    assert [f.name for f in PIO._MORE_FORMATS] == ["png_layout"]
    # the dispatch gives the layout decoder only what the stream inspector refuses: ordinary PNGs are RTN_PNG_STREAM_MIN's to place
    plain = P.write(P.random_page(np.random.RandomState(0), 9, 5, 2, 8), 2, 8)
    info, blob = pkg._lib.PngInfo(), np.zeros(4096, np.uint8)
    assert PIO._MORE_FORMATS[0].inspect(None, plain, len(plain), C.byref(info), blob.ctypes.data, blob.size) == -1
    assert not blob.any()
    assert PIO.png_layout_inspect(plain)[0] is not None
    monkeypatch.delenv("RTN_PNG_LAYOUT_MIN", raising=False)
    assert PIO.png_layout_min() == PIO.PNG_LAYOUT_MIN_DEFAULT >= 0
    for value, want in (("3", 3), ("0", 0), ("-2", 0), ("x", PIO.PNG_LAYOUT_MIN_DEFAULT), ("", PIO.PNG_LAYOUT_MIN_DEFAULT)):
        monkeypatch.setenv("RTN_PNG_LAYOUT_MIN", value)
        assert PIO.png_layout_min() == want, value
    rng = np.random.RandomState(9)
    data = P.write(P.random_page(rng, 9, 5, 6, 8), 6, 8, 1)
    info, blob = PIO.png_layout_inspect(data)
    assert (info.width, info.height, info.components) == (9, 5, 4) and len(blob) == info.blob_bytes
    assert PIO.png_stream_inspect(data)[0] is None
    info, why = PIO.png_layout_inspect(P.write(P.random_page(rng, 9, 5, 0, 16), 0, 16))
    assert info is None and "16-bit gray" in why


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_cabi_surface(pkg):
    L = pkg._lib
    sz, i, p = C.c_size_t, C.c_int, C.c_void_p
    want = {
        "rtn_png_layout_blob_bound": (sz, [sz]),
        "rtn_png_layout_inspect": (i, [p, p, sz, C.POINTER(L.PngInfo), p, sz]),
        "rtn_png_layout_decode_workspace_bytes": (sz, [i, p, p]),
        "rtn_png_layout_decode": (i, [p, i, p, p, p, p, p, p, sz]),
        "rtn_png_layout_pixels_host": (i, [p, p, sz, p, C.POINTER(C.c_int32)]),
    }
    lib = C.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rtn.h")).read()
    for name, sig in want.items():
        assert hasattr(lib, name), name
        assert L.SIGNATURES[name] == sig, name
        assert name + "(" in header
    for name in ("inspect", "decode_workspace_bytes", "decode"):
        assert L.SIGNATURES["rtn_png_layout_" + name] == L.SIGNATURES["rtn_png_stream_" + name]
    assert L.lib.rtn_png_layout_blob_bound(1000) >= L.lib.rtn_png_stream_blob_bound(1000)
    rng, pal, samp, z = small_files()
    data = P.wrap(9, 5, 3, 2, 0, z, pal)
    info = L.PngInfo()
    assert L.lib.rtn_png_layout_inspect(None, data, len(data), None, None, 0) == -1
    assert L.lib.rtn_png_layout_inspect(None, None, 10, C.byref(info), None, 0) == -1
    assert L.lib.rtn_png_layout_inspect(None, data, 0, C.byref(info), None, 0) == -1
    rc, info, _, blob = inspect(pkg, data)
    offs = np.zeros(1, np.int64)
    assert L.lib.rtn_png_layout_decode_workspace_bytes(1, blob.ctypes.data, offs.ctypes.data) == info.workspace_bytes
    assert L.lib.rtn_png_layout_decode_workspace_bytes(0, blob.ctypes.data, offs.ctypes.data) == 0
    assert L.lib.rtn_png_layout_decode(None, 1, None, None, None, None, None, None, 0) == -1
    # each decoder takes its own inspector's blobs only
    assert L.lib.rtn_png_stream_decode_workspace_bytes(1, blob.ctypes.data, offs.ctypes.data) == 0
    plain = P.write(P.random_page(rng, 9, 5, 2, 8), 2, 8)
    _, _, _, sblob = inspect(pkg, plain, which="stream")
    assert L.lib.rtn_png_layout_decode_workspace_bytes(1, sblob.ctypes.data, offs.ctypes.data) == 0
    want_bytes = P.stream_bytes(9, 5, 3, 2, 0)
    stream, out, st = np.zeros(want_bytes, np.uint8), np.zeros(9 * 5 * 3, np.uint8), C.c_int32(0)
    args = (blob.ctypes.data, stream.ctypes.data, want_bytes, out.ctypes.data, C.byref(st))
    assert L.lib.rtn_png_layout_pixels_host(*args) == 0 and st.value == 0
    for k in (0, 1, 3, 4):
        assert L.lib.rtn_png_layout_pixels_host(*[None if j == k else a for j, a in enumerate(args)]) == -1
    assert L.lib.rtn_png_layout_pixels_host(blob.ctypes.data, stream.ctypes.data, want_bytes - 1, out.ctypes.data, C.byref(st)) == -1
    assert L.lib.rtn_png_layout_pixels_host(sblob.ctypes.data, stream.ctypes.data, want_bytes, out.ctypes.data, C.byref(st)) == -1


# ---- the same host code as a program of its own -------------------------------------------------------------------------------------------------
def test_stand_alone_fuzz_program(tmp_path):
    """tools/png_layout_fuzz.cpp is the program the sanitizer runs use (its header has the -fsanitize command line).  Here it is
    built without a sanitizer."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "png_layout_fuzz"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "retinanet-for-table-detection_amd", "csrc"),
                           os.path.join(ROOT, "tools", "png_layout_fuzz.cpp"), "-o", str(exe)])
    rng = np.random.RandomState(10)
    files = []
    for k, (ctype, depth, interlace) in enumerate(((0, 1, 0), (3, 4, 1), (6, 8, 1), (2, 16, 0), (4, 16, 1))):
        f = tmp_path / ("f%d.png" % k)
        pal = P.random_palette(rng, 9) if ctype == 3 else None
        f.write_bytes(P.write(P.random_page(rng, 65, 33, ctype, depth, smooth=True), ctype, depth, interlace, rng, palette=pal))
        files.append(str(f))
    run = subprocess.run([str(exe), "80"] + files, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "mutated or cut blobs 400" in run.stdout.splitlines()[-1]
