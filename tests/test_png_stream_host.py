"""CPU tests of the host half of the stream PNG decoder (csrc/rtn_png_stream.h): the reference helper
tests/png_stream_ref.py against Pillow, what rtn_png_stream_inspect accepts and what it leaves to Pillow, and
rtn_png_stream_inflate_host, which runs the device's find, count, chain, marker-decode, window and resolve functions
(csrc/rtn_png_inflate.h) on a CPU, against zlib on streams of every shape and on mutated and truncated copies.  The same host code
is also a stand-alone program for sanitizer builds (tools/png_stream_fuzz.cpp).  No kernel is launched here."""
import ctypes as C
import io
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image
from PIL.PngImagePlugin import PngInfo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_ref as R  # noqa: E402
import png_stream_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEGMENTS = (256, 1024, 4096, 1 << 20)


@pytest.fixture(scope="module")
def crops():
    """The three crops of tests/test_gpu_png_decode.py::crops: distance map, gray page, R,G,B page."""
    m = np.asarray(Image.open(os.path.join(GOLDEN, "sample_0717_023.jpg")).convert("RGB"))[:, :, ::-1]
    o = Image.open(os.path.join(GOLDEN, "sample_0717_023_orig.jpg"))
    page, gray = np.asarray(o.convert("RGB"))[:, :, ::-1], np.asarray(o.convert("L"))
    return [np.ascontiguousarray(m[300:397, 200:313]), np.ascontiguousarray(gray[1000:1300, 200:533]),
            np.ascontiguousarray(page[1000:1111, 3:1000])]


@pytest.fixture(scope="module")
def streams(crops):
    """[(name, w, h, c, filtered stream, raw deflate data)]: every stream shape of the 300x333 gray crop and the 111x997 page crop."""
    out = []
    for label, pg in (("gray", crops[1]), ("page", crops[2])):
        raw = R.filter_rows(pg, "minsum")
        for name, d in S.deflate_shapes(raw):
            out.append((label + "-" + name, *dims(pg), raw, d))
    return out


def dims(page):
    return page.shape[1], page.shape[0], (3 if page.ndim == 3 else 1)


def pillow_png(page, **kw):
    b = io.BytesIO()
    img = page if isinstance(page, Image.Image) else Image.fromarray(page[:, :, ::-1] if page.ndim == 3 else page)
    img.save(b, "PNG", **kw)
    return b.getvalue()


def host_rows(data):
    with Image.open(io.BytesIO(data)) as im:
        a = np.asarray(im)
    return a.reshape(a.shape[0], -1)


def inspect(pkg, data, with_blob=True, capacity=None, guard=0):
    """(rc, info, reason, blob array) of rtn_png_stream_inspect; `guard` bytes of 0xA5 follow the capacity."""
    L = pkg._lib
    info = L.PngInfo()
    cap = L.lib.rtn_png_stream_blob_bound(len(data)) if capacity is None else capacity
    blob = np.full(cap + guard, 0xa5, np.uint8)
    rc = L.lib.rtn_png_stream_inspect(None, data, len(data), C.byref(info), blob.ctypes.data if with_blob else None, cap)
    return rc, info, L.lib.rtn_last_error(None).decode(), blob


def twin(pkg, data, segment, want, guard=64):
    """(status, bytes written to out[0:want], whether the guards around out are intact) of rtn_png_stream_inflate_host."""
    L = pkg._lib
    rc, info, why, blob = inspect(pkg, data)
    assert rc == 0, why
    buf = np.full(want + 2 * guard, 0xa5, np.uint8)
    st = C.c_int32(-1)
    rc = L.lib.rtn_png_stream_inflate_host(blob.ctypes.data, segment, buf.ctypes.data + guard, want, C.byref(st))
    assert rc == 0, L.lib.rtn_last_error(None)
    intact = bool((buf[:guard] == 0xa5).all() and (buf[guard + want:] == 0xa5).all())
    return st.value, buf[guard:guard + want].tobytes(), intact


# ---- the reference helper ---------------------------------------------------------------------------------------------------------------
def helper_pages():
    rng = np.random.RandomState(2)
    for w in (1, 2, 3, 64):
        for h in (1, 2, 9):
            for c in (1, 3):
                page = rng.randint(0, 256, (h, w) if c == 1 else (h, w, 3)).astype(np.uint8)
                for t in range(6):
                    yield page, (np.full(h, t) if t < 5 else rng.randint(0, 5, h))


def test_helper_agrees_with_pillow():
    n = 0
    for page, types in helper_pages():
        w, h, c = dims(page)
        raw = S.filter_page(page, types)
        assert list(np.frombuffer(raw, np.uint8).reshape(h, -1)[:, 0]) == list(types)
        want = R.rgb_of(page).reshape(h, w * c)
        assert np.array_equal(S.unfilter(raw, w, h, c), want)
        data = S.assemble(w, h, c, zlib.compress(raw), cuts=[3, 3, 5] if len(zlib.compress(raw)) > 5 else None,
                          before=[(b"pHYs", struct.pack(">IIB", 2835, 2835, 1))], after=[(b"tEXt", b"Comment\x00x")])
        assert np.array_equal(host_rows(data), want)
        n += 1
    assert n == 4 * 3 * 2 * 6


def test_helper_can_fail():
    """A Paeth predictor whose ties go to the upper-left pixel decodes other pixels than Pillow does."""
    rng = np.random.RandomState(4)
    page = rng.randint(0, 256, (9, 64, 3)).astype(np.uint8)
    raw = S.filter_page(page, np.full(9, 4))
    want = host_rows(S.assemble(64, 9, 3, zlib.compress(raw)))
    assert np.array_equal(S.unfilter(raw, 64, 9, 3), want)
    assert not np.array_equal(S.unfilter(raw, 64, 9, 3, wrong_paeth=True), want)


# ---- the inspector ----------------------------------------------------------------------------------------------------------------------
def recut(data, cuts, empties=False):
    """The file with its zlib stream cut into IDATs at `cuts` (with an empty IDAT at every cut if asked)."""
    chunks = R.parse_chunks(data)
    z = b"".join(b for k, b in chunks if k == b"IDAT")
    (w, h), ctype = struct.unpack(">II", chunks[0][1][:8]), chunks[0][1][9]
    cuts = [c for c in cuts if c < len(z)]
    if empties:
        cuts = sorted(cuts + cuts)
    first = [k for k, _ in chunks].index(b"IDAT")
    return S.assemble(w, h, 3 if ctype == 2 else 1, z, cuts=cuts, before=chunks[1:first])


def test_accepts_pillow_files(pkg, crops, monkeypatch):
    monkeypatch.setenv("RTN_PNG_SEGMENT", "1024")
    meta = PngInfo()
    meta.add_text("Title", "a page")
    for page in crops:
        w, h, c = dims(page)
        for kw in ({}, {"compress_level": 1}, {"dpi": (72, 72)}, {"pnginfo": meta}):
            data = pillow_png(page, **kw)
            variants = [data] + [recut(data, S.every(len(data), n), e) for n in (1, 7, 65536) for e in (False, True)]
            for v in variants:
                assert np.array_equal(host_rows(v), R.rgb_of(page).reshape(h, w * c))
                rc, info, why, blob = inspect(pkg, v)
                assert rc == 0, why
                assert (info.width, info.height, info.components) == (w, h, c)
                zbytes = sum(len(b) for k, b in R.parse_chunks(v) if k == b"IDAT")
                assert info.payload_bytes == zbytes and info.chunks == (zbytes - 6 + 1023) // 1024
                assert info.blob_bytes % 16 == 0 and 0 < info.blob_bytes <= pkg._lib.lib.rtn_png_stream_blob_bound(len(v))
                assert info.workspace_bytes >= 3 * h * (1 + w * c)
    rc2, info2, _, _ = inspect(pkg, data, with_blob=False)
    assert rc2 == 0 and (info2.width, info2.blob_bytes, info2.workspace_bytes) == (info.width, info.blob_bytes, info.workspace_bytes)


def test_segment_knob_sets_the_segment_count(pkg, crops, monkeypatch):
    data = pillow_png(crops[1])
    zbytes = sum(len(b) for k, b in R.parse_chunks(data) if k == b"IDAT")
    for value, seg in (("256", 256), ("1024", 1024), ("1", 256), ("", 16384), ("1048576", 1 << 20)):
        monkeypatch.setenv("RTN_PNG_SEGMENT", value)
        assert inspect(pkg, data)[1].chunks == (zbytes - 6 + seg - 1) // seg
    monkeypatch.delenv("RTN_PNG_SEGMENT")
    assert inspect(pkg, data)[1].chunks == (zbytes - 6 + 16383) // 16384


def test_layout_files_go_to_the_chunked_decoder_first(pkg, crops):
    """Both inspectors accept a file of the chunked layout (it is an ordinary PNG too); the dispatch order gives it to the first."""
    PIO = sys.modules[pkg.__name__ + ".model.page_io"] if pkg.__name__ + ".model.page_io" in sys.modules else \
        __import__("importlib").import_module(pkg.__name__ + ".model.page_io")
    data = R.build_file(crops[0])
    assert [f.name for f in PIO._FORMATS] == ["jpeg", "png", "png_stream"]
    assert PIO._FORMATS[1].inspect is pkg._lib.lib.rtn_png_inspect and PIO._FORMATS[2].inspect is pkg._lib.lib.rtn_png_stream_inspect
    assert PIO.png_inspect(data)[0] is not None and PIO.png_stream_inspect(data)[0] is not None
    plain = pillow_png(crops[0])
    assert PIO.png_inspect(plain)[0] is None and PIO.png_stream_inspect(plain)[0] is not None
    took = [next(f.name for f in PIO._FORMATS if PIO._inspect(f, d)[0] is not None) for d in (data, plain)]
    assert took == ["png", "png_stream"]


def test_refuses_what_only_pillow_reads(pkg, crops):
    page = crops[0]
    w, h, c = dims(page)
    rgb = Image.fromarray(page[:, :, ::-1])
    raw = R.filter_rows(page, "minsum")
    z = zlib.compress(raw)
    good = S.assemble(w, h, c, z)
    assert inspect(pkg, good)[0] == 0
    refused = {
        "16-bit": pillow_png(Image.fromarray((page[:, :, 0].astype(np.uint16) * 257))),
        "palette": pillow_png(rgb.convert("P")),
        "rgba": pillow_png(rgb.convert("RGBA")),
        "interlace": R.SIGNATURE + S.ihdr(w, h, c, interlace=1) + R._chunk(b"IDAT", z) + R._chunk(b"IEND", b""),
        "tRNS": S.assemble(w, h, c, z, before=[(b"tRNS", b"\x00\x01\x00\x02\x00\x03")]),
        "critical": S.assemble(w, h, c, z, before=[(b"ABCD", b"x")]),
        "unknown ancillary": S.assemble(w, h, c, z, before=[(b"abCd", b"x")]),
        "bKGD": S.assemble(w, h, c, z, before=[(b"bKGD", b"\x00\x01\x00\x02\x00\x03")]),
        "IDAT after another chunk": S.assemble(w, h, c, z, cuts=[10], between=(b"tEXt", b"k\x00v")),
        "bytes after IEND": good + b"\x00",
        "no IDAT": R.SIGNATURE + S.ihdr(w, h, c) + R._chunk(b"IEND", b""),
        "zlib header": S.assemble(w, h, c, b"\x78\x02" + z[2:]),
        "preset dictionary": S.assemble(w, h, c, b"\x78\x20" + z[2:]),
        "no signature": b"\x88" + good[1:],
        "IHDR CRC": good[:30] + bytes([good[30] ^ 1]) + good[31:],
    }
    bad = bytearray(S.assemble(w, h, c, z, after=[(b"tEXt", b"Comment\x00hello")]))
    bad[bad.index(b"hello")] ^= 1                                        # an ancillary chunk with a stale CRC
    refused["ancillary CRC"] = bytes(bad)
    for name, data in refused.items():
        rc, info, why, _ = inspect(pkg, data)
        assert rc == -1 and why and info.blob_bytes == 0, name
    with Image.open(io.BytesIO(refused["interlace"])) as im:
        assert im.info.get("interlace") == 1


def test_refuses_every_truncation(pkg, crops):
    data = pillow_png(crops[0], dpi=(72, 72))
    assert inspect(pkg, data)[0] == 0
    cuts, pos = set(), 8
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        cuts.update((pos, pos + 4, pos + 8, pos + 8 + n))
        pos += 12 + n
    assert pos == len(data) and len(cuts) >= 12        # four chunks, their edges
    rng = np.random.RandomState(6)
    cuts.update(int(v) for v in rng.randint(0, len(data), 50))
    for cut in sorted(cuts):
        part = data[:cut]
        rc, _, why, _ = inspect(pkg, part)
        assert rc == -1 and why, cut


def test_blob_capacity_is_respected(pkg, crops):
    data = pillow_png(crops[1])
    rc, info, why, _ = inspect(pkg, data)
    assert rc == 0, why
    need = info.blob_bytes
    rc, _, why, blob = inspect(pkg, data, capacity=need - 1, guard=64)
    assert rc == -1 and "capacity" in why
    assert (blob == 0xa5).all()                                           # nothing written at all, so nothing past the capacity
    rc, _, _, blob = inspect(pkg, data, capacity=need, guard=64)
    assert rc == 0 and (blob[need:] == 0xa5).all() and not (blob[:need] == 0xa5).all()


# ---- the CPU twin of the device's inflate ---------------------------------------------------------------------------------------------------
def test_inflate_host_equals_zlib_on_every_stream_shape(pkg, streams):
    """No case may be left out: the chain has no "could not split" outcome for a valid stream."""
    assert len(streams) == 18
    for name, w, h, c, raw, d in streams:
        assert zlib.decompressobj(-15).decompress(d) == raw
        data = S.assemble(w, h, c, S.zwrap(d, raw), cuts=S.every(len(d) + 6, 8192))
        for seg in SEGMENTS:
            st, got, intact = twin(pkg, data, seg, len(raw))
            assert st == 0 and intact, (name, seg, st)
            assert got == raw, (name, seg)


def test_inflate_host_on_mutated_and_truncated_streams(pkg, streams):
    """2,000 copies with 1 .. 3 bytes changed, or cut short: status 0 exactly when zlib gives the original bytes with nothing left
    over, and never a write outside out[0:want]."""
    rng = np.random.RandomState(7)
    picked = [s for s in streams if s[0] in ("gray-l6m1", "gray-l1m1", "gray-flushes", "gray-fixed", "page-l6m2", "gray-stored",
                                             "page-rle", "gray-huffman")]
    assert len(picked) == 8
    accepted = refused = 0
    for i in range(2000):
        name, w, h, c, raw, d = picked[i % len(picked)]
        m = bytearray(d)
        if i % 4 == 3:
            m = m[:rng.randint(1, len(m) + 1)]
        else:
            for at in rng.randint(0, len(m), rng.randint(1, 4)):
                m[at] = (m[at] + 1 + rng.randint(0, 255)) % 256
        m = bytes(m)
        zo = zlib.decompressobj(-15)
        try:
            ok = zo.decompress(m) == raw and zo.eof and zo.unused_data == b""
        except zlib.error:
            ok = False
        data = S.assemble(w, h, c, S.zwrap(m, raw))
        st, got, intact = twin(pkg, data, SEGMENTS[rng.randint(0, 4)], len(raw))
        assert intact, (i, name)
        if ok:
            assert st == 0 and got == raw, (i, name, st)
            accepted += 1
        else:
            assert st != 0 and got == b"\xa5" * len(raw), (i, name, st)
            refused += 1
    assert refused >= 1500 and accepted >= 1                                # the full-length "cut" is the valid stream


def test_inflate_host_status_bits(pkg, crops):
    gray = crops[1]
    w, h, c = dims(gray)
    raw = R.filter_rows(gray, "minsum")
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 1)
    d = co.compress(raw) + co.flush()
    PI_ADLER, PI_CRC, PI_LEFT, PI_LENGTH = 256, 512, 2048, 4096
    assert twin(pkg, S.assemble(w, h, c, S.zwrap(d, raw, zlib.adler32(raw) ^ 1)), 1024, len(raw))[0] == PI_ADLER
    assert twin(pkg, S.assemble(w, h, c, S.zwrap(d + b"ab", raw)), 1024, len(raw))[0] & PI_LEFT
    assert twin(pkg, S.assemble(w, h + 1, c, S.zwrap(d, raw)), 1024, len(raw) + 1 + w)[0] & PI_LENGTH
    assert twin(pkg, S.assemble(w, h - 1, c, S.zwrap(d, raw)), 1024, len(raw) - 1 - w)[0] != 0
    data = bytearray(S.assemble(w, h, c, S.zwrap(d, raw), cuts=[5000]))
    data[data.index(b"IEND") - 8] ^= 0x40                                 # the last IDAT's stored CRC
    assert twin(pkg, bytes(data), 1024, len(raw))[0] == PI_CRC


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_cabi_surface(pkg, crops):
    L = pkg._lib
    sz, i, p = C.c_size_t, C.c_int, C.c_void_p
    want = {
        "rtn_png_stream_blob_bound": (sz, [sz]),
        "rtn_png_stream_inspect": (i, [p, p, sz, C.POINTER(L.PngInfo), p, sz]),
        "rtn_png_stream_decode_workspace_bytes": (sz, [i, p, p]),
        "rtn_png_stream_decode": (i, [p, i, p, p, p, p, p, p, sz]),
        "rtn_png_stream_inflate_host": (i, [p, sz, p, sz, C.POINTER(C.c_int32)]),
    }
    lib = C.CDLL(pkg.LIB_PATH)
    for name, (res, args) in want.items():
        assert hasattr(lib, name), name
        assert L.SIGNATURES[name] == (res, args), name
        # the chunked counterpart has the same signature
        other = {"rtn_png_stream_inspect": "rtn_png_inspect", "rtn_png_stream_decode_workspace_bytes": "rtn_png_decode_workspace_bytes",
                 "rtn_png_stream_decode": "rtn_png_decode"}.get(name)
        if other:
            assert L.SIGNATURES[other] == (res, args)
    header = open(os.path.join(ROOT, "include", "rtn.h")).read()
    for name in want:
        assert name + "(" in header
    assert L.lib.rtn_png_stream_blob_bound(1000) == L.png_blob_bound(1000)
    data = pillow_png(crops[0])
    info = L.PngInfo()
    assert L.lib.rtn_png_stream_inspect(None, data, len(data), None, None, 0) == -1
    assert L.lib.rtn_png_stream_inspect(None, None, 10, C.byref(info), None, 0) == -1
    assert L.lib.rtn_png_stream_inspect(None, data, 0, C.byref(info), None, 0) == -1
    offs = np.zeros(1, np.int64)
    rc, info, _, blob = inspect(pkg, data)
    assert L.lib.rtn_png_stream_decode_workspace_bytes(0, blob.ctypes.data, offs.ctypes.data) == 0
    assert L.lib.rtn_png_stream_decode_workspace_bytes(1, None, offs.ctypes.data) == 0
    assert L.lib.rtn_png_stream_decode_workspace_bytes(1, blob.ctypes.data, None) == 0
    assert L.lib.rtn_png_stream_decode_workspace_bytes(1, blob.ctypes.data, offs.ctypes.data) == info.workspace_bytes
    junk = np.zeros(256, np.uint8)
    assert L.lib.rtn_png_stream_decode_workspace_bytes(1, junk.ctypes.data, offs.ctypes.data) == 0
    assert L.lib.rtn_png_stream_decode(None, 1, None, None, None, None, None, None, 0) == -1
    st = C.c_int32(0)
    out = np.zeros(16, np.uint8)
    assert L.lib.rtn_png_stream_inflate_host(None, 0, out.ctypes.data, 16, C.byref(st)) == -1
    assert L.lib.rtn_png_stream_inflate_host(blob.ctypes.data, 0, None, 16, C.byref(st)) == -1
    assert L.lib.rtn_png_stream_inflate_host(blob.ctypes.data, 0, out.ctypes.data, 16, None) == -1
    assert L.lib.rtn_png_stream_inflate_host(junk.ctypes.data, 0, out.ctypes.data, 16, C.byref(st)) == -1
    assert L.lib.rtn_png_stream_inflate_host(blob.ctypes.data, 0, out.ctypes.data, 16, C.byref(st)) == -1       # want is not the page's
    assert L.lib.rtn_png_stream_inflate_host(blob.ctypes.data, 100, out.ctypes.data, 16, C.byref(st)) == -1


# ---- the same host code as a program of its own -------------------------------------------------------------------------------------------------
def test_stand_alone_fuzz_program(streams, crops, tmp_path):
    """tools/png_stream_fuzz.cpp is the program the sanitizer runs use (its header has the -fsanitize command line).  Here it is
    built without a sanitizer: its context still aborts on any position outside the range it was given."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "png_stream_fuzz"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "retinanet-for-table-detection_amd", "csrc"),
                           os.path.join(ROOT, "tools", "png_stream_fuzz.cpp"), "-o", str(exe)])
    files = []
    for name, w, h, c, raw, d in streams:
        if name.startswith("gray"):
            f = tmp_path / (name + ".png")
            f.write_bytes(S.assemble(w, h, c, S.zwrap(d, raw), cuts=S.every(len(d) + 6, 8192)))
            files.append(str(f))
    f = tmp_path / "pillow.png"
    f.write_bytes(pillow_png(crops[0], dpi=(72, 72)))
    files.append(str(f))
    run = subprocess.run([str(exe), "40"] + files, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "mutated or cut blobs 400" in run.stdout.splitlines()[-1]
