"""CPU tests of rtn_jpeg_decode_host, the CPU twin of the device JPEG decoder (csrc/rtn_jpeg_decode.h): the functions
the three kernels run (the self-synchronising Huffman decode over thread ranges, the segmented scan, the writing pass, the IDCT,
upsampling and colour), run for 1 .. 4096 virtual threads behind a context that aborts on any position outside its bounds.  The
oracle is always Pillow's decode of the same bytes and the comparison is array_equal: the files tests/test_gpu_jpeg.py decodes on
the device, the header layouts and coefficient-built files of tests/jpeg_stream_ref.py that Pillow never writes, sizes on both
sides of the narrow-plane switch of chroma_at, 65500-long strips, and thousands of damaged scans and blobs.  The same host code
is also a stand-alone program for sanitizer builds (tools/jpeg_decode_fuzz.cpp).  No kernel is launched here."""
import ctypes as C
import io
import os
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest
from PIL import Image, features

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_stream_ref as JS  # noqa: E402
from jpeg_corpus import build_corpus, content, encode  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = (1, 2, 7, 64, 1024, 4096)
SAMPLINGS = (0, 1, 2, None)                                           # Pillow's subsampling; None: a gray page
NARROW = ((9, 2), (9, 3), (9, 4), (9, 5), (9, 6), (2, 9), (3, 9), (4, 9), (2, 2), (3, 3), (4, 4), (5, 5), (1, 4), (1, 5))   # H x W

if not features.check_feature("libjpeg_turbo"):
    pytest.skip("Pillow is not linked against libjpeg-turbo: the decode the device reproduces is libjpeg-turbo's",
                allow_module_level=True)


def pillow_bgr(data):
    """read_image_bgr of a file holding these bytes"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with Image.open(io.BytesIO(data)) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def inspect(pkg, data):
    """(info, blob array of exactly blob_bytes) or (None, reason)"""
    L = pkg._lib
    info = L.JpegInfo()
    blob = np.zeros(L.jpeg_blob_bound(len(data)), np.uint8)
    rc = L.lib.rtn_jpeg_inspect(None, data, len(data), C.byref(info), blob.ctypes.data, blob.size)
    if rc != 0:
        return None, L.lib.rtn_last_error(None).decode()
    return info, blob[:info.blob_bytes].copy()


def twin(pkg, blob, shape, threads, guard=64):
    """(return code, status, page) of rtn_jpeg_decode_host; asserts that nothing was written around the page, nor into it unless the
    status is 0."""
    L = pkg._lib
    n = shape[0] * shape[1] * 3
    buf = np.full(n + 2 * guard, 0xa5, np.uint8)
    st = C.c_int32(-9)
    rc = L.lib.rtn_jpeg_decode_host(blob.ctypes.data, threads, buf.ctypes.data + guard, n, C.byref(st))
    assert (buf[:guard] == 0xa5).all() and (buf[guard + n:] == 0xa5).all()
    if rc != 0 or st.value != 0:
        assert (buf == 0xa5).all(), "a refused page was written"
    return rc, st.value, buf[guard:guard + n].reshape(shape[0], shape[1], 3)


def counters(pkg):
    p, b = C.c_int32(-1), C.c_int32(-1)
    pkg._lib.lib.rtn_jpeg_decode_host_counters(C.byref(p), C.byref(b))
    return p.value, b.value


def check_file(pkg, name, data, threads=THREADS):
    """status 0 and Pillow's bits at every thread count"""
    want = pillow_bgr(data)
    info, blob = inspect(pkg, data)
    assert info is not None, (name, blob)
    assert (info.height, info.width) == want.shape[:2], name
    for t in threads:
        rc, st, got = twin(pkg, blob, want.shape, t)
        assert rc == 0 and st == 0, (name, t, rc, st)
        assert np.array_equal(got, want), "%s at %d threads: %d bytes differ" % (name, t, int((got != want).sum()))


def noisy_smooth_page(h, w, seed):
    rng = np.random.RandomState(seed)
    img = content("smooth", h, w, rng).astype(np.int64) + rng.randint(-6, 7, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def pillow_file(img, ss, **kw):
    if ss is None:
        return encode(img[..., 0], **kw)
    return encode(img, subsampling=ss, **kw)


# ---- the helper ---------------------------------------------------------------------------------------------------------------------------
def test_helper_round_trip_and_variants_keep_the_picture():
    img = noisy_smooth_page(61, 45, 1)
    for ss in SAMPLINGS:
        for rs in ({}, {"restart_marker_blocks": 3}):
            data = pillow_file(img, ss, quality=90, **rs)
            assert JS.join(*JS.split(data)) == data
            want = pillow_bgr(data)
            names = set()
            for name, v in JS.variants(data).items():
                names.add(name)
                if name == "dqt16x40" or (ss is not None and name in JS.REFUSED):
                    continue                                            # other tables, or a file that says it holds R,G,B
                assert np.array_equal(pillow_bgr(v), want), (ss, rs, name)
            assert ("dri-huge" in names) == (not rs) and ("gray_samp44" in names) == (ss is None)
            assert len(names) == 16 + (not rs) + 4 * (ss is None)


# ---- files the device takes: Pillow's bits at every thread count ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return build_corpus(tmp_path_factory.mktemp("jpeg"))


def test_corpus_matches_pillow_at_every_thread_count(pkg, corpus):
    assert len(corpus) > 400
    for p in corpus:
        check_file(pkg, p, open(p, "rb").read())


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("ss", SAMPLINGS)
def test_header_variants(pkg, ss, restart):
    """Every layout of tests/jpeg_stream_ref.py on a 45x61 noisy smooth page.  Checked with Pillow 12.2.0 on libjpeg-turbo: every
    variant the inspector accepts gave status 0 and Pillow's bits; a newer Pillow that decodes one of them differently is a finding."""
    data = pillow_file(noisy_smooth_page(61, 45, 2), ss, quality=90, **({"restart_marker_blocks": 3} if restart else {}))
    check_file(pkg, "plain", data)
    seen = 0
    for name, v in JS.variants(data).items():
        if ss is not None and name in JS.REFUSED:
            info, why = inspect(pkg, v)
            assert info is None and why == JS.REFUSED[name], (name, why)
        elif name == "dqt16x40":                                        # tables of 640 .. 10000: the IDCT may leave its exact range
            want = pillow_bgr(v)
            info, blob = inspect(pkg, v)
            assert info is not None, blob
            for t in THREADS:
                rc, st, got = twin(pkg, blob, want.shape, t)
                assert rc == 0 and (st == 2 or (st == 0 and np.array_equal(got, want))), (name, t, rc, st)
        else:
            check_file(pkg, name, v)
        seen += 1
    assert seen == 16 + (not restart) + 4 * (ss is None)


@pytest.mark.parametrize("ss", [1, 2])
def test_both_sides_of_the_narrow_plane_switch(pkg, ss):
    """chroma_at takes libjpeg's box upsampler for a chroma plane of width <= 2 (W <= 4) and the fancy one from width 3 (W = 5, 6)."""
    rng = np.random.RandomState(3)
    for h, w in NARROW:
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        for q in (75, 100):
            data = encode(img, quality=q, subsampling=ss)
            info, _ = inspect(pkg, data)
            assert info is not None and (info.width + 1) // 2 == (w + 1) // 2
            check_file(pkg, "%dx%d q%d" % (h, w, q), data)


@pytest.mark.parametrize("shape", [(1, 65500), (65500, 1)])
def test_longest_strips(pkg, shape):
    rng = np.random.RandomState(4)
    img = np.repeat(rng.randint(0, 256, (-(-shape[0] // 5), -(-shape[1] // 5), 3)), 5, 0).repeat(5, 1)[:shape[0], :shape[1]].astype(np.uint8)
    for ss in (2, None):
        check_file(pkg, "strip %dx%d %s" % (shape + (ss,)), pillow_file(img, ss, quality=90))


def test_coefficient_built_files(pkg):
    built = JS.built()
    assert len(built) == 10
    for name, (data, w, h) in built.items():
        assert pillow_bgr(data).shape == (h, w, 3)
        check_file(pkg, name, data)
    # the periodic streams: at 4:2:0 an MCU is a thread's 32 bits, so every guess is right and the two passes that always run (the
    # guesses, and one that finds no exit state changed) are all; at 4:2:2 (20 bits) and gray (6 bits) most guesses are wrong
    for name, guessed in (("allzero-420", True), ("allzero-422", False), ("allzero-gray", False)):
        info, blob = inspect(pkg, built[name][0])
        assert twin(pkg, blob, (250, 333), 1024)[:2] == (0, 0)
        passes, busy = counters(pkg)
        assert (passes == 2) == guessed and busy > 64, (name, passes, busy)


def test_the_parallel_path_really_runs(pkg):
    """At 1024 threads the 250x333 noise file needs more than one pass to settle (two always run: the guesses, and one that finds no
    exit state changed), and more than half the threads have bits to decode."""
    img = content("noise", 250, 333, np.random.RandomState(5))
    for ss in SAMPLINGS:
        data = pillow_file(img, ss, quality=95)
        info, blob = inspect(pkg, data)
        rc, st, got = twin(pkg, blob, (250, 333), 1024)
        assert rc == 0 and st == 0 and np.array_equal(got, pillow_bgr(data))
        passes, busy = counters(pkg)
        assert passes > 2 and busy > 512, (ss, passes, busy)
        twin(pkg, blob, (250, 333), 1)
        assert counters(pkg) == (2, 1)


def test_arguments(pkg):
    L = pkg._lib
    data = encode(noisy_smooth_page(16, 16, 6), quality=90)
    info, blob = inspect(pkg, data)
    out = np.zeros(16 * 16 * 3 + 8, np.uint8)
    st = C.c_int32(-9)
    for threads, n in ((0, 768), (-1, 768), (65537, 768), (4, 767), (4, 776)):
        assert L.lib.rtn_jpeg_decode_host(blob.ctypes.data, threads, out.ctypes.data, n, C.byref(st)) == -1
        assert L.lib.rtn_last_error(None)
    assert L.lib.rtn_jpeg_decode_host(None, 4, out.ctypes.data, 768, C.byref(st)) == -1
    bad = blob.copy()
    bad[0] ^= 1
    assert L.lib.rtn_jpeg_decode_host(bad.ctypes.data, 4, out.ctypes.data, 768, C.byref(st)) == -1
    assert not out.any() and st.value == -9
    assert L.lib.rtn_jpeg_decode_host(blob.ctypes.data, 5000, out.ctypes.data, 768, C.byref(st)) == 0 and st.value == 0


# ---- damage ---------------------------------------------------------------------------------------------------------------------------------
def small_files():
    img = noisy_smooth_page(40, 56, 7)
    return [pillow_file(img, ss, quality=90, **rs) for ss in SAMPLINGS for rs in ({}, {"restart_marker_blocks": 3})]


def damaged_copy(data, rng):
    """1 .. 3 scan bytes changed (never to or from 0xFF), or the scan cut short (EOI kept)"""
    segs, scan = JS.split(data)
    if rng.randint(0, 4) == 0:
        return JS.join(segs, scan[:int(rng.randint(1, len(scan)))])
    b = bytearray(scan)
    for i in rng.randint(0, len(b), int(rng.randint(1, 4))):
        if b[i] != 0xFF and (i == 0 or b[i - 1] != 0xFF):
            b[i] = int((b[i] + 1 + rng.randint(0, 254)) % 255)
    return JS.join(segs, bytes(b))


def test_damaged_scans_never_give_other_bits(pkg):
    """2,000 damaged copies of eight small files, each at a random thread count: status 0 only with the bits Pillow gives for those
    same bytes; any other status is fine; the bounds context never aborts."""
    rng = np.random.RandomState(8)
    counts = {"refused by the inspector": 0, "status 0": 0, "status 1": 0, "status 2": 0}
    for data in small_files():
        for _ in range(250):
            bad = damaged_copy(data, rng)
            t = int(rng.choice((1, 2, 3, 7, 64, 333, 1024, 4096)))
            info, blob = inspect(pkg, bad)
            if info is None:
                counts["refused by the inspector"] += 1
                continue
            rc, st, got = twin(pkg, blob, (info.height, info.width), t)
            assert rc == 0 and st in (0, 1, 2)
            counts["status %d" % st] += 1
            if st == 0:
                try:
                    want = pillow_bgr(bad)
                except Exception as e:                                  # noqa: BLE001
                    raise AssertionError("status 0 at %d threads for bytes Pillow refuses: %r" % (t, e))
                assert np.array_equal(got, want), "status 0 at %d threads with %d bytes that differ" % (t, int((got != want).sum()))
    print(counts)
    assert sum(counts.values()) == 2000 and counts["status 1"] > 0


def test_damaged_blobs_never_leave_their_bounds(pkg):
    """Bytes changed in the header, the Huffman and quantisation tables and the segment table of an inspected blob: jpeg_blob_ok
    refuses the blob (-1), or the decode returns with some status; the bounds context never aborts."""
    rng = np.random.RandomState(9)
    refused = decoded = 0
    for data in small_files():
        info, blob = inspect(pkg, data)
        shape = (info.height, info.width)
        off_seg, off_data = (int(v) for v in blob[308:316].view(np.int32))     # JHdr.off_seg, JHdr.off_data
        assert off_seg == 512 + 8 * 1440 + 512 and off_seg < off_data < blob.size
        regions = ((0, 512), (512, 512 + 8 * 1440), (off_seg, off_data), (0, off_data))
        for i in range(400):
            bad = blob.copy()
            lo, hi = regions[i % 4]
            for k in rng.randint(lo, hi, int(rng.randint(1, 4))):
                bad[k] = int(rng.randint(0, 256))
            rc, st, _ = twin(pkg, bad, shape, int(rng.choice((1, 7, 1024))))
            assert rc in (0, -1) and (rc == -1 or st in (0, 1, 2))
            refused += rc == -1
            decoded += rc == 0
    assert refused > 800 and decoded > 400, (refused, decoded)


def test_stand_alone_fuzz_program(tmp_path):
    """tools/jpeg_decode_fuzz.cpp is the program the sanitizer runs use (its header has the -fsanitize command line).  Here it is
    built without a sanitizer: its context still aborts on any position outside the range it was given."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "jpeg_decode_fuzz"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "retinanet-for-table-detection_amd", "csrc"),
                           os.path.join(ROOT, "tools", "jpeg_decode_fuzz.cpp"), "-o", str(exe)])
    files = []
    for i, data in enumerate(small_files()):
        f = tmp_path / ("small%d.jpg" % i)
        f.write_bytes(JS.variants(data)["fill"] if i & 1 else data)
        files.append(str(f))
    f = tmp_path / "longcodes.jpg"
    f.write_bytes(JS.built()["longcodes-420"][0])
    files.append(str(f))
    run = subprocess.run([str(exe), "40"] + files, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "mutated or cut scans 360" in run.stdout.splitlines()[-1] and "damaged blobs 360" in run.stdout.splitlines()[-1]
