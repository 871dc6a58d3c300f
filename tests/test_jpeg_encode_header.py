"""CPU tests of the host half of the device JPEG encoder (csrc/rtn_jpeg_enc.hip): rtn_jpeg_encode_header writes exactly the bytes
Pillow writes in front of the entropy-coded data (SOI .. SOS) for every quality, gray and every colour subsampling, and sizes up
to libjpeg's 65500-pixel limit; the invalid arguments give RTN_EINVAL with a reason; rtn_jpeg_encode_bound covers a
high-entropy scan.  No kernel is launched here."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image, features

if not features.check_feature("libjpeg_turbo"):
    pytest.skip("Pillow is not linked against libjpeg-turbo: the encoder reproduces libjpeg-turbo's files",
                allow_module_level=True)

SIZES = [(1, 1), (7, 9), (16, 16), (2200, 1712), (65500, 2), (2, 65500)]          # (H, W)
MODES = [("gray", 1, 0), ("gray", 1, 1), ("gray", 1, 2), ("444", 3, 0), ("422", 3, 1), ("420", 3, 2)]


def pillow_file(h, w, nc, ss, q):
    img = np.zeros((h, w, 3) if nc == 3 else (h, w), np.uint8)
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q, subsampling=ss)
    return b.getvalue()


def head_and_scan(data):
    """(bytes up to and including the SOS segment, the entropy-coded bytes before EOI)"""
    p = 2
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        p += 2 + n
        if m == 0xDA:
            assert data[-2:] == b"\xff\xd9"
            return data[:p], data[p:-2]


def header(pkg, w, h, nc, ss, q, cap=1024):
    L = pkg._lib
    buf = (C.c_uint8 * cap)()
    n = C.c_size_t(0)
    rc = L.lib.rtn_jpeg_encode_header(w, h, nc, ss, q, buf, cap, C.byref(n))
    return rc, bytes(buf[:n.value]), L.lib.rtn_last_error(None).decode()


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("mode", MODES, ids=["%s-s%d" % (m[0], m[2]) for m in MODES])
def test_header_bytes_equal_pillow(pkg, size, mode):
    (h, w), (_, nc, ss) = size, mode
    for q in range(1, 101):
        want, _ = head_and_scan(pillow_file(h, w, nc, ss, q))
        rc, got, err = header(pkg, w, h, nc, ss, q)
        assert rc == 0, err
        assert got == want, "q=%d: header differs from Pillow's (%d vs %d bytes)" % (q, len(got), len(want))


def test_invalid_arguments(pkg):
    cases = [((64, 64, 3, 2, 0), "quality"), ((64, 64, 3, 2, 101), "quality"), ((64, 64, 3, 2, -5), "quality"),
             ((0, 64, 3, 2, 75), "width and height"), ((64, 0, 3, 2, 75), "width and height"),
             ((65501, 64, 3, 2, 75), "width and height"), ((64, 65501, 1, 0, 75), "width and height"),
             ((64, 64, 2, 2, 75), "components"), ((64, 64, 4, 2, 75), "components"), ((64, 64, 0, 2, 75), "components"),
             ((64, 64, 3, 3, 75), "subsampling"), ((64, 64, 3, -1, 75), "subsampling")]
    for args, word in cases:
        rc, got, err = header(pkg, *args)
        assert rc == -1 and got == b"", args
        assert word in err, (args, err)
    rc, _, err = header(pkg, 64, 64, 3, 2, 75, cap=100)                # a buffer too small for the 623 header bytes
    assert rc == -1 and "623" in err
    assert pkg._lib.lib.rtn_jpeg_encode_bound(64, 64, 3, 3) == 0
    assert pkg._lib.lib.rtn_jpeg_encode_bound(65501, 8, 1, 0) == 0


def test_bound_covers_a_high_entropy_scan(pkg):
    img = np.random.RandomState(0).randint(0, 256, (64, 64, 3)).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=100, subsampling=0)
    data = b.getvalue()
    head, scan = head_and_scan(data)
    bound = pkg._lib.lib.rtn_jpeg_encode_bound(64, 64, 3, 0)
    print("64x64 noise q100 4:4:4: file %d bytes, scan %d bytes, bound %d bytes" % (len(data), len(scan), bound))
    assert bound >= len(head) + len(scan) + 2 and bound >= len(data)


def test_workspace_bytes(pkg):
    L = pkg._lib
    arr = lambda *v: np.asarray(v, np.int32)                             # noqa: E731
    w, h, c, s = arr(1712, 1, 65500), arr(2200, 1, 2), arr(3, 1, 3), arr(2, 0, 1)
    one = [L.lib.rtn_jpeg_encode_workspace_bytes(1, w[i:].ctypes.data, h[i:].ctypes.data, c[i:].ctypes.data, s[i:].ctypes.data)
           for i in range(3)]
    assert all(v > 0 and v % 256 == 0 for v in one)
    assert L.lib.rtn_jpeg_encode_workspace_bytes(3, w.ctypes.data, h.ctypes.data, c.ctypes.data, s.ctypes.data) == sum(
        L.lib.rtn_jpeg_encode_workspace_bytes(1, w[i:i + 1].ctypes.data, h[i:i + 1].ctypes.data, c[i:i + 1].ctypes.data,
                                              s[i:i + 1].ctypes.data) for i in range(3))
    assert one[0] >= 88596 * 128                                        # a 2200x1712 4:2:0 page holds 88596 blocks of 64 int16
    bad = arr(3)
    assert L.lib.rtn_jpeg_encode_workspace_bytes(1, w.ctypes.data, h.ctypes.data, bad.ctypes.data, bad.ctypes.data) == 0
