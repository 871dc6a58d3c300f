"""CPU tests of rtn_jpeg_inspect, the host half of the device JPEG decoder (csrc/rtn_jpeg.hip): the geometry, sampling, restart
interval and table counts it reports for files Pillow writes, the reasons it gives for files that stay on the host path, and
that truncated or corrupted headers give an error code rather than a crash.  No kernel is launched here."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image


def encode(img, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


def inspect(pkg, data, with_blob=True):
    L = pkg._lib
    info = L.JpegInfo()
    blob = np.zeros(L.jpeg_blob_bound(len(data)), np.uint8)
    rc = L.lib.rtn_jpeg_inspect(None, data, len(data), C.byref(info), blob.ctypes.data if with_blob else None, blob.size)
    return rc, info, L.lib.rtn_last_error(None).decode()


def page(h, w, seed=0):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 3 + yy) % 256, (yy * 2) % 256, ((xx + yy) // 2) % 256], -1)
    return np.clip(img + rng.randint(-8, 9, img.shape), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("subsampling,hv", [(0, (1, 1)), (1, (2, 1)), (2, (2, 2))])
def test_geometry_and_sampling(pkg, subsampling, hv):
    data = encode(page(37, 53), quality=90, subsampling=subsampling)
    rc, info, _ = inspect(pkg, data)
    assert rc == 0
    assert (info.width, info.height, info.components) == (53, 37, 3)
    assert (info.h_samp, info.v_samp) == hv
    assert info.restart_interval == 0
    assert info.huffman_tables == 4 and info.quant_tables == 2
    assert 0 < info.scan_bytes < len(data) and info.blob_bytes % 16 == 0
    assert info.blob_bytes <= pkg._lib.jpeg_blob_bound(len(data))
    # geometry only (no blob): the same answer, blob_bytes an upper bound
    rc2, info2, _ = inspect(pkg, data, with_blob=False)
    assert rc2 == 0 and (info2.width, info2.height, info2.h_samp) == (53, 37, hv[0]) and info2.blob_bytes >= info.blob_bytes


def test_grayscale_and_optimized_tables(pkg):
    rc, info, _ = inspect(pkg, encode(page(20, 9)[..., 0], quality=75))
    assert rc == 0 and (info.width, info.height, info.components) == (9, 20, 1)
    assert info.huffman_tables == 2 and info.quant_tables == 1
    rc, info, _ = inspect(pkg, encode(page(64, 64), quality=95, optimize=True))
    assert rc == 0 and info.components == 3 and info.huffman_tables == 4


def test_restart_intervals(pkg):
    img = page(40, 70)
    rc, info, _ = inspect(pkg, encode(img, quality=90, subsampling=2, restart_marker_blocks=7))
    assert rc == 0 and info.restart_interval == 7
    rc, info, _ = inspect(pkg, encode(img, quality=90, subsampling=2, restart_marker_rows=1))
    mcus_per_row = (70 + 15) // 16
    assert rc == 0 and info.restart_interval == mcus_per_row
    rc, info, _ = inspect(pkg, encode(img[..., 1], quality=90, restart_marker_blocks=1))
    assert rc == 0 and info.restart_interval == 1


def test_rejects_what_stays_on_the_host(pkg):
    img = page(32, 48)
    rc, _, why = inspect(pkg, encode(img, quality=90, progressive=True))
    assert rc == -1 and "progressive" in why
    b = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(b, "JPEG", quality=90)
    rc, _, why = inspect(pkg, b.getvalue())
    assert rc == -1 and "CMYK" in why
    b = io.BytesIO()
    Image.fromarray(img).save(b, "PNG")
    rc, _, why = inspect(pkg, b.getvalue())
    assert rc == -1 and "not a JPEG" in why
    rc, _, why = inspect(pkg, b"")
    assert rc == -1


def test_truncated_and_corrupted_headers_never_crash(pkg):
    data = encode(page(12, 19), quality=80, subsampling=2, restart_marker_blocks=1)
    sos = data.index(b"\xff\xda")
    header_end = sos + 2 + (data[sos + 2] << 8 | data[sos + 3])
    for cut in range(0, header_end + 8):
        rc, _, why = inspect(pkg, data[:cut])
        assert rc == -1 and why, cut
    rng = np.random.RandomState(1)
    for _ in range(400):
        bad = bytearray(data)
        i = int(rng.randint(2, header_end))
        bad[i] = int(rng.randint(0, 256))
        rc, info, why = inspect(pkg, bytes(bad))
        assert rc in (0, -1)
        if rc == 0:
            assert info.blob_bytes <= pkg._lib.jpeg_blob_bound(len(bad))
    # RST markers out of sequence, a scan without EOI
    rst = data.index(b"\xff\xd0", header_end)
    swapped = data[:rst + 1] + b"\xd3" + data[rst + 2:]
    rc, _, why = inspect(pkg, swapped)
    assert rc == -1 and "restart" in why
    rc, _, why = inspect(pkg, data[:-2])
    assert rc == -1 and "EOI" in why


def test_sample_pages_parse(pkg):
    import os
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    data = open(os.path.join(root, "sample_0717_023.jpg"), "rb").read()
    rc, info, _ = inspect(pkg, data)
    assert rc == 0 and (info.width, info.height, info.components, info.h_samp, info.v_samp) == (1712, 2200, 3, 2, 2)
    data = open(os.path.join(root, "sample_0717_023_orig.jpg"), "rb").read()
    rc, info, _ = inspect(pkg, data)
    assert rc == 0 and info.components == 1
