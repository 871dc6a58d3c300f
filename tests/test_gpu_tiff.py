"""GPU tests of the TIFF decoder (tfd_strip_kernel and tfd_pixel_kernel of csrc/rtn_tiff.hip) behind decode_tiff_bgr and
read_images_bgr: the grid of tests/test_tiff_host.py (every compression x layout x width x height x strip height, both byte orders,
photometrics, fill orders and predictors) must come back with Pillow's bits, status 0 and no file left to the host; damaged files
must come back through Pillow with a non-zero status, or raise what Pillow raises; the device's status words and pages equal those of
the CPU twin rtn_tiff_decode_host."""
import ctypes as C
import importlib
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_ref as T  # noqa: E402
from test_tiff_host import damaged_files  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def PIO():
    return importlib.import_module("retinanet-for-table-detection_amd.model.page_io")


@pytest.fixture
def device_path(monkeypatch):
    monkeypatch.setenv("RTN_TIFF_MIN", "1")
    monkeypatch.setenv("RTN_TIFF_G4_ONE_STRIP", "1")
    return monkeypatch


def check_all(PIO, files, labels=None):
    """Every file decoded on the device (status 0: none refused, none handed to the host) to Pillow's bits."""
    pages, status = PIO.decode_tiff_bgr(files, return_status=True)
    assert status.count(None) == 0, "%d files were refused by the inspector" % status.count(None)
    assert status == [0] * len(files), [(labels[k] if labels else k, hex(s)) for k, s in enumerate(status) if s][:5]
    for k, (f, g) in enumerate(zip(files, pages)):
        assert g.dtype == torch.uint8 and g.is_cuda and g.is_contiguous()
        assert np.array_equal(g.cpu().numpy(), T.pillow_bgr(f)), labels[k] if labels else k


@pytest.mark.parametrize("compression", list(T.COMPRESSIONS))
def test_grid_on_the_device(PIO, device_path, compression):
    """Fails without the feature (decode_tiff_bgr does not exist; no device decoder takes a TIFF)."""
    corpus = T.corpus(compression)
    check_all(PIO, [d for _, d in corpus], [label for label, _ in corpus])


def test_mixed_call_keeps_the_order(PIO, device_path, tmp_path):
    rng = np.random.RandomState(1)
    rgb = T.random_image(rng, "RGB", 70, 33)
    names, want = [], []
    for k, (ext, kw) in enumerate(((".tif", {"compression": "tiff_lzw"}), (".jpg", {"quality": 90}), (".png", None), (".bmp", {}),
                                   (".tif", {"compression": "group4"}), (".tif", {"compression": "jpeg"}))):
        im = rgb.convert("1") if kw and kw.get("compression") == "group4" else rgb
        path = str(tmp_path / ("page%d%s" % (k, ext)))
        if kw is None:                                                   # the chunked layout of DESIGN §3.4d
            with open(path, "wb") as f:
                f.write(PIO.encode_png_bgr([np.ascontiguousarray(np.asarray(rgb)[:, :, ::-1])])[0])
        else:
            im.save(path, **kw)
        names.append(path)
        want.append(PIO.read_image_bgr(path))
    pages = PIO.read_images_bgr(names)
    for g, w in zip(pages, want):
        assert np.array_equal(g.cpu().numpy(), w)
    datas = [open(p, "rb").read() for p in names]
    _, status = PIO.decode_tiff_bgr(datas, return_status=True)
    assert status == [0, 0, 0, None, 0, None], status                    # BMP and JPEG-in-TIFF stay on the host
    assert PIO.tiff_inspect(datas[5])[0] is None and "JPEG" in PIO.tiff_inspect(datas[5])[1]


def test_damaged_files(PIO, device_path, tmp_path):
    files = damaged_files()
    datas = [d for _, d in files]
    names = []
    for k, d in enumerate(datas):
        names.append(str(tmp_path / ("d%d.tif" % k)))
        with open(names[-1], "wb") as f:
            f.write(d)
    readable = [k for k, d in enumerate(datas) if pillow_or_none_any(d) is not None]
    got, status = PIO.decode_tiff_bgr([datas[k] for k in readable], return_status=True)
    assert None not in status
    for k, g, st in zip(readable, got, status):
        assert np.array_equal(g.cpu().numpy(), T.pillow_bgr(datas[k])), (files[k][0], hex(st))
    assert sum(1 for s in status if s) >= 1
    got = PIO.read_images_bgr([names[k] for k in readable])
    for k, g in zip(readable, got):
        assert np.array_equal(g.cpu().numpy(), T.pillow_bgr(datas[k])), files[k][0]
    broken = [k for k in range(len(datas)) if k not in readable]
    for k in broken[:4]:                                                 # raises what Pillow raises, whatever else is in the call
        with pytest.raises(Exception) as want:
            T.pillow_bgr(datas[k])
        with pytest.raises(type(want.value)):
            PIO.read_images_bgr([names[readable[0]], names[k]])


def pillow_or_none_any(data):
    try:
        return T.pillow_bgr(data)
    except Exception:
        return None


def test_tiff_min_semantics(PIO, monkeypatch):
    rng = np.random.RandomState(2)
    files = [T.pillow_tiff(T.random_image(rng, "L", 20, 10), "tiff_lzw")] * 3
    monkeypatch.setenv("RTN_TIFF_MIN", "0")
    assert PIO.tiff_min() == 0 and PIO.decode_tiff_bgr(files, return_status=True)[1] == [None] * 3
    monkeypatch.setenv("RTN_TIFF_MIN", "4")
    pages, status = PIO.decode_tiff_bgr(files, return_status=True)
    assert status == [None] * 3 and np.array_equal(pages[0].cpu().numpy(), T.pillow_bgr(files[0]))
    monkeypatch.setenv("RTN_TIFF_MIN", "3")
    assert PIO.decode_tiff_bgr(files, return_status=True)[1] == [0] * 3
    monkeypatch.delenv("RTN_TIFF_MIN")
    assert PIO.tiff_min() == PIO.TIFF_MIN_DEFAULT >= 1
    assert PIO.decode_tiff_bgr(files * max(1, PIO.TIFF_MIN_DEFAULT), return_status=True)[1] == [0] * (3 * max(1, PIO.TIFF_MIN_DEFAULT))


def test_sample_sized_pages(PIO, device_path):
    """One 2200 x 1712 page per kind of tools/bench_decode_tiff.py; Group 4 at Pillow's strips and as one strip."""
    kinds = T.sample_tiffs(os.path.join(GOLDEN, "sample_0717_023.jpg"))
    assert len(kinds) == 7
    for f in kinds.values():
        assert Image.open(io.BytesIO(f)).size == (1712, 2200) or Image.open(io.BytesIO(f)).size == (2200, 1712)
    info = PIO.tiff_inspect(kinds["g4_one_strip"])[0]
    assert info.strips == 1 and PIO.tiff_inspect(kinds["g4"])[0].strips > 1
    check_all(PIO, list(kinds.values()), list(kinds))


def test_device_equals_the_host_twin(PIO, device_path, pkg):
    L = pkg._lib
    files = [d for _, d in damaged_files(seed=9, flips=3)] + [d for _, d in T.corpus("group4")[::25]] + [d for _, d in T.corpus("tiff_lzw")[::60]]
    kept = [f for f in files if PIO.tiff_inspect(f)[0] is not None]
    assert len(kept) >= 40
    seen = []

    def host(i):                                                         # the pages the device flags
        seen.append(i)
        return np.zeros((1, 1, 3), np.uint8)

    with PIO._reader(None) as (dev, h):
        pages, status = PIO._decode_datas(kept, host, dev, h, torch.cuda.current_stream(dev))
    for k, f in enumerate(kept):
        info, blob = PIO.tiff_inspect(f)
        out = np.zeros((info.height, info.width, 3), np.uint8)
        st = C.c_int32(-1)
        assert L.lib.rtn_tiff_decode_host(blob.ctypes.data, out.ctypes.data, out.size, C.byref(st)) == 0
        assert status[k] == st.value, (k, hex(status[k]), hex(st.value))
        if st.value == 0:
            assert np.array_equal(pages[k].cpu().numpy(), out), k
        else:
            assert k in seen
    assert any(status) and not all(status)
