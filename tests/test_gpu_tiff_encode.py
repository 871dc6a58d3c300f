"""GPU tests of the Group 4 TIFF encoder (the tfe_* kernels of csrc/rtn_tiff_enc.hip) behind encode_tiff_bgr,
write_images_bgr(tiff="g4"), deskew_files(tiff="g4") and binarize_files: over the corpus of tests/tiff_encode_ref.py and over one
batch of mixed sizes the device's files equal those of the CPU twin rtn_tiff_encode_host byte for byte (the twin equals Pillow /
libtiff strip for strip: tests/test_tiff_encode_host.py), for CUDA and host inputs and from call to call; decode_tiff_bgr reads the
files back on the device path to the masks; the file writers write what Pillow opens to the expected pixels and leave the other
formats of the same call as they were."""
import importlib
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_encode_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def PIO():
    return importlib.import_module("retinanet-for-table-detection_amd.model.page_io")


@pytest.fixture(scope="module")
def P():
    return importlib.import_module("retinanet-for-table-detection_amd.model.preprocess")


@pytest.fixture(scope="module")
def twin_files(pkg):
    return [R.twin_file(pkg, c) for c in R.corpus()]


def encode(PIO, cases, cuda):
    pages = [torch.from_numpy(c.page).cuda() if cuda else c.page for c in cases]
    return PIO.encode_tiff_bgr(pages, threshold=[c.threshold for c in cases], rows_per_strip=[c.rows_per_strip for c in cases],
                               photometric=[c.photometric for c in cases])


def pillow_pixels(path_or_bytes):
    with Image.open(io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, bytes) else path_or_bytes) as im:
        assert im.mode == "1"
        return np.asarray(im).copy()


@pytest.fixture(scope="module")
def device_files(PIO):
    """The whole corpus in one call, from CUDA tensors."""
    return encode(PIO, R.corpus(), cuda=True)


def test_corpus_equals_the_twin(device_files, twin_files):
    """Fails without the feature (encode_tiff_bgr does not exist)."""
    cases = R.corpus()
    assert len(device_files) == len(cases)
    bad = [c.label for c, d, t in zip(cases, device_files, twin_files) if d != t]
    assert not bad, (len(bad), bad[:5])


def test_host_inputs_and_a_second_call_give_the_same_bytes(PIO, device_files):
    cases = R.corpus()
    assert encode(PIO, cases, cuda=False) == device_files
    assert encode(PIO, cases, cuda=True) == device_files


def test_mixed_batch_equals_the_twin_and_the_single_calls(PIO, pkg):
    cases = R.mixed_batch()
    want = [R.twin_file(pkg, c) for c in cases]
    assert encode(PIO, cases, cuda=True) == want
    assert encode(PIO, cases[::-1], cuda=False) == want[::-1]
    assert [encode(PIO, [c], cuda=True)[0] for c in cases] == want              # a page's file does not depend on its batch
    for c, f in zip(cases, want):
        R.check_parity(f, c)


def test_wave_per_row_variant_gives_the_same_bytes(PIO, pkg, monkeypatch):
    """RTN_TIFF_ENC_WAVE_ROW=1, the variant tools/bench_encode_tiff.py measures, writes the same files."""
    cases = R.mixed_batch()
    monkeypatch.setenv("RTN_TIFF_ENC_WAVE_ROW", "1")
    assert encode(PIO, cases, cuda=True) == [R.twin_file(pkg, c) for c in cases]


def test_settings_as_ints_and_defaults(PIO, pkg):
    c = next(c for c in R.corpus() if c.label.startswith("sample crop rps 64 photometric 0"))
    (f,) = PIO.encode_tiff_bgr([torch.from_numpy(c.page).cuda()])
    assert f == R.twin_file(pkg, c)                                              # the defaults: threshold 128, 64 rows, WhiteIsZero
    bgr = np.ascontiguousarray(np.repeat(c.page[:, :, None], 3, axis=2))
    assert PIO.encode_tiff_bgr([bgr, c.page], threshold=128, rows_per_strip=64, photometric=0) == [f, f]


def test_decode_tiff_bgr_reads_the_files_on_the_device(PIO, device_files, monkeypatch):
    """Every file of at most 64 rows per strip comes back through the device decoder (status 0) as the mask, 0 / 255."""
    monkeypatch.setenv("RTN_TIFF_MIN", "1")
    cases = R.corpus()
    keep = [k for k, c in enumerate(cases) if c.rows_per_strip <= 64]
    pages, status = PIO.decode_tiff_bgr([device_files[k] for k in keep], return_status=True)
    assert status == [0] * len(keep)
    for k, page in zip(keep, pages):
        want = np.where(R.mask_of(cases[k]), 255, 0).astype(np.uint8)
        got = page.cpu().numpy()
        assert got.shape == want.shape + (3,) and (got == want[:, :, None]).all(), cases[k].label


def test_write_images_bgr_g4_next_to_other_formats(PIO, tmp_path):
    """The .tif and .tiff names become Group 4 files Pillow opens to the mask; the .jpg and the .png of the same call are unchanged."""
    rng = np.random.RandomState(5)
    pages = [R.random_page(rng, 150, 70, 0.3, 128, True), R.random_page(rng, 65, 130, 0.5, 128, False),
             rng.randint(0, 256, (40, 50, 3)).astype(np.uint8), rng.randint(0, 256, (33, 21, 3)).astype(np.uint8)]
    names = [str(tmp_path / n) for n in ("a.tif", "b.TIFF", "c.jpg", "d.png")]
    plain = [str(tmp_path / n) for n in ("c0.jpg", "d0.png")]
    PIO.write_images_bgr(plain, pages[2:])
    PIO.write_images_bgr(names, [torch.from_numpy(p).cuda() for p in pages], tiff="g4")
    for n, p in zip(names[:2], pages[:2]):
        data = open(n, "rb").read()
        case = R.Case(n, p, 128, 64, 0)
        assert np.array_equal(pillow_pixels(data), R.mask_of(case)), n
        R.check_parity(data, case)
    for n, w in zip(names[2:], plain):
        assert open(n, "rb").read() == open(w, "rb").read(), n
    PIO.write_images_bgr(names[:1], pages[:1])                                   # tiff="host" is still write_image's file
    with Image.open(names[0]) as im:
        assert im.mode == "RGB"


def test_deskew_files_g4(P, PIO, tmp_path):
    rng = np.random.RandomState(6)
    pages = []
    for h, w in ((120, 160), (90, 100)):                                          # text-like rows of ink on white
        p = np.full((h, w), 255, np.uint8)
        for y in range(10, h - 10, 12):
            p[y:y + 4, 8:w - 8] = np.where(rng.random_sample((4, w - 16)) < 0.8, 20, 235)
        pages.append(p)
    src = []
    for i, p in enumerate(pages):
        src.append(str(tmp_path / ("s%d.png" % i)))
        Image.fromarray(p).save(src[-1], "PNG")
    dst = [str(tmp_path / ("d%d.tif" % i)) for i in range(len(pages))]
    angles = P.deskew_files(src, dst, tiff="g4")
    out, want_angles = P.deskew_images(PIO.read_images_bgr(src))
    assert angles == want_angles
    for d, o in zip(dst, out):
        assert np.array_equal(pillow_pixels(d), R.gray_of(o.cpu().numpy()) >= 128), d


def test_binarize_files(P, PIO, tmp_path):
    crop = np.load(os.path.join(R.GOLDEN, "sample_page_crop.npz"))["orig_gray"]
    pages = [np.ascontiguousarray(crop[:200, :300]), np.ascontiguousarray(crop[100:230, 50:250]), np.ascontiguousarray(crop[300:500, 200:500])]
    src = []
    for i, p in enumerate(pages):
        src.append(str(tmp_path / ("s%d.png" % i)))
        Image.fromarray(p).save(src[-1], "PNG")
    dst = [str(tmp_path / ("d%d.tif" % i)) for i in range(len(pages))]
    P.binarize_files(src, dst)
    for d, p in zip(dst, pages):
        binary = P.preprocess_pages(np.repeat(p[:, :, None], 3, axis=2), return_binary=True)[1]
        data = open(d, "rb").read()
        assert np.array_equal(pillow_pixels(data), binary >= 128), d
        info, _ = PIO.tiff_inspect(data)
        assert info is not None and info.compression == 4 and info.strips == -(-p.shape[0] // 64)
    P.binarize_files(src[:1], [str(tmp_path / "h.tif")], tiff="host")
    with Image.open(str(tmp_path / "h.tif")) as im:
        assert im.mode == "L"
