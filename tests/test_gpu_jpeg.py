"""GPU: the device JPEG decoder (csrc/rtn_jpeg.hip, csv_generator.read_images_bgr) is bit-identical to read_image_bgr (Pillow,
libjpeg-turbo) on files Pillow writes here: every sampling, quality, optimize and restart setting, sizes from 1x1 to a
2200x1712 page, smooth / page / noise / constant content, one batched call and one call per file; files the device does not
take (or flags) give exactly what read_image_bgr gives; and a CSVGenerator over JPEG pages gives the batches it gave with Pillow,
without calling read_image_bgr.  The header layouts and coefficient-built files of tests/jpeg_stream_ref.py (what other writers
produce and Pillow never does) decode the same way, and the device's status word and page equal those of its CPU twin,
rtn_jpeg_decode_host; everything damaged beyond the six files below runs on that twin (tests/test_jpeg_decode_host.py)."""
import ctypes as C
import importlib
import io
import os
import random
import sys
import warnings

import numpy as np
import pytest
import torch
from PIL import Image, features

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_stream_ref as JS  # noqa: E402
from jpeg_corpus import GOLDEN, build_corpus, content, encode  # noqa: E402,F401

if not features.check_feature("libjpeg_turbo"):
    pytest.skip("Pillow is not linked against libjpeg-turbo: the decode the device reproduces is libjpeg-turbo's",
                allow_module_level=True)


@pytest.fixture(scope="module")
def CG():
    return importlib.import_module("retinanet-for-table-detection_amd.csv_generator")


@pytest.fixture(scope="module")
def PIO():
    return importlib.import_module("retinanet-for-table-detection_amd.model.page_io")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """(path, bytes) of every file the bit-exactness tests decode."""
    return build_corpus(tmp_path_factory.mktemp("jpeg"))


def test_device_decode_is_bit_identical(CG, corpus):
    want = [CG.read_image_bgr(p) for p in corpus]
    for p in corpus:                                            # every file is one the device takes
        info, _ = CG.jpeg_inspect(open(p, "rb").read())
        assert info is not None, p
    batched = CG.read_images_bgr(corpus)
    torch.cuda.synchronize()
    for p, w, g in zip(corpus, want, batched):
        assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == w.shape, p
        got = g.cpu().numpy()
        assert np.array_equal(got, w), "%s: %d bytes differ" % (p, int((got != w).sum()))
    for p, w in zip(corpus[:: 7] + corpus[-3:], want[:: 7] + want[-3:]):
        (g,) = CG.read_images_bgr([p])
        assert np.array_equal(g.cpu().numpy(), w), p


def test_device_path_is_taken(CG, PIO, corpus, monkeypatch):
    """With read_image_bgr unavailable the supported files still decode: no page of the corpus needed the host."""
    def no_host(path):
        raise AssertionError("host decode of %s" % path)
    monkeypatch.setattr(PIO, "read_image_bgr", no_host)
    out = CG.read_images_bgr(corpus[-3:] + corpus[:40])
    assert len(out) == 43 and all(t.is_cuda for t in out)


def test_other_files_take_the_host_path(CG, tmp_path):
    rng = np.random.RandomState(5)
    img = content("smooth", 48, 64, rng)
    paths = []

    def put(name, data):
        p = tmp_path / name
        p.write_bytes(data)
        paths.append(str(p))

    put("prog.jpg", encode(img, quality=90, progressive=True))
    b = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(b, "JPEG", quality=90)
    put("cmyk.jpg", b.getvalue())
    b = io.BytesIO()
    Image.fromarray(img).save(b, "PNG")
    put("page.png", b.getvalue())
    good = encode(content("noise", 40, 56, rng), quality=90, subsampling=2)
    sos = good.index(b"\xff\xda")
    scan = sos + 2 + (good[sos + 2] << 8 | good[sos + 3])
    for j in range(6):                                          # a few scan bytes changed, never to or from 0xFF
        bad = bytearray(good)
        for i in rng.randint(scan, len(good) - 2, 3):
            if bad[i] != 0xFF and bad[i - 1] != 0xFF:
                bad[i] = int((bad[i] + 1 + rng.randint(0, 250)) % 255)
        put("corrupt%d.jpg" % j, bytes(bad))
    put("ok.jpg", good)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [CG.read_image_bgr(p) for p in paths]
        got = CG.read_images_bgr(paths)
    for p, w, g in zip(paths, want, got):
        assert np.array_equal(g.cpu().numpy(), w), p
    # a truncated file raises what read_image_bgr raises
    put("trunc.jpg", good[: len(good) // 2])
    with pytest.raises(Exception) as host_exc:
        CG.read_image_bgr(paths[-1])
    with pytest.raises(type(host_exc.value)):
        CG.read_images_bgr(paths[-2:])
    with pytest.raises(FileNotFoundError):
        CG.read_images_bgr([str(tmp_path / "missing.jpg")])


def make_jpeg_dataset(tmp_path, n=5, seed=0):
    """The generator tests' dataset with its pages written as baseline JPEG (q95 4:2:0, what cv2.imwrite writes for a .jpg name)
    under the CSV's .png names (the CSV reader keeps .png ids, like the reference); every file holds JPEG data."""
    rng = np.random.RandomState(seed)
    d = tmp_path / "pages"
    d.mkdir()
    rows = ["image_id,xmin,ymin,xmax,ymax,label"]
    for i in range(n):
        h, w = int(rng.randint(300, 420)), int(rng.randint(240, 330))
        page = content("smooth", h, w, rng)
        name = "page_%02d.png" % i
        (d / name).write_bytes(encode(page[:, :, ::-1], quality=95, subsampling=2))
        for _ in range(int(rng.randint(1, 4))):
            bw, bh = rng.uniform(60, 200), rng.uniform(50, 200)
            x1, y1 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
            rows.append("%s,%.2f,%.2f,%.2f,%.2f,table" % (name, x1, y1, x1 + bw, y1 + bh))
    csvf = tmp_path / "train.csv"
    csvf.write_text("\n".join(rows) + "\n")
    return str(csvf), str(d)


def generator_batches(CG, csvf, d, augment):
    T = importlib.import_module("retinanet-for-table-detection_amd.model.transform")
    random.seed(1)
    kw = dict(batch_size=2, group_method="none", shuffle_groups=False, image_min_side=224, image_max_side=288, dtype=torch.float32)
    if augment:
        kw.update(transform_generator=T.random_transform_generator(prng=np.random.RandomState(21), min_rotation=-0.1, max_rotation=0.1,
                                                                   flip_x_chance=0.5, min_scaling=(0.9, 0.9), max_scaling=(1.1, 1.1)),
                  transform_parameters=T.TransformParameters())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gen = CG.CSVGenerator(csvf, d, {"table": 0}, **kw)
        out = []
        for gi in range(len(gen)):
            x, (reg, lab) = gen[gi]
            out.append((x.cpu().numpy(), reg.cpu().numpy(), lab.cpu().numpy()))
        gen.close()
    return out


@pytest.mark.parametrize("augment", [False, True])
def test_generator_over_jpeg_pages(CG, PIO, tmp_path, monkeypatch, augment):
    csvf, d = make_jpeg_dataset(tmp_path)
    device = generator_batches(CG, csvf, d, augment)
    with monkeypatch.context() as m:                            # the same dataset decoded by read_image_bgr, page by page
        m.setattr(CG.CSVGenerator, "load_image_group", CG.Generator.load_image_group)
        host = generator_batches(CG, csvf, d, augment)
    assert len(device) == len(host) == 3
    for a, b in zip(device, host):
        for x, y in zip(a, b):
            assert x.shape == y.shape and np.array_equal(x, y)

    def no_host(path):
        raise AssertionError("host decode of %s" % path)
    monkeypatch.setattr(PIO, "read_image_bgr", no_host)
    monkeypatch.setattr(CG, "read_image_bgr", no_host)          # CSVGenerator.load_image looks the name up there
    again = generator_batches(CG, csvf, d, augment)
    for a, b in zip(again, host):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


# ---- files Pillow never writes (tests/jpeg_stream_ref.py); everything damaged stays on the CPU twin (tests/test_jpeg_decode_host.py) ----
def noisy_smooth_page(h, w, seed):
    rng = np.random.RandomState(seed)
    img = content("smooth", h, w, rng).astype(np.int64) + rng.randint(-6, 7, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def layout_files():
    """(accepted, refused): {name: bytes} of every header variant of a 45x61 page at every sampling, with and without restarts, and
    of the sizes on both sides of chroma_at's narrow-plane switch; refused holds the variants that must take the host path."""
    accepted, refused = {}, {}
    img = noisy_smooth_page(61, 45, 2)
    for ss in (0, 1, 2, None):
        for rs in (0, 3):
            kw = dict(quality=90)
            if rs:
                kw["restart_marker_blocks"] = rs
            data = encode(img[..., 0], **kw) if ss is None else encode(img, subsampling=ss, **kw)
            for name, v in JS.variants(data).items():
                host = name == "dqt16x40" or (ss is not None and name in JS.REFUSED)
                (refused if host else accepted)["%s-ss%s-rs%d" % (name, ss, rs)] = v
    rng = np.random.RandomState(3)
    for h, w in ((9, 2), (9, 3), (9, 4), (9, 5), (9, 6), (2, 9), (3, 9), (4, 9), (2, 2), (3, 3), (4, 4), (5, 5), (1, 4), (1, 5)):
        page = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        for ss in (1, 2):
            for q in (75, 100):
                accepted["narrow%dx%d-ss%d-q%d" % (h, w, ss, q)] = encode(page, quality=q, subsampling=ss)
    return accepted, refused


def write_all(tmp_path, files):
    paths = []
    for name, data in files.items():
        p = tmp_path / (name + ".jpg")
        p.write_bytes(data)
        paths.append(str(p))
    return paths


def device_only(CG, PIO, monkeypatch, paths):
    """read_images_bgr of files the device must take itself: every one passes the inspector, and read_image_bgr is unavailable, so
    that a silent host fallback cannot pass.  Every page must equal read_image_bgr's."""
    want = [CG.read_image_bgr(p) for p in paths]
    for p in paths:
        info, why = CG.jpeg_inspect(open(p, "rb").read())
        assert info is not None, (p, why)

    def no_host(path):
        raise AssertionError("host decode of %s" % path)
    monkeypatch.setattr(PIO, "read_image_bgr", no_host)
    got = CG.read_images_bgr(paths)
    torch.cuda.synchronize()
    for p, w, g in zip(paths, want, got):
        assert g.is_cuda and tuple(g.shape) == w.shape, p
        g = g.cpu().numpy()
        assert np.array_equal(g, w), "%s: %d bytes differ" % (p, int((g != w).sum()))


def test_layouts_pillow_never_writes(CG, PIO, tmp_path, monkeypatch):
    accepted, _ = layout_files()
    assert len(accepted) == (6 * 13 + 3) + (2 * 19 + 1) + 56      # colour and gray variants (dri-huge without restarts), narrow sizes
    device_only(CG, PIO, monkeypatch, write_all(tmp_path, accepted))


def test_coefficient_built_files(CG, PIO, tmp_path, monkeypatch):
    """Long Huffman codes, ZRL runs, index 63, the largest DC and AC categories, all-zero 250x333 pages."""
    device_only(CG, PIO, monkeypatch, write_all(tmp_path, {name: data for name, (data, w, h) in JS.built().items()}))


def test_refused_layouts_take_the_host_path(CG, tmp_path):
    _, refused = layout_files()
    assert len(refused) == 6 * 3 + 2                             # dqt16x40 everywhere; the two REFUSED names in colour
    paths = write_all(tmp_path, refused)
    for p in paths:
        info, why = CG.jpeg_inspect(open(p, "rb").read())
        assert (info is None) == ("dqt16x40" not in p), (p, why)
        if info is None:
            assert why in JS.REFUSED.values()
    want = [CG.read_image_bgr(p) for p in paths]
    got = CG.read_images_bgr(paths)
    for p, w, g in zip(paths, want, got):
        assert np.array_equal(g.cpu().numpy(), w), p


def test_twin_equals_device(pkg, CG, PIO, corpus, tmp_path):
    """The device's status word and page equal rtn_jpeg_decode_host's at the device's 1,024 threads: corpus files of every sampling
    and size, and two valid files whose 16-bit tables take the IDCT out of its exact range (status 2 on both)."""
    _, refused = layout_files()
    paths = corpus[3:256:32] + corpus[-5:-2:2] + corpus[-2:] + write_all(
        tmp_path, {k: v for k, v in refused.items() if k in ("dqt16x40-ss2-rs3", "dqt16x40-ssNone-rs0")})
    assert len(paths) == 14, len(paths)
    datas = [open(p, "rb").read() for p in paths]

    def no_host(i):
        return np.zeros((1, 1, 3), np.uint8)
    with PIO._reader(None) as (dev, h):
        pages, words = PIO._decode_datas(datas, no_host, dev, h, torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    L = pkg._lib
    for p, data, page, word in zip(paths, datas, pages, words):
        info, blob = CG.jpeg_inspect(data)
        assert info is not None and word is not None, p
        blob = np.ascontiguousarray(blob)
        out = np.zeros((info.height, info.width, 3), np.uint8)
        st = C.c_int32(-9)
        assert L.lib.rtn_jpeg_decode_host(blob.ctypes.data, 1024, out.ctypes.data, out.size, C.byref(st)) == 0, p
        assert st.value == word, (p, st.value, word)
        assert word == (2 if "dqt16x40" in p else 0), (p, word)
        if word == 0:
            assert np.array_equal(page.cpu().numpy(), out), p
