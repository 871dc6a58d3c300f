"""GPU: the data-generator row through the C-ABI against oracle/ref_generator.py.
rtn_warp_affine_u8 is integer work after two double products: bit-exact.  A whole CSVGenerator batch: targets bit-exact, the
resized canvas within float32 rounding of the oracle's bicubic (1e-5, as for rtn_resize_cubic alone)."""
import ctypes as C
import importlib
import os
import random

import numpy as np
import pytest
import torch

from oracle import ref_generator as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_KW = dict(min_rotation=-0.1, max_rotation=0.1, min_translation=(-0.1, -0.1), max_translation=(0.1, 0.1), min_shear=-0.1,
                max_shear=0.1, min_scaling=(0.9, 0.9), max_scaling=(1.1, 1.1), flip_x_chance=0.5, flip_y_chance=0.5)


@pytest.fixture(scope="module")
def CG():
    return importlib.import_module("retinanet-for-table-detection_amd.csv_generator")


@pytest.fixture(scope="module")
def T():
    return importlib.import_module("retinanet-for-table-detection_amd.model.transform")


def device_warp(pkg, handle, img, matrix, interp, border, cval):
    src = torch.as_tensor(img).cuda()
    dst = torch.empty_like(src)
    H, W = img.shape[:2]
    Cc = img.shape[2] if img.ndim == 3 else 1
    inv = np.ascontiguousarray(G.invert_affine(matrix))
    cv = np.array([cval, 0, 0, 0], np.uint8)
    handle.check(pkg.lib.rtn_warp_affine_u8(handle.raw, src.data_ptr(), H, W, Cc, inv.ctypes.data_as(C.c_void_p), interp, border,
                                            cv.ctypes.data_as(C.c_void_p), dst.data_ptr()))
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def check_warp_bit_exact(pkg, handle, rng, H, W, interp, border):
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    prng = np.random.RandomState(3)
    mats = [G.adjust_for_image(G.random_transform(prng, **TRAIN_KW), H, W) for _ in range(4)]
    mats.append(np.eye(3))
    mats.append(G.adjust_for_image(G.random_transform(prng, min_rotation=1.0, max_rotation=2.0, min_scaling=(0.3, 0.4), max_scaling=(0.5, 0.6)), H, W))
    mats.append(np.array([[1, 0, 400.0], [0, 1, -300.0], [0, 0, 1]]))            # everything off the page
    for m in mats:
        want = G.warp_affine_u8(img, m, interp, border, cval=77)
        got = device_warp(pkg, handle, img, m, interp, border, 77)
        assert np.array_equal(got, want), "%dx%d: warp differs on %d bytes" % (H, W, int((got != want).sum()))
    gray = img[..., 0].copy()
    assert np.array_equal(device_warp(pkg, handle, gray, mats[0], interp, border, 5), G.warp_affine_u8(gray, mats[0], interp, border, cval=5))


@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("border", [0, 1, 2, 3])
def test_warp_affine_bit_exact(pkg, handle, interp, border):
    rng = np.random.RandomState(10 * interp + border)
    check_warp_bit_exact(pkg, handle, rng, 211, 173, interp, border)           # 173 * 3 % 4 != 0: every store is per byte
    # W * 3 % 4 == 0: full 64-pixel blocks leave as packed dwords (dword_rows).  172 and 196: packed blocks, then a partial last
    # block that takes the per-byte path; 64: one packed block and nothing else; 211, 9 and 6 rows: the last 4-row block of the
    # grid is partial, so the packed store's own row guard decides
    for H, W in ((211, 172), (9, 64), (6, 196)):
        assert W * 3 % 4 == 0 and H % 4 != 0
        check_warp_bit_exact(pkg, handle, np.random.RandomState(1000 * H + 10 * W + 10 * interp + border), H, W, interp, border)


def test_warp_affine_rejects_bad_arguments(pkg, handle):
    x = torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    m = np.array([1, 0, 0, 0, 1, 0], np.float64)
    f = pkg.lib.rtn_warp_affine_u8
    p = m.ctypes.data_as(C.c_void_p)
    assert f(handle.raw, x.data_ptr(), 8, 8, 3, p, 2, 1, None, y.data_ptr()) == -1      # cubic is not implemented
    assert b"interpolation" in pkg.lib.rtn_last_error(handle.raw)
    assert f(handle.raw, x.data_ptr(), 8, 8, 3, p, 1, 4, None, y.data_ptr()) == -1
    assert f(handle.raw, x.data_ptr(), 8, 8, 5, p, 1, 1, None, y.data_ptr()) == -1
    assert f(handle.raw, x.data_ptr(), 8, 8, 3, p, 1, 1, None, x.data_ptr()) == -1      # in place
    bad = np.array([1, 0, np.nan, 0, 1, 0], np.float64)
    assert f(handle.raw, x.data_ptr(), 8, 8, 3, bad.ctypes.data_as(C.c_void_p), 1, 1, None, y.data_ptr()) == -1
    assert f(handle.raw, x.data_ptr(), 8, 8, 3, p, 1, 1, None, y.data_ptr()) == 0


def test_apply_transform_surface(T):
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, (90, 120, 3)).astype(np.uint8)
    gen = T.random_transform_generator(prng=np.random.RandomState(9), **TRAIN_KW)
    for fill, mode in (("nearest", 1), ("constant", 0), ("reflect", 2), ("wrap", 3)):
        params = T.TransformParameters(fill_mode=fill, cval=31)
        m = T.adjust_transform_for_image(next(gen), img, params.relative_translation)
        got = T.apply_transform(m, img, params)
        assert isinstance(got, np.ndarray) and np.array_equal(got, G.warp_affine_u8(img, m, 1, mode, cval=31))
        dev = T.apply_transform(m, torch.as_tensor(img).cuda(), params)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)
    with pytest.raises(ValueError):
        T.apply_transform(np.eye(3), img.astype(np.float32), T.TransformParameters())


def make_dataset(tmp_path, n=5, seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    d = tmp_path / "pages"
    d.mkdir()
    rows = ["image_id,xmin,ymin,xmax,ymax,label"]
    pages = {}
    for i in range(n):
        h, w = int(rng.randint(300, 420)), int(rng.randint(240, 330))
        # smooth heavy-tailed pages like the distance maps, in B,G,R order once read back
        base = np.clip(rng.exponential(12.0, (h // 8 + 2, w // 8 + 2, 3)) * 6, 0, 255)
        page = np.kron(base, np.ones((8, 8, 1)))[:h, :w].astype(np.uint8)
        name = "page_%02d.png" % i
        Image.fromarray(page[:, :, ::-1]).save(str(d / name))
        pages[name] = page
        for _ in range(int(rng.randint(1, 4))):
            bw, bh = rng.uniform(60, 200), rng.uniform(50, 200)
            x1, y1 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
            rows.append("%s,%.2f,%.2f,%.2f,%.2f,table" % (name, x1, y1, x1 + bw, y1 + bh))
    rows.append("%s,10,10,5,50,table" % name)              # an invalid box the filter must drop (x2 < x1)
    csvf = tmp_path / "trainV2.csv"
    csvf.write_text("\n".join(rows) + "\n")
    return str(csvf), str(d), pages


def oracle_batch(gen, group, pages, transforms, min_side, max_side):
    names = [gen.image_data[i].name for i in group]
    boxes = [gen.image_data[i].boxes for i in group]
    labels = [np.zeros(len(b)) for b in boxes]
    return G.compute_input_output([pages[n] for n in names], boxes, labels, 1, transforms=transforms, min_side=min_side, max_side=max_side)


@pytest.mark.parametrize("augment", [False, True])
def test_csv_generator_batch_matches_oracle(tmp_path, CG, T, augment):
    csvf, d, pages = make_dataset(tmp_path)
    random.seed(1)
    kw = dict(batch_size=2, group_method="none", shuffle_groups=False, image_min_side=224, image_max_side=288, dtype=torch.float32)
    if augment:
        kw.update(transform_generator=T.random_transform_generator(prng=np.random.RandomState(21), **TRAIN_KW),
                  transform_parameters=T.TransformParameters())
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gen = CG.CSVGenerator(csvf, d, {"table": 0}, **kw)
        assert gen.size() == 5 and len(gen) == 3 and gen.groups[2] == [4, 0] and gen.num_classes() == 1
        assert gen.name_to_label("table") == 0 and gen.label_to_name(0) == "table" and gen.has_name("table") and gen.has_label(0)
        assert np.array_equal(gen.load_image(1), pages["page_01.png"])
        prng = np.random.RandomState(21)
        for gi in range(len(gen)):
            inputs, (reg, lab) = gen[gi]
            tfs = [G.random_transform(prng, **TRAIN_KW) for _ in gen.groups[gi]] if augment else None
            want_in, want_reg, want_lab, want_boxes = oracle_batch(gen, gen.groups[gi], pages, tfs, 224, 288)
            assert inputs.is_cuda and inputs.dtype == torch.float32 and tuple(inputs.shape) == want_in.shape
            assert np.abs(inputs.cpu().numpy() - want_in).max() <= 1e-5
            for a, b in zip(gen.last_annotations, want_boxes):
                assert np.array_equal(a["bboxes"], b)
            assert np.array_equal(reg.cpu().numpy(), want_reg) and np.array_equal(lab.cpu().numpy(), want_lab)
            assert (want_reg[..., 4] == 1).sum() > 0
    gen.close()


def test_csv_generator_prefetch_and_numpy_output(tmp_path, CG):
    csvf, d, pages = make_dataset(tmp_path, n=6, seed=3)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gen = CG.CSVGenerator(csvf, d, {"table": 0}, batch_size=4, group_method="ratio", shuffle_groups=False, image_min_side=160,
                              image_max_side=224, dtype=torch.bfloat16)
        ratios = [gen.image_aspect_ratio(i) for i in range(gen.size())]
        flat = [i for g in gen.groups for i in g][:6]
        assert all(ratios[a] <= ratios[b] for a, b in zip(flat, flat[1:]))
        direct = [gen[i] for i in range(len(gen))]
        streamed = list(gen.batches(prefetch=2, epochs=2))
        assert len(streamed) == 2 * len(gen)
        for k, (x, (reg, lab)) in enumerate(streamed):
            dx, (dreg, dlab) = direct[k % len(gen)]
            assert x.dtype == torch.bfloat16 and torch.equal(x, dx) and torch.equal(reg, dreg) and torch.equal(lab, dlab)
        # a consumer that stops early does not leave the worker thread behind
        it = gen.batches(prefetch=1, epochs=50)
        next(it)
        it.close()
        gen.output = "numpy"
        x, (reg, lab) = gen[0]
        assert isinstance(x, np.ndarray) and x.dtype == np.float32 and reg.dtype == np.float32 and lab.shape[-1] == 2
        assert np.array_equal(x, direct[0][0].float().cpu().numpy())
    gen.close()
    with pytest.raises(ValueError):
        CG.CSVGenerator(csvf, d, {"table": 0}, preprocess_image=lambda x: x)


def test_trainer_consumes_generator_batches(tmp_path, pkg, CG):
    """Two training steps straight from the generator's device tensors (RetinaNet.py:268-278's fit loop in miniature)."""
    E = importlib.import_module("retinanet-for-table-detection_amd.engine")
    Wt = importlib.import_module("retinanet-for-table-detection_amd.weights")
    Tr = importlib.import_module("retinanet-for-table-detection_amd.trainer")
    csvf, d, _ = make_dataset(tmp_path, n=4, seed=8)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gen = CG.CSVGenerator(csvf, d, {"table": 0}, batch_size=2, group_method="none", shuffle_groups=False, image_min_side=192,
                              image_max_side=256, dtype=torch.bfloat16)
        eng = E.Engine("resnet50", 1, 9, dtype="bf16")
        eng.load_state(Wt.init_state("resnet50", 1, 9, seed=1, randomize_bn=True, cls_bias=-2.0, tame=True))
        tr = Tr.Trainer(eng, lr=1e-4, clipnorm=0.001)
        losses = [tr.train_on_batch(x, reg, lab)[0] for x, (reg, lab) in gen.batches(prefetch=2, epochs=1)]
    assert len(losses) == 2 and all(np.isfinite(losses))
    gen.close()
