"""GPU tests of the detection renderer (csrc/rtn_render.hip): the kernel against its CPU twin and against a NumPy page
put through the unchanged draw_box / extract_box / draw_caption (tests/render_cases.py), the files render_detections_device writes
against the host path's, and detect_files against render_detections fed with predict_on_batch."""
import importlib
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import render_cases as K

pytestmark = pytest.mark.gpu
U = K.U


def device_images(pages, plan):
    """One rtn_render_pages launch over uploads of the NumPy pages -> {(page, k): image}; the pages must come back unchanged and
    the bytes between the images untouched."""
    dev = [torch.from_numpy(p.copy()).cuda() for p in pages]
    out, views = U._render_device(plan, dev)
    torch.cuda.synchronize()
    assert all(np.array_equal(d.cpu().numpy(), p) for d, p in zip(dev, pages))
    assert [tuple(v.shape) for v in views] == [(h, w, 3) for _p, _k, h, w, _off in plan["images"]]
    return K.images_of(plan, out.cpu().numpy())


def twin_images(pkg, pages, plan):
    buf = np.zeros(plan["out_bytes"], np.uint8)
    args = U._render_args(plan, [p.ctypes.data for p in pages], plan["masks"].ctypes.data if plan["masks"].size else None, buf.ctypes.data)
    assert pkg._lib.lib.rtn_render_host(*args) == 0
    return K.images_of(plan, buf)


@pytest.mark.parametrize("thickness", K.THICKNESSES)
def test_kernel_equals_the_twin_and_the_numpy_sequence_on_the_grid(pkg, thickness):
    """All pages of the grid, of 29 different sizes, in one launch."""
    pages, kept, want = K.grid_case(thickness)
    plan = U._render_plan([p.shape[:2] for p in pages], kept, K.LABELS, thickness=thickness)
    got = device_images(pages, plan)
    twin = twin_images(pkg, pages, plan)
    assert got.keys() == twin.keys() and all(np.array_equal(got[k], twin[k]) for k in got)
    K.assert_images(got, kept, want, thickness)


def test_kernel_equals_the_twin_and_the_numpy_sequence_on_300_boxes(pkg):
    pages, kept, want = K.many_case()
    plan = U._render_plan([p.shape[:2] for p in pages], kept, K.LABELS)
    got = device_images(pages, plan)
    twin = twin_images(pkg, pages, plan)
    assert all(np.array_equal(got[k], twin[k]) for k in got)
    K.assert_images(got, kept, want, 300)


def detections_of(kept, n=300):
    """(B,300,.) detection arrays at scale 1 that give the kept lists back at any threshold in (0, 0.9]."""
    B = len(kept)
    boxes = np.full((B, n, 4), -1, np.float32)
    scores = np.full((B, n), -1, np.float32)
    labels = np.full((B, n), -1, np.int32)
    for i, dets in enumerate(kept):
        for k, (b, s, l) in enumerate(dets):
            boxes[i, k], scores[i, k], labels[i, k] = b, s, l
    return boxes, scores, labels


def test_return_pages_through_the_python_surface(pkg, tmp_path):
    """render_detections_device(return_pages=True) on pages of different sizes, detections on the device: kept lists and every image."""
    pages, kept, want = K.grid_case(5)
    pick = [0, 8, 13, 22, 26, 27, 28]
    pages, kept, want = [pages[i] for i in pick], [kept[i] for i in pick], [want[i] for i in pick]
    boxes, scores, labels = (torch.from_numpy(a).cuda() for a in detections_of(kept))
    dev = [torch.from_numpy(p.copy()).cuda() for p in pages]
    got_kept, per_page = U.render_detections_device(dev, boxes, scores, labels, [1.0] * len(dev), str(tmp_path),
                                                   ["p%d.png" % i for i in range(len(dev))], return_pages=True)
    for g, w in zip(got_kept, kept):
        assert len(g) == len(w) and all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(g, w))
    for (crops, page), (wcrops, wpage) in zip(per_page, want):
        assert np.array_equal(page.cpu().numpy(), wpage) and len(crops) == len(wcrops)
        for c, w in zip(crops, wcrops):
            assert (c is None) == (w is None) and (c is None or np.array_equal(c.cpu().numpy(), w))
    with pytest.raises(ValueError):
        U.render_detections_device([dev[0][:, :, 0]], boxes[:1], scores[:1], labels[:1], [1.0], str(tmp_path), ["g.png"])
    with pytest.raises(ValueError):
        U.render_detections_device([dev[0].float()], boxes[:1], scores[:1], labels[:1], [1.0], str(tmp_path), ["g.png"])


def read_bgr(path):
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))[:, :, ::-1]


def pillow_q95(bgr):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(b, "JPEG", quality=95, subsampling=2)
    return b.getvalue()


def listing(root):
    return {d: sorted(os.listdir(os.path.join(root, d))) for d in ("detections_cropped", "detections_inImage")}


def check_files(root, names, expected, ext):
    """expected: {file name without extension, relative to root: host-rendered array}.  .png: decoded pixels equal; .jpg: file
    bytes equal Pillow's quality 95, 4:2:0 of the array."""
    for rel, want in expected.items():
        path = os.path.join(root, rel + ext)
        if ext == ".png":
            assert np.array_equal(read_bgr(path), want), rel
        else:
            assert open(path, "rb").read() == pillow_q95(want), rel


def test_files_of_a_batch_equal_the_host_paths(pkg, tmp_path):
    """Three pages: two kept boxes; none (the noDete name); one whose second box lies left of the page, so that its crop rectangle
    is empty (the host path slices NumPy with negative indices there and writes a file, the device path writes none)."""
    shapes = [(90, 140), (50, 70), (80, 120)]
    pages = [K.page_of(H, W, 40 + i) for i, (H, W) in enumerate(shapes)]
    kept = [K.detections_for(90, 140, [(10, 20, 100, 70), (60, 55, 130, 85)]), [],
            K.detections_for(80, 120, [(10, 60, 40, 75), (-8, 10, -2, 30), (20, 30, 60, 50)])]
    boxes, scores, labels = detections_of(kept)
    scores[1, 0] = 0.25
    want = [K.numpy_sequence(p, d) for p, d in zip(pages, kept)]
    expected = {}
    for i, (crops, page) in enumerate(want):
        for k, c in enumerate(crops):
            if c is not None:
                expected["detections_cropped/p%d_%d" % (i, k)] = c
        expected["detections_inImage/p%d" % i] = page
    expected["detections_cropped/p1_noDete_minScore-_0.25"] = pages[1]
    for ext, png in ((".png", "host"), (".png", "device"), (".jpg", "host")):
        names = ["p%d%s" % (i, ext) for i in range(3)]
        host_dir, dev_dir = str(tmp_path / ("host" + ext + png)), str(tmp_path / ("dev" + ext + png))
        for i in range(3):
            U.render_detections(None, pages[i].copy(), boxes[i:i + 1], scores[i:i + 1], labels[i:i + 1], 1.0, host_dir, names[i])
        dev = [torch.from_numpy(p.copy()).cuda() for p in pages]
        got = U.render_detections_device(dev, boxes, scores, labels, [1.0, 1.0, 1.0], dev_dir, names, png=png)
        assert [len(g) for g in got] == [2, 0, 3]
        assert all(np.array_equal(d.cpu().numpy(), p) for d, p in zip(dev, pages))                    # the input pages are only read
        hl, dl = listing(host_dir), listing(dev_dir)
        assert "p2_1" + ext in hl["detections_cropped"]
        hl["detections_cropped"].remove("p2_1" + ext)
        assert dl == hl and sorted(dl["detections_cropped"] + dl["detections_inImage"]) == sorted(os.path.basename(k) + ext for k in expected)
        check_files(dev_dir, names, expected, ext)
        if ext == ".png":                                                                             # the host path's own files hold the same pixels
            for rel in expected:
                assert np.array_equal(read_bgr(os.path.join(host_dir, rel + ext)), expected[rel]), rel


def test_detect_files_equals_render_detections_on_predict_on_batch(pkg, tmp_path):
    D = importlib.import_module("retinanet-for-table-detection_amd.model.defineModel")
    Wt = importlib.import_module("retinanet-for-table-detection_amd.weights")
    P = importlib.import_module("retinanet-for-table-detection_amd.model.preprocess")
    src = []
    for i in range(4):                                           # mid-gray pages with a little noise: the random network's scores stay apart
        img = (128 + np.random.default_rng(9 + i).integers(-10, 11, (120, 160, 3))).astype(np.uint8)
        path = str(tmp_path / ("page_%d.jpg" % i))
        Image.fromarray(img).save(path, "JPEG", quality=90)
        src.append(path)
    m = D.Model("resnet50", 1, 9, dtype="f32")
    m._state = Wt.init_state("resnet50", 1, 9, seed=0, cls_bias=0.0, tame=True)
    pm = D.retinanet_bbox(model=m)
    with pytest.raises(ValueError):
        U.detect_files(m, src, src, str(tmp_path / "no"), min_side=300, max_side=500)

    # the host path: the canvases detect_files builds (batches of two) through predict_on_batch, then render_detections page by page
    # under .png names, whose files hold its arrays
    IO = importlib.import_module("retinanet-for-table-detection_amd.model.page_io")
    pages = [p.cpu().numpy() for p in IO.read_images_bgr(src)]
    parts, scales = [], []
    for j in (0, 2):
        canvas, sc = P.compute_inputs_device(IO.read_images_bgr(src[j:j + 2]), min_side=300, max_side=500, dtype=torch.float32)
        assert tuple(canvas.shape) == (2, 300, 400, 3)
        parts.append(pm.predict_on_batch(canvas.cpu().numpy()))
        scales += list(sc)
    boxes, scores, labels = (np.concatenate([p[k] for p in parts]) for k in range(3))
    thr = float(np.nextafter(scores[:, 3].max(), np.float32(2)))   # the next float32: every page keeps at most 3 detections
    assert 0 < thr < 1 and (scores[:, 0] >= thr).any()
    host_dir, dev_dir = str(tmp_path / "host"), str(tmp_path / "dev")
    want_kept = [U.render_detections(None, pages[i].copy(), boxes[i:i + 1], scores[i:i + 1], labels[i:i + 1], scales[i], host_dir,
                                     "page_%d.png" % i, score_threshold=thr) for i in range(4)]
    assert 1 <= max(len(k) for k in want_kept) <= 3

    got_kept = U.detect_files(pm, src, src, dev_dir, batch_size=2, score_threshold=thr, min_side=300, max_side=500)
    assert len(got_kept) == 4
    for g, w in zip(got_kept, want_kept):
        assert len(g) == len(w) and all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(g, w))
    hl, dl = listing(host_dir), listing(dev_dir)
    assert {d: [os.path.splitext(n)[0] for n in v] for d, v in dl.items()} == {d: [os.path.splitext(n)[0] for n in v] for d, v in hl.items()}
    for d, names in hl.items():
        for n in names:
            jpg = os.path.join(dev_dir, d, os.path.splitext(n)[0] + ".jpg")
            assert open(jpg, "rb").read() == pillow_q95(read_bgr(os.path.join(host_dir, d, n))), (d, n)
