"""GPU: the device evaluator (csrc/rtn_eval.hip via model/eval.py DeviceEvaluator / evaluate_generator, model/customCallbacks.py
Evaluate) against the host evaluator model/eval.py evaluate_detections (t = 0.5) and the NumPy restatement tests/eval_multi_ref.py
(every threshold).  Hit masks and counts exact, AP within 1e-12."""
import ctypes as C
import importlib
import warnings

import numpy as np
import pytest
import torch

import eval_multi_ref as M
from test_eval_device import random_detect_set

pytestmark = pytest.mark.gpu
PKG = "retinanet-for-table-detection_amd"


@pytest.fixture(scope="module")
def E():
    return importlib.import_module(PKG + ".model.eval")


def run_device(E, images, anns, scales, K, thresholds, batches=1, **kw):
    ev = E.DeviceEvaluator(K, thresholds, **kw)
    B = len(images)
    cuts = np.linspace(0, B, batches + 1).astype(int)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi == lo:
            continue
        boxes = torch.as_tensor(np.stack([images[i][0] for i in range(lo, hi)])).cuda()
        scores = torch.as_tensor(np.stack([images[i][1] for i in range(lo, hi)])).cuda()
        labels = torch.as_tensor(np.stack([images[i][2] for i in range(lo, hi)])).cuda()
        ev.add(boxes, scores, labels, scales[lo:hi], anns[lo:hi])
    return ev.result(), ev.slot_view()


def check(E, got, slots, want, want_slots, K, thresholds, host=None):
    score, mask, cls = slots
    for i, (c, s, m) in enumerate(want_slots):
        assert np.array_equal(cls[i], c), i
        assert np.array_equal(mask[i], m), i
        assert np.array_equal(score[i][c >= 0], s[c >= 0]), i
    for t in thresholds:
        for c in range(K):
            g, w = got["average_precision"][t][c], want["average_precision"][t][c]
            assert g[1] == w[1]
            assert g[0] == pytest.approx(w[0], abs=1e-12), (t, c)
            gf, wf = got["f1"][t][c], want["f1"][t][c]
            assert gf[:3] == wf[:3], (t, c)
            assert gf[3:] == pytest.approx(wf[3:], abs=1e-15)
        assert got["mean_ap"][t] == pytest.approx(want["mean_ap"][t], abs=1e-12)
    assert got["weighted_f1"] == pytest.approx(want["weighted_f1"], abs=1e-12)
    if host is not None:                                  # model/eval.py's host path at t = 0.5
        for c in range(K):
            assert got["average_precision"][0.5][c][1] == host[c][1]
            assert got["average_precision"][0.5][c][0] == pytest.approx(host[c][0], abs=1e-12)


def host_eval(E, images, anns, scales, K):
    dets = [E.split_detections(b, s, l, K, sc) for (b, s, l), sc in zip(images, scales)]
    a = [[np.asarray(x)[np.asarray(x)[:, 4] == c, :4] for c in range(K)] for x in anns]
    return E.evaluate_detections(dets, a, num_classes=K, iou_threshold=0.5)


def edge_case_pages():
    """Hand-made pages (scale 1): ties, IoU exactly at float32(t) and between float32(t) and t, two detections on one
    annotation, an argmax on a taken annotation, a page without annotations, a page without detections, 64 annotations,
    300 kept rows, a label outside the classes."""
    D = 300
    pages, anns = [], []

    def page(rows, ann):
        b = np.full((D, 4), -1, np.float32)
        s = np.full(D, -1, np.float32)
        lab = np.full(D, -1, np.int32)
        for i, (box, sc, l) in enumerate(rows):
            b[i], s[i], lab[i] = box, sc, l
        pages.append((b, s, lab))
        anns.append(np.asarray(ann, np.float64).reshape(-1, 5))
    # IoU 0.7 (double) -> float32(0.7) < 0.7: a hit at 0.7 only in the float32 compare; 0.55 = 220/400 -> float32(0.55) > 0.55
    page([([0, 0, 10, 7], .9, 0), ([0, 0, 20, 11], .9, 1), ([100, 100, 110, 110], .9, 0)],
         [[0, 0, 10, 10, 0], [0, 0, 20, 20, 1], [300, 300, 310, 310, 0]])
    # a double IoU (55 / 100.000001) just below 0.55 that rounds to float32(0.55): a hit in the float32 compare only
    page([([0, 0, 10, 5.5], .8, 0)], [[0, 0, 10, 10.0000001, 0]])
    # two detections on one annotation (ties in score), and an argmax that points at the annotation taken before
    page([([0, 0, 10, 10], .7, 0), ([0, 0, 10, 10], .7, 0), ([0, 0, 10, 9], .6, 0), ([2, 0, 12, 10], .5, 0)],
         [[0, 0, 10, 10, 0], [3, 0, 13, 10, 0]])
    page([([0, 0, 10, 10], .9, 0), ([5, 5, 10, 10], .3, 2)], [])                     # no annotations
    page([], [[0, 0, 10, 10, 0], [5, 5, 50, 50, 2]])                                  # no detections
    rng = np.random.default_rng(5)
    g = rng.uniform(0, 900, (64, 2))
    a64 = np.concatenate([g, g + rng.uniform(10, 100, (64, 2)), rng.integers(0, 3, (64, 1))], 1)
    src = a64[rng.integers(0, 64, D)]
    d = src[:, :4] + rng.normal(0, 3, (D, 4))
    d[:, 2:] = np.maximum(d[:, 2:], d[:, :2] + 1)
    sc = np.sort(np.round(rng.uniform(0.06, 1, D), 2).astype(np.float32))[::-1]
    lab = src[:, 4].astype(np.int32)
    lab[7] = 5                                                                         # outside the 3 classes: kept, then dropped
    page([(d[i], sc[i], lab[i]) for i in range(D)], a64)                              # 300 kept rows, 64 annotations
    return pages, anns


def test_device_evaluator_edge_cases(E):
    K = 3
    thresholds = (0.5, 0.55, 0.7, 0.75, 0.3, 0.9, 1.0, 0.05, 0.6, 0.65, 0.8, 0.85, 0.95, 0.45, 0.4, 0.35)     # T = 16
    pages, anns = edge_case_pages()
    scales = [1.0] * len(pages)
    want, want_slots = M.evaluate(pages, anns, scales, K, thresholds)
    got, slots = run_device(E, pages, anns, scales, K, thresholds)
    check(E, got, slots, want, want_slots, K, thresholds, host_eval(E, pages, anns, scales, K))
    mask = slots[1]
    assert mask[0][0] & (1 << 2) and not mask[0][0] & (1 << 3)          # IoU float32(0.7): hit at 0.7, miss at 0.75
    assert mask[0][1] & (1 << 1)                                          # IoU float32(0.55) >= float32(0.55)
    assert mask[1][0] & (1 << 1)
    assert list(mask[2][:4] & 1) == [1, 0, 0, 1]


@pytest.mark.parametrize("K", [1, 3, 20])
def test_device_evaluator_random_sets(E, K):
    rng = np.random.default_rng(40 + K)
    n = {1: 600, 3: 2000, 20: 300}[K]                     # twenty classes: 300 pages, every class's lists far shorter
    images, anns, scales = random_detect_set(rng, n, K, n_max=120)
    thresholds = M.COCO
    want, want_slots = M.evaluate(images, anns, scales, K, thresholds)
    got, slots = run_device(E, images, anns, scales, K, thresholds)
    check(E, got, slots, want, want_slots, K, thresholds)
    assert got["map_50_95"] == pytest.approx(want["map_50_95"], abs=1e-12)
    # several batches give the same result as one, bit for bit; and the same again (no float atomics)
    got3, slots3 = run_device(E, images, anns, scales, K, thresholds, batches=7)
    assert got3 == got
    for a, b in zip(slots3, slots):
        assert np.array_equal(a, b)
    # host evaluate_detections at t = 0.5 on a subset
    sub = slice(0, 150)
    got_s, _ = run_device(E, images[sub], anns[sub], scales[sub], K, (0.5,))
    host = host_eval(E, images[sub], anns[sub], scales[sub], K)
    for c in range(K):
        assert got_s["average_precision"][0.5][c][1] == host[c][1]
        assert got_s["average_precision"][0.5][c][0] == pytest.approx(host[c][0], abs=1e-12)


def test_eval_rejects_bad_arguments(pkg, handle):
    L = pkg._lib
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = d.data_ptr()

    def match(T=1, thr=0.5, score=0.05, D=300, gt=64, md=300):
        th = (C.c_double * max(T, 1))(*([thr] * max(T, 1)))
        return L.lib.rtn_eval_match(handle.raw, 1, D, p, p, p, p, p, p, p, gt, 1, T, th, score, md, p, p)
    for kw, text in [(dict(T=0), b"IoU thresholds"), (dict(T=17), b"IoU thresholds"), (dict(thr=0.0), b"(0, 1]"),
                     (dict(thr=1.5), b"(0, 1]"), (dict(score=-0.5), b"score_threshold"), (dict(D=301), b"detections per image"),
                     (dict(gt=65), b"annotations per image"), (dict(md=0), b"max_detections")]:
        assert match(**kw) == -1, kw
        assert text in L.lib.rtn_last_error(handle.raw), (kw, L.lib.rtn_last_error(handle.raw))
    assert L.lib.rtn_eval_finalize(handle.raw, 1, 300, p, p, 1, 1, 0.5, p, p, 16) == -3      # workspace too small


# ---------------------------------------------------------------------------------------------------------- end to end
def make_pages(tmp_path, n, seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    d = tmp_path / "pages"
    d.mkdir(exist_ok=True)
    rows = []
    for i in range(n):
        h, w = int(rng.randint(200, 260)), int(rng.randint(160, 220))
        base = np.clip(rng.exponential(12.0, (h // 8 + 2, w // 8 + 2, 3)) * 6, 0, 255)
        page = np.kron(base, np.ones((8, 8, 1)))[:h, :w].astype(np.uint8)
        name = "page_%02d.png" % i
        Image.fromarray(page[:, :, ::-1]).save(str(d / name))
        for _ in range(int(rng.randint(1, 4))):
            bw, bh = rng.uniform(40, 150), rng.uniform(30, 150)
            x1, y1 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
            rows.append("%s,%.2f,%.2f,%.2f,%.2f,table" % (name, x1, y1, x1 + bw, y1 + bh))
    csvf = tmp_path / "val.csv"
    csvf.write_text("\n".join(rows) + "\n")
    return str(csvf), str(d)


def generator(csvf, d, batch_size):
    CG = importlib.import_module(PKG + ".csv_generator")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return CG.CSVGenerator(csvf, d, {"table": 0}, batch_size=batch_size, group_method="none", shuffle_groups=False,
                               image_min_side=160, image_max_side=224)


def seeded_model(seed=2):
    DM = importlib.import_module(PKG + ".model.defineModel")
    Wt = importlib.import_module(PKG + ".weights")
    m = DM.Model("resnet50", 1, 9)
    m._state = Wt.init_state("resnet50", 1, 9, seed=seed, randomize_bn=True, cls_bias=0.0, tame=True)
    return m, DM.retinanet_bbox(model=m)


def test_evaluate_generator_matches_host_evaluate(tmp_path, E):
    csvf, d = make_pages(tmp_path, 5, seed=1)
    _, infer = seeded_model()
    thresholds = (0.5, 0.3)
    g1 = generator(csvf, d, 1)
    images, anns, scales = [], [], []
    for group in g1.groups:
        canvas, sc, an = E._generator_batch(g1, group)
        images.append(canvas[0].float().cpu().numpy())
        scales += sc
        anns += [np.concatenate([a["bboxes"], np.asarray(a["labels"], np.float64)[:, None]], 1) for a in an]
    got = E.evaluate_generator(infer, g1, iou_thresholds=thresholds, in_flight=1)
    for t in thresholds:
        host = E.evaluate(infer, images, anns, scales=scales, num_classes=1, iou_threshold=t)
        assert got["average_precision"][t][0][1] == host[0][1] > 0
        assert got["average_precision"][t][0][0] == pytest.approx(host[0][0], abs=1e-12)
    assert got["f1"][0.3][0][0] + got["f1"][0.3][0][1] > 0               # the seeded weights do produce detections
    assert got["average_precision"][0.3][0][0] > 0.0
    g2 = generator(csvf, d, 2)
    a = E.evaluate_generator(infer, g2, iou_thresholds=thresholds, in_flight=1)
    b = E.evaluate_generator(infer, g2, iou_thresholds=thresholds, in_flight=2)
    assert a == b
    g1.close(); g2.close()


def test_fit_generator_with_evaluate_callback(tmp_path, E):
    CB = importlib.import_module(PKG + ".model.customCallbacks")
    DM = importlib.import_module(PKG + ".model.defineModel")
    csvf, d = make_pages(tmp_path, 4, seed=3)
    m, infer = seeded_model(seed=4)
    m.compile(loss={'regression': None, 'classification': None}, optimizer=DM.Adam(lr=1e-4, clipnorm=0.001))
    train = generator(csvf, d, 2)
    val = generator(csvf, d, 2)
    thresholds = (0.3, 0.5)
    seen = []

    class After:
        def on_epoch_end(self, epoch, logs=None):
            seen.append(dict(logs))
    m.fit_generator(train, steps_per_epoch=2, epochs=1, verbose=0,
                    callbacks=[CB.RedirectModel(CB.Evaluate(val, iou_thresholds=thresholds, verbose=0), infer), After()])
    assert len(seen) == 1 and "mAP" in seen[0] and "weighted_f1" in seen[0]
    fresh = DM.Model("resnet50", 1, 9)
    fresh._state = {k: np.array(v, copy=True) for k, v in m.get_state().items()}
    r = E.evaluate_generator(DM.retinanet_bbox(model=fresh), val, iou_thresholds=thresholds)
    assert seen[0]["mAP"] == r["mAP"]
    assert seen[0]["weighted_f1"] == r["weighted_f1"]
    train.close(); val.close()
