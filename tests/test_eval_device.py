"""CPU side of the device evaluator: the multi-threshold NumPy restatement (tests/eval_multi_ref.py) against oracle/ref_eval.py,
the Evaluate / RedirectModel callbacks inside Model.fit_generator's callback loop (stub model, stub evaluator), and the argument
checks of the C ABI and DeviceEvaluator that need no GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest

from oracle import ref_eval as RE
import eval_multi_ref as M


def random_detect_set(rng, n_img, K, D=300, n_max=40, ties=True):
    """Detect-format arrays (score-descending, -1 padded) with annotations in original coordinates and per-image scales."""
    images, anns, scales = [], [], []
    for _ in range(n_img):
        scale = float(rng.choice([1.0, 0.5, 0.8125, 1.37]))
        m = int(rng.integers(0, 6))
        g = rng.uniform(0, 400, (m, 2))
        a = np.concatenate([g, g + rng.uniform(20, 200, (m, 2)), rng.integers(0, K, (m, 1))], 1)
        n = int(rng.integers(0, n_max))
        src = a[rng.integers(0, m, n), :4] if m else rng.uniform(0, 500, (n, 4))
        d = src + rng.normal(0, 12, (n, 4))
        d[:, 2:] = np.maximum(d[:, 2:], d[:, :2] + 1)
        s = rng.uniform(0.01, 1, n)
        if ties:
            s = np.round(s, 2)
        s = np.sort(s.astype(np.float32))[::-1]
        boxes = np.full((D, 4), -1, np.float32)
        scores = np.full(D, -1, np.float32)
        labels = np.full(D, -1, np.int32)
        boxes[:n] = (d * scale).astype(np.float32)
        scores[:n] = s
        labels[:n] = a[rng.integers(0, m, n), 4] if m and rng.uniform() < 0.8 else rng.integers(0, K, n)
        images.append((boxes, scores, labels))
        anns.append(a)
        scales.append(scale)
    return images, anns, scales


@pytest.mark.parametrize("K", [1, 3])
def test_restatement_matches_oracle_at_half(K):
    rng = np.random.default_rng(11 + K)
    images, anns, scales = random_detect_set(rng, 25, K)
    thresholds = (0.5, 0.75, 0.3)
    got, slots = M.evaluate(images, anns, scales, K, thresholds)
    dets = [M.split(b, s, l, K, sc)[2] for (b, s, l), sc in zip(images, scales)]
    per_cls_anns = [[a[a[:, 4] == c, :4] for c in range(K)] for a in anns]
    for t in thresholds:
        want = RE.evaluate_detections(dets, per_cls_anns, num_classes=K, iou_threshold=t)
        for c in range(K):
            assert got["average_precision"][t][c][1] == want[c][1]
            assert got["average_precision"][t][c][0] == pytest.approx(want[c][0], abs=1e-12)
    # a slot per kept index: its class, score and mask bits only where a detection was kept
    for cls, sc, mk in slots:
        assert np.all(mk[cls < 0] == 0) and np.all(mk < (1 << len(thresholds)))
    f1 = got["f1"][0.5]
    for c in range(K):
        TP, FP, FN, P, R, F = f1[c]
        assert TP + FN == got["average_precision"][0.5][c][1]
        assert F == pytest.approx(2 * P * R / (P + R) if P + R else 0.0)
    assert got["weighted_f1"] == pytest.approx(sum(t * got["f1_micro"][t] for t in thresholds) / sum(thresholds))


def test_restatement_known_answers():
    # one page, two tables; detections: TP(.9), duplicate of the first table (.8), second table at IoU exactly 0.7 (.6)
    boxes = np.full((300, 4), -1, np.float32)
    scores = np.full(300, -1, np.float32)
    labels = np.full(300, -1, np.int32)
    boxes[:3] = [[0, 0, 10, 10], [0, 0, 10, 9.5], [20, 20, 30, 27]]
    scores[:3] = [0.9, 0.8, 0.6]
    labels[:3] = 0
    ann = np.array([[0, 0, 10, 10, 0], [20, 20, 30, 30, 0]], np.float64)
    out, slots = M.evaluate([(boxes, scores, labels)], [ann], [1.0], 1, (0.5, 0.7, 0.75))
    cls, sc, mk = slots[0]
    # IoU 0.7 in double rounds to float32(0.7) < 0.7: a hit at t = 0.7 in the float32 compare
    assert list(mk[:3]) == [0b111, 0, 0b011] and list(cls[:4]) == [0, 0, 0, -1]
    assert out["average_precision"][0.5][0] == (pytest.approx(0.5 + 0.5 * 2 / 3), 2)
    assert out["average_precision"][0.75][0] == (pytest.approx(0.5), 2)
    assert out["f1"][0.5][0][:3] == (2, 1, 0)          # score >= 0.5: all three
    assert out["map_50_95"] is None


class _StubInference:
    bbox = True
    num_classes = 1


def _stub_result(thresholds):
    ap = {t: {0: (0.25 + t / 10, 3)} for t in thresholds}
    f1 = {t: {0: (1, 1, 2, 0.5, 1 / 3, 0.4)} for t in thresholds}
    import importlib as il
    E = il.import_module("retinanet-for-table-detection_amd.model.eval")
    return E.summarize(thresholds, ap, f1)


def test_evaluate_callback_logs_and_order(monkeypatch):
    CB = importlib.import_module("retinanet-for-table-detection_amd.model.customCallbacks")
    DM = importlib.import_module("retinanet-for-table-detection_amd.model.defineModel")
    calls = []

    def stub_evaluate(model, generator, iou_thresholds, **kw):
        calls.append((model, generator, iou_thresholds, kw))
        return _stub_result(iou_thresholds)

    seen = []

    class Checkpoint:                      # ModelCheckpoint(monitor='mAP') stand-in: reads the logs after Evaluate wrote them
        def on_epoch_end(self, epoch, logs=None):
            seen.append(dict(logs))

    infer = _StubInference()
    thresholds = (0.6, 0.7, 0.8, 0.9)
    ev = CB.Evaluate("validation-generator", iou_thresholds=thresholds, verbose=0, evaluate=stub_evaluate)
    redirect = CB.RedirectModel(ev, infer)
    # Model.fit_generator's own callback loop, with training replaced by a stub step
    m = DM.Model.__new__(DM.Model)
    m._compiled, m.stop_training, m.bbox = DM.Adam(), False, False
    m.train_on_batch = lambda x, y: [1.0, 0.5, 0.5]
    hist = m.fit_generator([(None, None)] * 2, steps_per_epoch=2, epochs=2, verbose=0, callbacks=[redirect, Checkpoint()])
    assert hist.history["loss"] == [1.0, 1.0]
    assert len(calls) == 2 and calls[0][0] is infer and calls[0][1] == "validation-generator" and calls[0][2] == thresholds
    want = _stub_result(thresholds)
    assert len(seen) == 2
    for logs in seen:
        assert logs["mAP"] == pytest.approx(want["mAP"]) and logs["weighted_f1"] == pytest.approx(want["weighted_f1"])
        assert logs["loss"] == 1.0
    # weighted F1 = sum t * F1_t / sum t; one threshold: no weighted_f1 key
    assert want["weighted_f1"] == pytest.approx(0.4)
    seen.clear()
    single = CB.Evaluate("g", verbose=0, evaluate=stub_evaluate)
    single.set_model(infer)
    logs = single.on_epoch_end(0, {})
    assert set(logs) == {"mAP"} and logs["mAP"] == pytest.approx(0.25 + 0.05)


def test_summarize_map_50_95():
    E = importlib.import_module("retinanet-for-table-detection_amd.model.eval")
    ap = {t: {0: (1.0 - t, 5), 1: (0.5, 0)} for t in E.COCO_IOU_THRESHOLDS}
    f1 = {t: {0: (1, 0, 4, 1.0, 0.2, 1 / 3), 1: (0, 2, 0, 0.0, 0.0, 0.0)} for t in E.COCO_IOU_THRESHOLDS}
    r = E.summarize(E.COCO_IOU_THRESHOLDS, ap, f1)
    assert r["mean_ap"][0.5] == pytest.approx(0.5)                  # class 1 has no annotations: left out of the mean
    assert r["map_50_95"] == pytest.approx(np.mean([1.0 - t for t in E.COCO_IOU_THRESHOLDS]))
    assert r["f1_micro"][0.5] == pytest.approx(2 * (1 / 3) * 0.2 / (1 / 3 + 0.2))


def test_eval_arguments_without_gpu(pkg):
    L = pkg._lib
    assert L.lib.rtn_eval_workspace_bytes(300, 1, 1) > 0
    assert L.lib.rtn_eval_workspace_bytes(10000 * 300, 1, 16) > 10000 * 300 * 16
    for bad in [(300, 1, 0), (300, 1, 17), (300, 0, 1), (300, 65536, 1), (0, 1, 1), (1 << 29, 1, 1)]:
        assert L.lib.rtn_eval_workspace_bytes(*bad) == 0, bad
    thr = (C.c_double * 1)(0.5)
    assert L.lib.rtn_eval_match(None, 1, 300, None, None, None, None, None, None, None, 64, 1, 1, thr, 0.05, 300, None, None) == -1
    assert L.lib.rtn_eval_finalize(None, 1, 300, None, None, 1, 1, 0.5, None, None, 0) == -1
    E = importlib.import_module("retinanet-for-table-detection_amd.model.eval")
    for kw in [dict(iou_thresholds=()), dict(iou_thresholds=(0.5,) * 17), dict(iou_thresholds=(0.0,)), dict(iou_thresholds=(1.5,)),
               dict(score_threshold=-0.1), dict(max_detections=301), dict(max_detections=0)]:
        with pytest.raises(ValueError):
            E.DeviceEvaluator(1, **kw)
