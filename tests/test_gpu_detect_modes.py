"""GPU parity of FilterDetections' other modes (class_specific_filter=False and/or nms=False, model/layers.py:177-264):
rtn_decode_filter_nms_ex / rtn_filter_detections_ex / rtn_gather_detections against the NumPy restatement in
tests/detect_modes_ref.py.  Boxes, scores, labels and indices must be BIT-EXACT."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_numpy as R
from detect_modes_ref import filter_detections_modes, gather_other

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANVAS = (800, 1333)
AGN, NO_NMS = 1, 2
MODES = [0, AGN, NO_NMS, AGN | NO_NMS]


def run_ex(pkg, handle, canvas, reg, cls, flags, thr=0.05, iou=0.5, max_det=300, old=False, refused=False):
    """One rtn_decode_filter_nms_ex (old=True: rtn_decode_filter_nms) call -> boxes, scores, labels, indices (None for old).
    refused=True: the call must fail; -> (the RtnError, the four output arrays as the call left them)."""
    E = importlib.import_module(pkg.__name__ + ".engine")
    cfg, N = E.make_anchor_cfg(canvas)
    B, _, K = cls.shape
    assert reg.shape == (B, N, 4)
    r = torch.as_tensor(reg).to(DEV)
    c = torch.as_tensor(cls).to(DEV)
    wsb = pkg.lib.rtn_detect_workspace_bytes(B, N, K) if old else pkg.lib.rtn_detect_workspace_bytes_ex(B, N, K, flags)
    if refused:
        wsb = max(wsb, pkg.lib.rtn_detect_workspace_bytes_ex(B, N, K, flags | AGN))     # a workspace some mode accepts: not what is refused
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    boxes = torch.full((B, max_det, 4), 7.0, dtype=torch.float32, device=DEV)
    scores = torch.full((B, max_det), 7.0, dtype=torch.float32, device=DEV)
    labels = torch.full((B, max_det), 7, dtype=torch.int32, device=DEV)
    idx = torch.full((B, max_det), 7, dtype=torch.int32, device=DEV)
    if old:
        handle.check(pkg.lib.rtn_decode_filter_nms(handle.raw, C.byref(cfg), B, K, r.data_ptr(), c.data_ptr(), canvas[0], canvas[1], thr,
                                                   iou, max_det, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), ws.data_ptr(),
                                                   wsb))
    else:
        rc = pkg.lib.rtn_decode_filter_nms_ex(handle.raw, C.byref(cfg), B, K, r.data_ptr(), c.data_ptr(), canvas[0], canvas[1],
                                              thr, iou, max_det, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                                              ws.data_ptr(), wsb, flags, idx.data_ptr())
        if refused:
            with pytest.raises(pkg.RtnError) as err:
                handle.check(rc)
            torch.cuda.synchronize()
            return err.value, [boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy(), idx.cpu().numpy()]
        handle.check(rc)
    torch.cuda.synchronize()
    out = [boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy()]
    return out + [None if old else idx.cpu().numpy()]


def restate(canvas, reg, cls, flags, thr=0.05, iou=0.5, max_det=300):
    a32 = R.anchors_f32(canvas + (3,))
    out = []
    for b in range(reg.shape[0]):
        boxes = R.decode_boxes_f32(a32, reg[b], canvas)
        out.append(filter_detections_modes(boxes, cls[b], not (flags & AGN), not (flags & NO_NMS), thr, max_det, iou))
    return [np.stack([o[i] for o in out]) for i in range(4)]


def compare(got, want):
    for name, g, w in zip(("boxes", "scores", "labels", "indices"), got, want):
        assert np.array_equal(g, w), name + " differ"


def synth(canvas, B, K, seed, frac_above, quantise=None, reg_scale=0.5, class_ties=0.0):
    rng = np.random.RandomState(seed)
    N = R.anchors_for_shape(canvas + (3,)).shape[0]
    reg = (rng.normal(size=(B, N, 4)) * reg_scale).astype(np.float32)
    cls = rng.uniform(0.0, 0.05, size=(B, N, K)).astype(np.float32)
    hot = rng.uniform(size=(B, N, K)) < frac_above
    vals = rng.uniform(0.051, 0.99, size=(B, N, K)).astype(np.float32)
    if quantise:
        vals = (np.round(vals * quantise) / quantise).astype(np.float32)      # many exact score ties
    cls[hot] = vals[hot]
    if class_ties and K > 1:                                                   # the max shared by two classes: pins the argmax rule
        tie = rng.uniform(size=(B, N)) < class_ties
        m = cls.max(axis=2)
        c2 = rng.randint(1, K, size=(B, N))
        cls[tie, 0] = m[tie]
        cls[tie, c2[tie]] = m[tie]
    return reg, cls


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("flags", MODES)
def test_modes_bit_exact_with_ties(pkg, handle, K, flags):
    """~2,000 candidates per image at 800x1333 (the bench's regime), quantised scores and cross-class ties of the max."""
    reg, cls = synth(CANVAS, 2, K, 10 + K, 0.01 / K, quantise=64, class_ties=0.02)
    got = run_ex(pkg, handle, CANVAS, reg, cls, flags)
    compare(got, restate(CANVAS, reg, cls, flags))


@pytest.mark.parametrize("flags", MODES)
def test_modes_more_than_one_batch_of_candidates(pkg, handle, flags):
    """Image 0: ~9,000 candidates per list (radix select), image 1: every one of the 200,700 anchors above the threshold."""
    rng = np.random.RandomState(20)
    reg, cls = synth(CANVAS, 2, 3, 21, 0.045, quantise=32, reg_scale=0.3, class_ties=0.05)
    N = cls.shape[1]
    assert N == 200700
    cls[1] = (np.round(rng.uniform(0.3, 0.7, size=(N, 3)) * 32) / 32).astype(np.float32)
    assert (cls[0] > np.float32(0.05)).sum(axis=0).min() > 4096 and np.all(cls[1] > np.float32(0.05))
    compare(run_ex(pkg, handle, CANVAS, reg, cls, flags), restate(CANVAS, reg, cls, flags))


@pytest.mark.parametrize("flags", MODES)
def test_no_candidates_and_max_detections(pkg, handle, flags):
    canvas = (256, 384)
    reg, cls = synth(canvas, 2, 3, 30, 0.0)
    for b, n, c, v in ((1, 1234, 2, 0.7), (1, 77, 1, 0.6), (1, 77, 2, 0.6), (1, 900, 0, 0.65)):
        cls[b, n, c] = v
    bx, sc, lb, ix = run_ex(pkg, handle, canvas, reg, cls, flags)
    assert np.all(bx[0] == -1) and np.all(sc[0] == -1) and np.all(lb[0] == -1) and np.all(ix[0] == -1)
    compare((bx, sc, lb, ix), restate(canvas, reg, cls, flags))
    reg, cls = synth(canvas, 2, 3, 31, 0.05, quantise=16)
    for md in (1, 300):
        compare(run_ex(pkg, handle, canvas, reg, cls, flags, max_det=md), restate(canvas, reg, cls, flags, max_det=md))


@pytest.mark.parametrize("K", [20, 27])
@pytest.mark.parametrize("flags", MODES)
def test_modes_bit_exact_at_many_classes(pkg, handle, K, flags):
    """Twenty and twenty-seven lists per image at 256 x 384 (27 x 300 = 8100: the most the class-specific merge holds), ~1,000
    candidates per image, quantised scores and cross-class ties of the max; every class keeps detections."""
    canvas = (256, 384)
    reg, cls = synth(canvas, 2, K, 50 + K, 0.03 / K, quantise=64, class_ties=0.02)
    got = run_ex(pkg, handle, canvas, reg, cls, flags)
    if not flags & NO_NMS:
        assert set(got[2][got[2] >= 0].tolist()) == set(range(K))
    compare(got, restate(canvas, reg, cls, flags))


def test_class_specific_limit_at_28_classes(pkg, handle):
    """include/rtn.h: class-specific filtering handles classes * max_detections <= 8192, class-agnostic mode has no such limit.
    28 x 300 = 8400: the class-specific modes are refused with RTN_EINVAL and a message that names the limit, before anything is
    written; both class-agnostic modes run and equal the restatement; 28 x 292 = 8176 is accepted again."""
    canvas, K = (256, 384), 28
    reg, cls = synth(canvas, 2, K, 78, 0.03 / K, quantise=64, class_ties=0.02)
    for flags in (0, NO_NMS):
        err, outs = run_ex(pkg, handle, canvas, reg, cls, flags, refused=True)
        assert err.code == -1 and "classes*max_detections > 8192" in str(err), str(err)
        assert all(np.all(o == 7) for o in outs), "a refused call wrote its outputs"
    for flags in (AGN, AGN | NO_NMS):
        compare(run_ex(pkg, handle, canvas, reg, cls, flags), restate(canvas, reg, cls, flags))
    compare(run_ex(pkg, handle, canvas, reg, cls, 0, max_det=292), restate(canvas, reg, cls, 0, max_det=292))


def test_invariants(pkg, handle):
    reg, cls = synth(CANVAS, 2, 3, 40, 0.004, quantise=64, class_ties=0.02)
    # _ex with flags = 0 is the old entry point, and repeatable
    old = run_ex(pkg, handle, CANVAS, reg, cls, 0, old=True)
    ex = run_ex(pkg, handle, CANVAS, reg, cls, 0)
    for a, b in zip(old[:3], ex[:3]):
        assert np.array_equal(a, b)
    a32 = R.anchors_f32(CANVAS + (3,))
    for flags in MODES:
        first = run_ex(pkg, handle, CANVAS, reg, cls, flags)
        again = run_ex(pkg, handle, CANVAS, reg, cls, flags)
        compare(again, first)
        for b in range(2):                               # the indices reproduce the boxes (and, class-specific, the scores)
            ok = first[3][b] >= 0
            assert ok.sum() > 0 and np.all(first[3][b][~ok] == -1)
            dec = R.decode_boxes_f32(a32, reg[b], CANVAS)
            assert np.array_equal(dec[first[3][b][ok]], first[0][b][ok])
            assert np.array_equal(cls[b][first[3][b][ok], first[2][b][ok]], first[1][b][ok])
    # class-agnostic with K = 1 is the class-specific path, bit for bit
    for nms_flag in (0, NO_NMS):
        compare(run_ex(pkg, handle, CANVAS, reg, cls[:, :, :1].copy(), AGN | nms_flag),
                run_ex(pkg, handle, CANVAS, reg, cls[:, :, :1].copy(), nms_flag))


def test_ex_rejects_unknown_flags(pkg, handle):
    E = importlib.import_module(pkg.__name__ + ".engine")
    cfg, N = E.make_anchor_cfg((128, 192))
    r = torch.zeros(1, N, 4, device=DEV)
    c = torch.zeros(1, N, 1, device=DEV)
    wsb = pkg.lib.rtn_detect_workspace_bytes(1, N, 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    out = torch.empty(1, 300, 4, device=DEV)
    lab = torch.empty(1, 300, dtype=torch.int32, device=DEV)
    for bad in (4, 1 << 20):
        with pytest.raises(pkg.RtnError):
            handle.check(pkg.lib.rtn_decode_filter_nms_ex(handle.raw, C.byref(cfg), 1, 1, r.data_ptr(), c.data_ptr(), 128, 192, 0.05,
                                                          0.5, 300, out.data_ptr(), out.data_ptr(), lab.data_ptr(), ws.data_ptr(),
                                                          wsb, bad, None))


@pytest.fixture(scope="module")
def M():
    """`from model import ...` as RetinaNet.py does, with the package directory on sys.path."""
    sys.path.insert(0, os.path.join(ROOT, "retinanet-for-table-detection_amd"))
    for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
        del sys.modules[k]
    mods = {n: importlib.import_module("model." + n) for n in ("layers", "utils", "defineModel")}
    yield type("Mods", (), mods)
    sys.path.pop(0)


def test_bbox_model_modes_end_to_end(M):
    """retinanet_bbox(applyNms=False / class_specific_filter=False).predict_on_batch = the restatement on the training model's raw
    outputs; predict_generator with two batches in flight = one batch at a time."""
    D = M.defineModel
    model = D.ResNetBackbone("resnet50").retinanet(3, num_anchors=None, modifier=None)
    # classification bias 0 instead of the prior's: scores near 0.5, every anchor a candidate in every class
    model._state = D.Wt.init_state("resnet50", 3, 9, seed=0, randomize_bn=True, cls_bias=0.0, tame=True)
    x = np.random.RandomState(60).randint(0, 256, (2, 128, 192, 3)).astype(np.uint8)
    reg, cls = model.predict_on_batch(x)
    assert (cls > np.float32(0.05)).mean() > 0.5
    a32 = R.anchors_f32((128, 192, 3))
    for kw, (csf, nms) in (({"applyNms": False}, (True, False)), ({"class_specific_filter": False}, (False, True)),
                           ({"nms": False, "class_specific_filter": False}, (False, False))):
        bbox = D.retinanet_bbox(model=model, **kw)
        got = bbox.predict_on_batch(x)
        for b in range(2):
            want = filter_detections_modes(R.decode_boxes_f32(a32, reg[b], (128, 192)), cls[b], csf, nms)
            for g, w in zip(got, want[:3]):
                assert np.array_equal(g[b], w)
    conv = M.utils.convert_model(model, nms=False, class_specific_filter=False)
    for g, w in zip(conv.predict_on_batch(x), got):
        assert np.array_equal(g, w)
    rng = np.random.RandomState(61)
    batches = [rng.randint(0, 256, (2, 128 + 32 * (i % 2), 160, 3)).astype(np.uint8) for i in range(4)]
    want = [conv.predict_on_batch(b) for b in batches]
    got = conv.predict_generator(batches, in_flight=2)
    for k in range(3):
        assert np.array_equal(got[k], np.concatenate([w[k] for w in want], axis=0))


@pytest.mark.parametrize("csf,nms", [(True, True), (False, False), (False, True)])
def test_filter_detections_layer_with_other(M, csf, nms):
    rng = np.random.RandomState(70)
    B, N, K = 2, 3000, 3
    xy = rng.uniform(0, 500, size=(B, N, 2)).astype(np.float32)
    boxes = np.concatenate([xy, xy + rng.uniform(5, 80, size=(B, N, 2)).astype(np.float32)], axis=2)
    cls = rng.uniform(0, 0.05, size=(B, N, K)).astype(np.float32)
    hot = rng.uniform(size=(B, N, K)) < 0.02                                  # ~180 candidates: fewer than 300 kept, -1 padding
    cls[hot] = rng.uniform(0.051, 0.99, size=int(hot.sum())).astype(np.float32)
    o_f = rng.normal(size=(B, N, 2, 3)).astype(np.float32)
    o_i = rng.randint(-5, 1000, size=(B, N)).astype(np.int32)
    layer = M.layers.FilterDetections(nms=nms, class_specific_filter=csf)
    out = layer([boxes, cls, o_f, o_i])
    assert len(out) == 5 and out[3].dtype == np.float32 and out[4].dtype == np.int32
    assert out[3].shape == (B, 300, 2, 3) and out[4].shape == (B, 300)
    for b in range(B):
        want = filter_detections_modes(boxes[b], cls[b], csf, nms)
        assert np.any(want[3] == -1)
        for g, w in zip(out[:3], want[:3]):
            assert np.array_equal(g[b], w)
        assert np.array_equal(out[3][b], gather_other(o_f[b], want[3]))
        assert np.array_equal(out[4][b], gather_other(o_i[b], want[3]))
    one = M.layers.filter_detections(boxes[1], cls[1], other=[o_i[1]], class_specific_filter=csf, nms=nms)
    for g, w in zip(one, [o[1] for o in (out[0], out[1], out[2], out[4])]):
        assert np.array_equal(g, w)
    with pytest.raises(TypeError):
        layer([boxes, cls, o_f.astype(np.float64)])
