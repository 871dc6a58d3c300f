"""CPU tests of FilterDetections' two switches (class_specific_filter, nms; model/layers.py:177-369 and
model/defineModel.py:296-353): the mode-aware restatement against the oracle, the workspace sizes of the modes
(host functions), and the Python surface that carries the switches.  No kernel is launched here."""
import importlib
import os
import sys

import numpy as np
import pytest

from oracle import ref_numpy as R
from detect_modes_ref import filter_detections_modes, gather_other

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    """`from model import ...` as RetinaNet.py does, with the package directory on sys.path."""
    sys.path.insert(0, os.path.join(ROOT, "retinanet-for-table-detection_amd"))
    for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
        del sys.modules[k]
    mods = {n: importlib.import_module("model." + n) for n in ("layers", "utils", "defineModel")}
    yield type("Mods", (), mods)
    sys.path.pop(0)


def random_case(seed, N=600, K=3, quantise=None):
    rng = np.random.RandomState(seed)
    xy = rng.uniform(0, 300, size=(N, 2)).astype(np.float32)
    wh = rng.uniform(5, 60, size=(N, 2)).astype(np.float32)
    boxes = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
    cls = rng.uniform(0, 0.3, size=(N, K)).astype(np.float32)
    if quantise:
        cls = (np.round(cls * quantise) / quantise).astype(np.float32)     # exact ties within and across classes
    return boxes, cls


@pytest.mark.parametrize("seed,quantise", [(0, None), (1, 16), (2, 8)])
def test_restatement_default_mode_is_the_oracle(seed, quantise):
    boxes, cls = random_case(seed, quantise=quantise)
    for md in (1, 7, 300):
        got = filter_detections_modes(boxes, cls, True, True, max_detections=md)
        want = R.filter_detections(boxes, cls, max_detections=md)
        for g, w in zip(got[:3], want):
            assert np.array_equal(g, w)
        ok = got[3] >= 0
        assert np.array_equal(boxes[got[3][ok]], got[0][ok])


def test_restatement_modes_relations():
    boxes, cls = random_case(3, quantise=16)
    # K = 1: the class-agnostic modes are the class-specific ones
    for nms in (True, False):
        a = filter_detections_modes(boxes, cls[:, :1], False, nms)
        c = filter_detections_modes(boxes, cls[:, :1], True, nms)
        for x, y in zip(a, c):
            assert np.array_equal(x, y)
    # nms=False: every candidate of the class-specific lists, the top 300 by (score desc, class asc, index asc)
    b, s, l, i = filter_detections_modes(boxes, cls, True, False)
    n, c = np.nonzero(cls > np.float32(0.05))
    order = np.lexsort((n, c, -cls[n, c].astype(np.float64)))[:300]
    assert np.array_equal(i[:len(order)], n[order]) and np.array_equal(l[:len(order)], c[order])
    # class-agnostic: the label is the first maximal class
    cls2 = cls.copy()
    cls2[:, 2] = cls2[:, 1]
    b, s, l, i = filter_detections_modes(boxes, cls2, False, False)
    ok = i >= 0
    assert ok.any() and np.all(l[ok] == np.argmax(cls2[i[ok]], axis=1)) and np.all(l[ok] != 2)
    assert np.array_equal(gather_other(np.arange(len(boxes), dtype=np.int32), i), np.where(ok, i, -1))


def test_workspace_bytes_of_the_modes(pkg):
    lib, L = pkg._lib.lib, pkg._lib
    for (B, N, K) in ((1, 1000, 1), (2, 200700, 1), (8, 200700, 3), (3, 5000, 7)):
        base = lib.rtn_detect_workspace_bytes(B, N, K)
        assert lib.rtn_detect_workspace_bytes_ex(B, N, K, 0) == base
        for f in (L.RTN_DET_CLASS_AGNOSTIC, L.RTN_DET_NO_NMS, L.RTN_DET_CLASS_AGNOSTIC | L.RTN_DET_NO_NMS):
            got = lib.rtn_detect_workspace_bytes_ex(B, N, K, f)
            assert 0 < got <= base
        # NMS-free: no 2 MiB bit matrix per list
        assert lib.rtn_detect_workspace_bytes_ex(B, N, K, L.RTN_DET_NO_NMS) <= base - B * K * 4096 * 4096 // 8
        for bad in (4, 8, 1 << 30, -1):
            assert lib.rtn_detect_workspace_bytes_ex(B, N, K, bad) == 0
    assert lib.rtn_detect_workspace_bytes_ex(0, 10, 1, 0) == 0


def test_retinanet_bbox_carries_the_switches(M):
    D = M.defineModel
    model = D.ResNetBackbone("resnet50").retinanet(2, num_anchors=None, modifier=None)
    m = D.retinanet_bbox(model=model)
    assert (m.nms, m.class_specific_filter) == (True, True)
    m = D.retinanet_bbox(model, applyNms=False)
    assert m.bbox and (m.nms, m.class_specific_filter) == (False, True)
    m = D.retinanet_bbox(model=model, class_specific_filter=False)
    assert (m.nms, m.class_specific_filter) == (True, False)
    m = D.retinanet_bbox(model=model, nms=False, class_specific_filter=False)            # keras-retinanet's spelling
    assert (m.nms, m.class_specific_filter) == (False, False)
    assert D.retinanet_bbox(model=model, nms=True, applyNms=True).nms
    with pytest.raises(ValueError):
        D.retinanet_bbox(model=model, nms=False, applyNms=True)
    with pytest.raises(ValueError):
        D.retinanet_bbox(model=model, nms=True, applyNms=False)
    m = M.utils.convert_model(model, nms=False)
    assert m.bbox and (m.nms, m.class_specific_filter) == (False, True)
    m = M.utils.convert_model(model, class_specific_filter=False)
    assert (m.nms, m.class_specific_filter) == (True, False)


def test_filter_detections_layer_config_and_shapes(M):
    FD = M.layers.FilterDetections
    f = FD(nms=False, class_specific_filter=False, max_detections=100, name="filtered_detections")
    cfg = f.get_config()
    assert cfg["nms"] is False and cfg["class_specific_filter"] is False and cfg["max_detections"] == 100
    g = FD(**cfg)
    assert g.get_config() == cfg
    shapes = [(2, 5000, 4), (2, 5000, 3), (2, 5000), (2, 5000, 7, 2)]
    assert g.compute_output_shape(shapes) == [(2, 100, 4), (2, 100), (2, 100), (2, 100), (2, 100, 7, 2)]
    assert g.compute_output_shape(shapes[:2]) == [(2, 100, 4), (2, 100), (2, 100)]
    assert len(g.compute_mask(shapes)) == 5
