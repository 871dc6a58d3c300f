"""The forward pass at more than five classes, op by op against float64 (the audit of tests/test_gpu_layer_audit.py, unchanged).

The classification output has K * 9 channels behind a sigmoid, stored as f32 into the concatenated [B][anchors][K] tensor.  Up to 48
channels the persistent head-output kernel (generation 6) takes it; from K = 6 on (54 channels) the launch falls to the 256-row
kernels, K = 20 (180) is wider than a 128-column tile and K = 30 (270) needs a second N tile and 384 weight rows.  Bounds are
layer_audit.py's own (SIGMOID_REL included); coverage is every layer exactly once, as in the full-size audit.
Run with -s for the per-op table.

MEASURED on the MI355X at 2 x 146 x 210 (71 layers, none missing, none twice; the classification output always on generation 2):
    bf16 K = 6   128 weight rows   output 0.016 of its bound   worst op 0.996 (conv: the bf16 output rounding)   0.8 s
    bf16 K = 20  256               0.016                        0.996                                             0.5 s
    bf16 K = 30  384               0.017                        0.996                                             0.5 s
    f32  K = 20  256               0.003                        0.187 (conv)                                      0.5 s"""
import pytest

from test_gpu_layer_audit import audit_forward, images, mods

pytestmark = pytest.mark.gpu
CANVAS = (146, 210)
CLS = "pyramid_classification"


@pytest.mark.parametrize("dtype,K", [("bf16", 6), ("bf16", 20), ("bf16", 30), ("f32", 20)])
def test_forward_audit_at_many_classes(pkg, dtype, K):
    E, Wt = mods(pkg)
    state = Wt.init_state("resnet50", K, 9, seed=0, randomize_bn=True, cls_bias=0.0, tame=True)
    eng = E.Engine("resnet50", K, 9, dtype=dtype)
    eng.load_state(state)
    assert eng.K == K
    x = images(2, CANVAS, seed=41 + K)
    au, reg, cls = audit_forward(pkg, eng, state, x, "%s/K%d" % (dtype, K))
    anchors = reg.shape[1]
    assert tuple(reg.shape) == (2, anchors, 4) and tuple(cls.shape) == (2, anchors, K)
    rows = -(-K * 9 // 128) * 128
    assert eng.layout[CLS]["cout"] == K * 9 and eng.layout[CLS]["rows"] == rows and eng.w[CLS][0].shape[0] == rows
    recs = [r for r in au.rows_log if r["name"].startswith(CLS) and not r["name"][len(CLS):].lstrip("_").isdigit()]
    assert len(recs) == 1, [r["name"] for r in au.rows_log if CLS in r["name"]]
    impl = recs[0]["impl"]
    print("%s K=%d: %s ran generation %s on %d weight rows, worst err/bound %.3f" % (dtype, K, recs[0]["name"], impl, rows, recs[0]["worst"]))
    # csrc/rtn_conv.hip: generation 6 needs N <= 48; a grouped 3x3 layer is neither a streaming 1x1 nor a split-K candidate (generation 1),
    # and the shared-halo kernel (3) wants N >= 256 on 256-wide tiles, which the cost model does not pick on a grid this small
    assert impl == 2, impl
    assert float(cls.min()) >= 0.0 and float(cls.max()) <= 1.0 and float(cls.std()) > 0.0
