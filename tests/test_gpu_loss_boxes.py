"""GPU: rtn_retina_loss_boxes_fwd (csrc/rtn_loss.hip) - focal + smooth-L1 sums per image straight from the ground-truth boxes.

Main check: image_sums[b] has the BITS of rtn_anchor_targets on the batch followed by rtn_retina_loss_fwd on image b's rows alone
(np.array_equal on the float64 sums).  Against oracle/ref_numpy.py (anchor_targets -> focal_loss / smooth_l1_loss): 2e-5 relative
on the sums - float32 terms against a float64 oracle, the tolerance of tests/test_gpu_kernels.py for the same reason - and exact
counts.  A second launch gives the same bits.  The inputs are checked with the oracle on the CPU first: every batch except the
no-box one holds a positive and an ignored anchor."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANVAS = (160, 224)                   # 6,759 anchors: no multiple of 256, and P7 is a single row of cells
SPECIAL_P = [0.0, 1.0, 1e-9, 1 - 1e-9]   # hit the epsilon clip of K.binary_crossentropy


def engine_mod(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".engine")


def boxes64(rng, canvas):
    h, w = canvas
    bw, bh = rng.uniform(24, 110, 64), rng.uniform(24, 100, 64)
    x1, y1 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
    return np.stack([x1, y1, x1 + bw, y1 + bh], axis=1)


def image(kind, rng, canvas):
    """-> (boxes (G,4) float64 at network scale, the image's own (h, w))."""
    h, w = canvas
    if kind == "empty":
        return np.zeros((0, 4)), (h, w)
    if kind == "boxes64":
        return boxes64(rng, canvas), (h, w)
    if kind == "ties":
        # two identical boxes (the argmax tie goes to the first), a box partly off the image, and an image smaller than the canvas:
        # anchors centred past (hh, ww) are ignored
        hh, ww = int(h * 0.75), int(w * 0.7)
        b = np.array([[16.0, 24.0, 80.0, 88.0], [16.0, 24.0, 80.0, 88.0], [ww - 40.0, hh - 50.0, ww + 30.0, hh + 20.0],
                      [70.5, 10.25, 140.0, 58.0]])
        return b, (hh, ww)
    if kind == "large":                                    # full-size pages: tables of a few hundred pixels
        g = 5
        bw, bh = rng.uniform(120, 700, g), rng.uniform(90, 500, g)
        x1, y1 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
        b = np.stack([x1, y1, x1 + bw, y1 + bh], axis=1)
        return np.concatenate([b, b[:1]]), (h - 37, w - 101)
    raise ValueError(kind)


BATCHES = {"one_boxes64": ["boxes64"], "one_ties": ["ties"], "one_empty": ["empty"], "three": ["boxes64", "ties", "empty"]}


def make_case(kinds, K, canvas, seed):
    rng = np.random.RandomState(seed)
    gts, shapes, labs = [], [], []
    for kind in kinds:
        b, hw = image(kind, rng, canvas)
        gts.append(b)
        shapes.append(hw)
        lab = rng.randint(0, K, len(b))
        if kind == "ties" and K > 1:
            lab[:] = [1, 2, 0, 0]                          # a tie that went to the second box would change the class
        labs.append(lab)
    anchors = R.anchors_for_shape(canvas + (3,))
    wreg, wlab = R.anchor_targets(anchors, shapes, gts, labs, K)
    B, N = len(kinds), anchors.shape[0]
    p = rng.uniform(0.001, 0.999, size=(B, N, K)).astype(np.float32)
    for b in range(B):                                     # saturated probabilities on kept rows: negatives, and positives' own class
        kept = np.nonzero(wlab[b, :, K] != -1)[0]
        p[b, kept[:4], 0] = SPECIAL_P
        pos = np.nonzero(wlab[b, :, K] == 1)[0][:4]
        for j, n in enumerate(pos):
            p[b, n, int(np.argmax(wlab[b, n, :K]))] = SPECIAL_P[j]
    pred = (wreg[..., :4] + rng.normal(scale=0.15, size=(B, N, 4))).astype(np.float32)
    return gts, shapes, labs, wreg, wlab, p, pred


def check_inputs(kinds, wreg, wlab, K):
    """The conditions on the inputs, from the oracle's targets alone."""
    state = wlab[..., K]
    assert np.array_equal(state, wreg[..., 4])
    if any(k != "empty" for k in kinds):
        assert (state == 1).any() and (state == -1).any()
    for b, kind in enumerate(kinds):
        if kind == "empty":
            assert not (state[b] == 1).any() and not wreg[b, :, :4].any()      # (cells centred below the canvas are ignored)
        if kind == "boxes64":
            assert (state[b] == 1).sum() >= 4
        if kind == "ties":
            pos = np.nonzero(state[b] == 1)[0]
            assert len(pos) >= 1
            if K > 1:                                      # some positive anchor belongs to the tied pair: class of the FIRST box
                assert (wlab[b, pos, 1] == 1).any() and not (wlab[b, pos, 2] == 1).any()
            # the smaller image: anchors whose centre is outside it are ignored whatever they overlap
            assert (state[b] == -1).sum() > (state[b] == 1).sum()


def upload_gt(gts, labs, shapes):
    B = len(gts)
    gb = np.zeros((B, 64, 4), np.float64)
    gl = np.zeros((B, 64), np.int32)
    gc = np.zeros((B,), np.int32)
    for i, g in enumerate(gts):
        gb[i, :len(g)], gl[i, :len(g)], gc[i] = g, labs[i], len(g)
    hw = np.asarray(shapes, np.int32).reshape(B, 2)
    return [torch.as_tensor(a).to(DEV) for a in (gb, gl, gc, hw)]


def two_kernel_sums(pkg, handle, cfg, N, K, t, p_d, pred_d, alpha, gamma, sigma):
    """rtn_anchor_targets once, then rtn_retina_loss_fwd per image (rows = N) -> (B,4) float64."""
    B = p_d.shape[0]
    reg = torch.full((B, N, 5), 9.0, dtype=torch.float32, device=DEV)
    lab = torch.full((B, N, K + 1), 9.0, dtype=torch.float32, device=DEV)
    handle.check(pkg.lib.rtn_anchor_targets(handle.raw, C.byref(cfg), B, K, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                            t[3].data_ptr(), 0.4, 0.5, reg.data_ptr(), lab.data_ptr()))
    wsb = pkg.lib.rtn_retina_loss_workspace_bytes(N)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    out = torch.zeros(B, 4, dtype=torch.float64, device=DEV)
    for b in range(B):
        handle.check(pkg.lib.rtn_retina_loss_fwd(handle.raw, N, K, lab[b].data_ptr(), reg[b].data_ptr(), p_d[b].data_ptr(),
                                                 pred_d[b].data_ptr(), alpha, gamma, sigma, out[b].data_ptr(), ws.data_ptr(), wsb))
    torch.cuda.synchronize()
    return out.cpu().numpy(), reg.cpu().numpy(), lab.cpu().numpy()


def boxes_sums(pkg, handle, cfg, N, K, t, p_d, pred_d, alpha, gamma, sigma):
    """rtn_retina_loss_boxes_fwd at row 1 of a (B+2, 4) array -> the B rows; the rows around them stay as they were."""
    B = p_d.shape[0]
    wsb = pkg.lib.rtn_retina_loss_boxes_workspace_bytes(B, N)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    out = torch.full((B + 2, 4), float("nan"), dtype=torch.float64, device=DEV)
    handle.check(pkg.lib.rtn_retina_loss_boxes_fwd(handle.raw, C.byref(cfg), B, K, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                                   t[3].data_ptr(), 0.4, 0.5, p_d.data_ptr(), pred_d.data_ptr(), alpha, gamma, sigma,
                                                   out[1:].data_ptr(), ws.data_ptr(), wsb))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isnan(o[0]).all() and np.isnan(o[-1]).all()
    return o[1:-1]


def run_case(pkg, handle, kinds, K, canvas, gamma, seed):
    alpha, sigma = 0.25, 3.0
    gts, shapes, labs, wreg, wlab, p, pred = make_case(kinds, K, canvas, seed)
    check_inputs(kinds, wreg, wlab, K)
    cfg, N = engine_mod(pkg).make_anchor_cfg(canvas)
    assert N == wreg.shape[1]
    t = upload_gt(gts, labs, shapes)
    p_d, pred_d = torch.as_tensor(p).to(DEV), torch.as_tensor(pred).to(DEV)
    want, reg, lab = two_kernel_sums(pkg, handle, cfg, N, K, t, p_d, pred_d, alpha, gamma, sigma)
    assert np.array_equal(reg, wreg) and np.array_equal(lab, wlab)       # the dense path itself still has the oracle's bits
    got = boxes_sums(pkg, handle, cfg, N, K, t, p_d, pred_d, alpha, gamma, sigma)
    print("loss_boxes %s K=%d gamma=%g\n got  %r\n want %r" % (kinds, K, gamma, got, want))
    assert np.array_equal(got, want)
    for b in range(len(kinds)):
        fc, npos = R.focal_loss(wlab[b:b + 1], p[b:b + 1], alpha=alpha, gamma=gamma)
        rl, nposr = R.smooth_l1_loss(wreg[b:b + 1], pred[b:b + 1], sigma=sigma)
        assert abs(got[b, 0] - fc) <= 2e-5 * abs(fc) and abs(got[b, 1] - rl) <= 2e-5 * abs(rl), (b, got[b], fc, rl)
        assert got[b, 2] == npos and got[b, 3] == nposr
    again = boxes_sums(pkg, handle, cfg, N, K, t, p_d, pred_d, alpha, gamma, sigma)
    assert np.array_equal(again, got)


@pytest.mark.parametrize("gamma", [2.0, 1.5])
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_loss_boxes_bits_of_two_kernel_path(pkg, handle, batch, K, gamma):
    run_case(pkg, handle, BATCHES[batch], K, CANVAS, gamma, seed=7 + K)


def test_loss_boxes_full_size(pkg, handle):
    run_case(pkg, handle, ["large", "large"], 1, (800, 1333), 2.0, seed=3)      # 200,700 anchors per image


def test_loss_boxes_clamps_gt_count(pkg, handle):
    """gt_count outside [0, RTN_MAX_GT] is clamped, as in anchor_targets_kernel: 100 reads the 64 boxes there are, -5 none."""
    K, alpha, gamma, sigma = 1, 0.25, 2.0, 3.0
    gts, shapes, labs, wreg, wlab, p, pred = make_case(["boxes64", "boxes64"], K, CANVAS, seed=21)
    cfg, N = engine_mod(pkg).make_anchor_cfg(CANVAS)
    p_d, pred_d = torch.as_tensor(p).to(DEV), torch.as_tensor(pred).to(DEV)
    t = upload_gt(gts, labs, shapes)
    want = boxes_sums(pkg, handle, cfg, N, K, t, p_d, pred_d, alpha, gamma, sigma)
    t[2] = torch.as_tensor(np.array([100, -5], np.int32)).to(DEV)
    got = boxes_sums(pkg, handle, cfg, N, K, t, p_d, pred_d, alpha, gamma, sigma)
    assert np.array_equal(got[0], want[0])
    t[2] = torch.as_tensor(np.array([64, 0], np.int32)).to(DEV)
    assert np.array_equal(boxes_sums(pkg, handle, cfg, N, K, t, p_d, pred_d, alpha, gamma, sigma), got)
    assert got[1, 1] == 0 and got[1, 2] == 0 and got[1, 0] > 0


def test_loss_boxes_rejects_bad_arguments(pkg, handle):
    L = pkg._lib
    cfg, N = engine_mod(pkg).make_anchor_cfg(CANVAS)
    d = torch.zeros(4096, dtype=torch.float64, device=DEV)
    p = d.data_ptr()
    wsb = L.lib.rtn_retina_loss_boxes_workspace_bytes(1, N)
    assert wsb == ((N + 255) // 256) * 4 * 8 and L.lib.rtn_retina_loss_boxes_workspace_bytes(3, N) == 3 * wsb

    def call(B=1, K=1, cfg_=C.byref(cfg), gt=p, lab=p, cnt=p, hw=p, cls=p, reg=p, out=p, ws=p, nbytes=wsb):
        return L.lib.rtn_retina_loss_boxes_fwd(handle.raw, cfg_, B, K, gt, lab, cnt, hw, 0.4, 0.5, cls, reg, 0.25, 2.0, 3.0, out, ws, nbytes)
    for kw, text in [(dict(B=0), b"B 0"), (dict(B=65536), b"B 65536"), (dict(K=0), b"classes 0"), (dict(gt=None), b"null pointer"),
                     (dict(lab=None), b"null pointer"), (dict(cnt=None), b"null pointer"), (dict(hw=None), b"null pointer"),
                     (dict(cls=None), b"null pointer"), (dict(reg=None), b"null pointer"), (dict(out=None), b"null pointer"),
                     (dict(ws=None), b"null pointer"), (dict(reg=p + 4), b"16-byte aligned"), (dict(cfg_=None), b"null cfg")]:
        assert call(**kw) == -1, kw
        assert text in L.lib.rtn_last_error(handle.raw), (kw, L.lib.rtn_last_error(handle.raw))
    assert call(nbytes=wsb - 1) == -3                                        # workspace too small
    assert b"workspace" in L.lib.rtn_last_error(handle.raw)
    assert L.lib.rtn_retina_loss_boxes_fwd(None, C.byref(cfg), 1, 1, p, p, p, p, 0.4, 0.5, p, p, 0.25, 2.0, 3.0, p, p, wsb) == -1
