"""Sensitivity of the per-layer comparator (tests/layer_audit.py), on the CPU.

A correct kernel is emulated - f32 accumulation in K steps of 32 channels over 64 x 256 tiles, a stream-K split of the K loop,
bias / residual / ReLU epilogue, one bf16 rounding - and must pass; every injected defect a real tiling can produce must be flagged
by the same bounds the GPU audit uses.  This is the evidence that the bounds are tight enough to see a subtly wrong kernel."""
import math

import pytest
import torch

import layer_audit as LA

B, H, W, CIN, COUT = 4, 11, 13, 64, 320          # 572 rows: nine 64-row tiles, the last one 60 rows; two column blocks of 256
TM, TN, KS = 64, 256, 32


def bf(t):
    return t.to(torch.bfloat16)


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(5)
    x = bf(torch.relu(torch.randn(B, H, W, CIN, generator=g)))
    w = bf(torch.randn(COUT, 3, 3, CIN, generator=g) * math.sqrt(2.0 / (9 * CIN))).double()
    bias = (0.5 * torch.randn(COUT, generator=g)).float().double()
    res = bf(torch.randn(B, H, W, COUT, generator=g))
    return {"x": x, "w": w, "bias": bias, "res": res}


def emulate(c, defect=None, pieces=1):
    """The f32 tile computation of a 3x3 'same' conv + bias + residual + ReLU, bf16 out; `pieces` cuts every tile's K loop into
    stream-K pieces whose partial sums the owner adds in order.  Returns [B, H, W, COUT] bf16."""
    rows = torch.arange(B * H * W)
    P = LA.gather(c["x"], rows, H, W, 3, 3, 1, (1, 1)).float()
    Wm = c["w"].reshape(COUT, -1).float()
    M, K = P.shape
    nk = K // KS
    bias = c["bias"].float()
    mid = (B // 2) * H * W + 2 * TM                # a tile of a middle image
    cuts = [round(i * nk / pieces) for i in range(pieces + 1)]
    acc = None
    for pi in range(pieces):
        part = (bias.expand(M, COUT).clone() if pi == 0 else torch.zeros(M, COUT))
        for k in range(cuts[pi], cuts[pi + 1]):
            step = P[:, k * KS:(k + 1) * KS] @ Wm[:, k * KS:(k + 1) * KS].t()
            if defect == "drop_kstep" and k == nk // 2:
                step[mid:mid + TM, :TN] = 0
            part = part + step
        acc = part if acc is None else acc + part
    if defect == "bias_twice":
        acc[mid:mid + TM, :TN] += bias[:TN]
    r = c["res"].reshape(M, COUT).float()
    pre = acc + r
    if defect == "res_twice":
        pre[:, TN:] += r[:, TN:]
    out = torch.relu(pre)
    if defect == "relu_group":
        out[:, 8:16] = torch.where(pre[:, 16:24] > 0, pre[:, 8:16], torch.zeros_like(pre[:, 8:16]))
    out = bf(out)
    if defect == "tail_shift":
        last = (M // TM) * TM
        out[last:] = out[last - 1:M - 1].clone()
    return out.view(B, H, W, COUT)


def audit(c, got, split):
    rows = LA.sample_rows(B, H, W)
    ref, A = LA.conv_rows_ref(c["x"], rows, H, W, c["w"], 1, (1, 1), bias=c["bias"], res=LA.rows_of(c["res"], rows), relu=True)
    return LA.compare(LA.rows_of(got, rows), ref, A, LA.conv_L(9 * CIN, "bf16", split), "bf16")


@pytest.mark.parametrize("pieces", [1, 3])
def test_correct_emulation_passes(case, pieces):
    r = audit(case, emulate(case, pieces=pieces), split=pieces > 1)
    assert r["bad"] == 0 and r["worst"] <= 1.0, r
    assert r["n"] == B * H * W * COUT


@pytest.mark.parametrize("defect", ["drop_kstep", "tail_shift", "res_twice", "relu_group", "bias_twice"])
def test_conv_defects_are_flagged(case, defect):
    pieces = 3 if defect == "bias_twice" else 1
    r = audit(case, emulate(case, defect, pieces=pieces), split=pieces > 1)
    assert r["bad"] > 0, (defect, r)


def test_sampling_covers_seams_corners_and_tail():
    Bs, Hs, Ws = 8, 200, 334
    rows = LA.sample_rows(Bs, Hs, Ws, seed=1)
    M, hw = Bs * Hs * Ws, Hs * Ws
    s = set(rows.tolist())
    assert len(rows) < LA.FULL_ROWS
    for b in range(Bs):
        assert {b * hw, b * hw + Ws - 1, b * hw + (Hs - 1) * Ws, b * hw + hw - 1} <= s
        assert sum(1 for r in s if b * hw <= r < (b + 1) * hw) >= 2048 // Bs
    assert set(range(M - 256, M)) <= s
    seams = [r for r in range(64, M - 1, 64) if {r - 1, r, r + 1} <= s]
    assert len(seams) >= 1000
    assert torch.equal(LA.sample_rows(2, 10, 10), torch.arange(200))


def test_interval_for_an_unstored_bf16_intermediate():
    """A fused pair (3x3 + ReLU, rounded to bf16 in registers, then 1x1 + ReLU): the device's f32 value of the intermediate may sit on
    the other side of a rounding midpoint from the float64 one; the interval reference accepts exactly those positions and still
    flags a wrong second stage."""
    g = torch.Generator().manual_seed(9)
    Bn, Hn, Wn, C1, C2 = 2, 9, 10, 64, 256
    a = bf(torch.relu(torch.randn(Bn, Hn, Wn, C1, generator=g)))
    w1 = bf(torch.randn(C1, 3, 3, C1, generator=g) * math.sqrt(2.0 / (9 * C1))).double()
    w2 = bf(torch.randn(C2, 1, 1, C1, generator=g) * math.sqrt(2.0 / C1)).double()
    rows = torch.arange(Bn * Hn * Wn)
    # the "device": f32 sums in reversed K order (another valid order), h1 rounded to bf16, then the 1x1
    P = LA.gather(a, rows, Hn, Wn, 3, 3, 1, (1, 1)).float()
    h1 = torch.zeros(len(rows), C1)
    for k in reversed(range(P.shape[1] // KS)):
        h1 = h1 + P[:, k * KS:(k + 1) * KS] @ w1.reshape(C1, -1).float()[:, k * KS:(k + 1) * KS].t()
    h1 = bf(torch.relu(h1))
    y = bf(torch.relu(h1.float() @ w2.reshape(C2, -1).float().t()))
    # reference: h1 in float64, its interval, then the second stage with the propagated width
    v, A1 = LA.conv_rows_ref(a, rows, Hn, Wn, w1, 1, (1, 1), relu=True)
    lo, hi = LA.bf16_interval(v, LA.gamma(LA.conv_L(9 * C1, "bf16", False)) * A1)
    assert bool(((h1.double() >= lo) & (h1.double() <= hi)).all())
    mid = v.float().to(torch.bfloat16).double()
    ref, A = LA.conv_rows_ref(mid.view(Bn, Hn, Wn, C1), rows, Hn, Wn, w2, 1, (0, 0), relu=True)
    extra = (hi - lo) @ w2.reshape(C2, -1).abs().t()
    r = LA.compare(y.reshape(-1, C2), ref, A, LA.conv_L(C1, "bf16", False), "bf16", extra=extra)
    assert r["bad"] == 0, r
    bad = y.reshape(-1, C2).clone()
    bad[:, 3] = bf(torch.relu(h1.float() @ w2.reshape(C2, -1).float()[4].t()))          # one filter row read off by one
    assert LA.compare(bad, ref, A, LA.conv_L(C1, "bf16", False), "bf16", extra=extra)["bad"] > 0


def test_wgrad_missing_image_is_flagged():
    """Batch-16 weight gradient of a 3x3 layer: f32 partial sums per 32-pixel step; one image left out must be flagged, the whole
    batch passes."""
    g = torch.Generator().manual_seed(11)
    Bn, Hn, Wn, C1, C2 = 16, 6, 7, 32, 64
    x = bf(torch.relu(torch.randn(Bn, Hn, Wn, C1, generator=g)))
    dy = bf(torch.randn(Bn, Hn, Wn, C2, generator=g))
    ref, A, bref, bA = LA.wgrad_ref(x, dy, 3, 3, 1, (1, 1))
    L = LA.L_TABLE["wgrad_bf16"](Bn * Hn * Wn, 1)

    def emulate(skip=None):
        keep = [b for b in range(Bn) if b != skip]
        P = LA.gather(x[keep], torch.arange(len(keep) * Hn * Wn), Hn, Wn, 3, 3, 1, (1, 1)).float()
        D = dy[keep].reshape(-1, C2).float()
        acc = torch.zeros(C2, P.shape[1])
        for lo in range(0, P.shape[0], 32):
            acc = acc + D[lo:lo + 32].t() @ P[lo:lo + 32]
        return acc, D.sum(0)

    good, gb = emulate()
    assert LA.compare(good, ref, A, L, "f32")["bad"] == 0
    assert LA.compare(gb, bref, bA, LA.L_TABLE["bgrad"](Bn * Hn * Wn, 1), "f32")["bad"] == 0
    badw, badb = emulate(skip=9)
    assert LA.compare(badw, ref, A, L, "f32")["bad"] > 0
    assert LA.compare(badb, bref, bA, LA.L_TABLE["bgrad"](Bn * Hn * Wn, 1), "f32")["bad"] > 0


def test_poolbwd_mode2_first_maximum():
    """MaxPool backward with the ReLU mask taken from the pooled tensor (mode 2): ties go to the FIRST maximum in scan order.  Small
    integers make ties common; a kernel that sends the gradient to the last maximum is flagged, element by element."""
    g = torch.Generator().manual_seed(3)
    Bn, Hn, Wn, Cn = 2, 9, 11, 16          # TF 'same' pads 1 / 1 on both axes: a flip maps windows onto windows
    xin = torch.randint(-1, 3, (Bn, Hn, Wn, Cn), generator=g).float().clamp_min(0)      # a ReLU output with many ties
    Ho, Wo = (Hn + 1) // 2, (Wn + 1) // 2
    pooled = LA.maxpool_rows(xin, torch.arange(Bn * Ho * Wo), Ho, Wo).view(Bn, Ho, Wo, Cn)
    dy = bf(torch.randn(Bn, Ho, Wo, Cn, generator=g))
    want, A = LA.maxpool_bwd_ref(dy, xin, 2, pooled)
    # the last maximum: scan the taps backwards with the same strict comparison
    flipped = LA.maxpool_bwd_ref(dy.flip(1, 2), xin.flip(1, 2), 2, pooled.flip(1, 2))[0].flip(1, 2)
    assert LA.compare(want, want, A, 4, "bf16")["bad"] == 0
    assert LA.compare(flipped, want, A, 4, "bf16")["bad"] > 0
    # mode 1 against mode 2 on a ReLU output: the same gradient; mode 2 reads its mask from the pooled tensor it is given
    assert torch.equal(LA.maxpool_bwd_ref(dy, xin, 1)[0], want)
    assert not torch.equal(LA.maxpool_bwd_ref(dy, xin, 2, pooled - 1)[0], want)


def test_gradient_bounds_see_one_image_at_the_benched_training_size():
    """The bias and weight gradients of a res2 layer at the benched training shape (16 x 200 x 334 pixels): with the reduction's
    real structure in L (ordered pixel pieces, then the piece adds), one image of 16 left out is still flagged, and a correct f32
    reduction in that structure passes."""
    g = torch.Generator().manual_seed(13)
    Bn, Hn, Wn, C1, C2, splits = 16, 200, 334, 8, 8, 64
    P = Bn * Hn * Wn
    x = bf(torch.relu(torch.randn(Bn, Hn, Wn, C1, generator=g)))
    dy = bf(torch.randn(Bn, Hn, Wn, C2, generator=g) * 1e-3)
    ref, A, bref, bA = LA.wgrad_ref(x, dy, 1, 1, 1, (0, 0))
    Lw, Lb = LA.L_TABLE["wgrad_bf16"](P, splits), LA.L_TABLE["bgrad"](P, splits)

    def emulate(skip=None):
        X = x.reshape(-1, C1).float()
        D = dy.reshape(-1, C2).float()
        if skip is not None:
            D = D.clone()
            D[skip * Hn * Wn:(skip + 1) * Hn * Wn] = 0
        per = -(-P // splits)
        w = torch.zeros(C2, C1)
        b = torch.zeros(C2)
        for lo in range(0, P, per):                   # ordered pieces, each an f32 reduction of its own
            w = w + D[lo:lo + per].t() @ X[lo:lo + per]
            b = b + D[lo:lo + per].sum(0)
        return w, b

    w, b = emulate()
    assert LA.compare(w, ref, A, Lw, "f32")["bad"] == 0
    assert LA.compare(b, bref, bA, Lb, "f32")["bad"] == 0
    w, b = emulate(skip=9)
    assert LA.compare(w, ref, A, Lw, "f32")["bad"] > 0
    assert LA.compare(b, bref, bA, Lb, "f32")["bad"] > 0


# ------------------------------------------------------------------------------------------------- gradients of the training step
def dgrad_f32(dy, w, Hin, Win, stride, pad, drop=None, odd=False):
    """The device's data gradient emulated: f32 accumulation over the taps in K steps of 32 gradient channels, nothing rounded before
    the caller's epilogue.  drop = (tap i, tap j, input column): that tap never reaches that column (a border test off by one);
    odd: the stride grid starts at pixel 1 instead of pixel 0.  Returns [B, Hin, Win, cin] f32."""
    Bn, Ho, Wo, N = dy.shape
    cout, kh, kw, cin = w.shape
    D = dy.reshape(-1, N).float()
    r = torch.arange(Bn * Ho * Wo)
    b, oy, ox = r // (Ho * Wo), (r % (Ho * Wo)) // Wo, r % Wo
    dx = torch.zeros(Bn * Hin * Win, cin)
    for i in range(kh):
        iy = oy * stride - pad[0] + i + (1 if odd else 0)
        for j in range(kw):
            ix = ox * stride - pad[1] + j + (1 if odd else 0)
            ok = (iy >= 0) & (iy < Hin) & (ix >= 0) & (ix < Win)
            if drop is not None and (i, j) == drop[:2]:
                ok = ok & (ix != drop[2])
            wt = w[:, i, j, :].float()
            for k in range(0, N, KS):
                dx.index_add_(0, (b * Hin * Win + iy * Win + ix)[ok], D[ok][:, k:k + KS] @ wt[k:k + KS])
    return dx.view(Bn, Hin, Win, cin)


@pytest.fixture(scope="module")
def gcase():
    g = torch.Generator().manual_seed(21)
    Bn, Hn, Wn, Cn = 2, 9, 11, 64
    return {"B": Bn, "H": Hn, "W": Wn, "C": Cn,
            "w3": bf(torch.randn(Cn, 3, 3, Cn, generator=g) * math.sqrt(2.0 / (9 * Cn))).double(),
            "w1": bf(torch.randn(Cn, 1, 1, Cn, generator=g) * math.sqrt(2.0 / Cn)).double(),
            "dy": bf(torch.randn(Bn, Hn, Wn, Cn, generator=g)),
            "dy2": bf(torch.randn(Bn, (Hn + 1) // 2, (Wn + 1) // 2, Cn, generator=g)),
            "ident": bf(torch.randn(Bn, Hn, Wn, Cn, generator=g)),
            "act": bf(torch.relu(torch.randn(Bn, Hn, Wn, Cn, generator=g)))}


def test_one_dropped_pixel_of_a_weight_gradient_is_flagged():
    """A 3x3 layer at P = 2 x 80 x 112 pixels under the bound the GPU audit uses (splits = 1): the f32 reduction in 32-pixel steps
    passes, and so does one cut into 7 ordered pieces; one pixel of 17920 left out of the sum is flagged."""
    g = torch.Generator().manual_seed(17)
    Bn, Hn, Wn, C1, C2 = 2, 80, 112, 16, 16
    P = Bn * Hn * Wn
    x = bf(torch.relu(torch.randn(Bn, Hn, Wn, C1, generator=g)))
    dy = bf(torch.randn(Bn, Hn, Wn, C2, generator=g))
    ref, A, bref, bA = LA.wgrad_ref(x, dy, 3, 3, 1, (1, 1))
    Lw, Lb = LA.L_TABLE["wgrad_bf16"](P, 1), LA.L_TABLE["bgrad"](P, 1)
    G = LA.gather(x, torch.arange(P), Hn, Wn, 3, 3, 1, (1, 1)).float()

    def emulate(pieces, skip=None):
        D = dy.reshape(-1, C2).float().clone()
        if skip is not None:
            D[skip] = 0
        per = -(-P // pieces)
        w, b = torch.zeros(C2, G.shape[1]), torch.zeros(C2)
        for p0 in range(0, P, per):
            pw, pb = torch.zeros(C2, G.shape[1]), torch.zeros(C2)
            for lo in range(p0, min(P, p0 + per), 32):
                hi = min(lo + 32, p0 + per)
                pw = pw + D[lo:hi].t() @ G[lo:hi]
                pb = pb + D[lo:hi].sum(0)
            w, b = w + pw, b + pb
        return w, b

    for pieces in (1, 7):
        w, b = emulate(pieces)
        assert LA.compare(w, ref, A, Lw, "f32")["bad"] == 0 and LA.compare(b, bref, bA, Lb, "f32")["bad"] == 0, pieces
    w, b = emulate(1, skip=Hn * Wn + 37 * Wn + 5)
    assert LA.compare(w, ref, A, Lw, "f32")["bad"] > 0


def test_dropped_border_tap_of_a_data_gradient_is_flagged(gcase):
    c = gcase
    ref, A = LA.dgrad_ref(c["dy"], c["w3"], c["H"], c["W"], 1, (1, 1))
    L = LA.conv_L(9 * c["C"], "bf16")
    good = bf(dgrad_f32(c["dy"], c["w3"], c["H"], c["W"], 1, (1, 1)))
    assert LA.compare(good, ref, A, L, "bf16")["bad"] == 0
    for col, tap in ((0, (1, 0)), (c["W"] - 1, (2, 2))):          # the tap that reaches the first / last column from inside the image
        bad = bf(dgrad_f32(c["dy"], c["w3"], c["H"], c["W"], 1, (1, 1), drop=tap + (col,)))
        r = LA.compare(bad, ref, A, L, "bf16")
        assert r["bad"] > 0, (col, tap, r)
        assert torch.equal(bad[:, :, 1:-1], good[:, :, 1:-1])     # the defect is confined to that one column


def test_stride2_gradient_on_the_odd_grid_is_flagged(gcase):
    """A stride-2 1x1 'valid' convolution: its data gradient lives on the even pixels; the same values one pixel off are flagged."""
    c = gcase
    ref, A = LA.dgrad_ref(c["dy2"], c["w1"], c["H"], c["W"], 2, (0, 0))
    assert not bool(ref[:, 1::2].any()) and not bool(ref[:, :, 1::2].any()) and bool(ref[:, ::2, ::2].any())
    L = LA.conv_L(c["C"], "bf16")
    assert LA.compare(bf(dgrad_f32(c["dy2"], c["w1"], c["H"], c["W"], 2, (0, 0))), ref, A, L, "bf16")["bad"] == 0
    assert LA.compare(bf(dgrad_f32(c["dy2"], c["w1"], c["H"], c["W"], 2, (0, 0), odd=True)), ref, A, L, "bf16")["bad"] > 0


def test_relu_mask_on_one_contribution_only_is_flagged(gcase):
    """A block input T = relu(.) with two consumers: the next block's identity add (its gradient arrives unmasked, as an alias of the
    sum's gradient) and a 1x1 convolution.  dT = (T > 0) (ident + dgrad); masking the convolution's part alone leaves the identity
    gradient alive where T = 0.  The bound of the GPU audit for a sum of n = 2 contributions."""
    c = gcase
    conv, Ac = LA.dgrad_ref(c["dy"], c["w1"], c["H"], c["W"], 1, (0, 0))
    ident = c["ident"].double()
    m = c["act"] > 0
    zero = torch.zeros_like(conv)
    ref, A = torch.where(m, conv + ident, zero), torch.where(m, Ac + ident.abs(), zero)
    n = 2
    L = LA.conv_L(c["C"], "bf16") + n
    extra = (n - 1) * LA.REL["bf16"] * torch.where(m, conv.abs() + ident.abs(), zero)
    f32 = dgrad_f32(c["dy"], c["w1"], c["H"], c["W"], 1, (0, 0))
    good = bf(torch.where(m, f32 + c["ident"].float(), torch.zeros_like(f32)))
    assert LA.compare(good, ref, A, L, "bf16", extra=extra)["bad"] == 0
    # written in two launches: the identity part masked and rounded first, the convolution added to it
    two = bf(torch.where(m, f32, torch.zeros_like(f32)) + bf(torch.where(m, c["ident"].float(), torch.zeros_like(f32))).float())
    assert LA.compare(two, ref, A, L, "bf16", extra=extra)["bad"] == 0
    bad = bf(torch.where(m, f32, torch.zeros_like(f32)) + c["ident"].float())
    assert LA.compare(bad, ref, A, L, "bf16", extra=extra)["bad"] > 0


def test_upsample_bwd_ref_inverts_the_forward_index():
    g = torch.Generator().manual_seed(2)
    Bn, Hs, Ws, Hd, Wd, Cn = 2, 5, 7, 10, 14, 3
    d = torch.randn(Bn, Hd, Wd, Cn, generator=g)
    src = torch.randn(Bn, Hs, Ws, Cn, generator=g).double()
    up = LA.upsample_rows(src, torch.arange(Bn * Hd * Wd), Hd, Wd).view(Bn, Hd, Wd, Cn)
    got, A = LA.upsample_bwd_ref(d, Hs, Ws)
    assert abs(float((up * d.double()).sum()) - float((src * got).sum())) <= 1e-9          # <U s, d> = <s, U^T d>
    assert torch.equal(A, LA.upsample_bwd_ref(d.abs(), Hs, Ws)[0])
    got2, _ = LA.upsample_bwd_ref(d[:, :9, :13], Hs, Ws)                                   # odd extents: 9 x 13 over 5 x 7
    assert abs(float(got2.sum()) - float(d[:, :9, :13].double().sum())) <= 1e-9


@pytest.mark.parametrize("Hn,Wn,k,s", [(9, 11, 3, 1), (10, 13, 3, 2), (9, 12, 3, 2), (9, 11, 1, 2)])
def test_dgrad_ref_is_the_adjoint_of_the_forward_reference(Hn, Wn, k, s):
    """<conv(x), dy> = <x, dgrad(dy)> against conv_rows_ref, at even and odd extents of the stride-2 'same' padding."""
    g = torch.Generator().manual_seed(Hn * Wn + k)
    Bn, C1, C2 = 2, 5, 6
    x = torch.randn(Bn, Hn, Wn, C1, generator=g).double()
    w = torch.randn(C2, k, k, C1, generator=g).double()
    Ho, Wo = -(-Hn // s), -(-Wn // s)
    pad = (LA.same_pad_before(Hn, k, s), LA.same_pad_before(Wn, k, s))
    dy = torch.randn(Bn, Ho, Wo, C2, generator=g).double()
    y, _ = LA.conv_rows_ref(x, torch.arange(Bn * Ho * Wo), Ho, Wo, w, s, pad)
    dx, A = LA.dgrad_ref(dy, w, Hn, Wn, s, pad)
    assert abs(float((y * dy.reshape(-1, C2)).sum()) - float((x * dx).sum())) <= 1e-9 * float(A.sum())
    assert bool((A >= dx.abs() - 1e-12).all())
