"""Per-layer audit of device results against float64: references, per-element bounds and row sampling.

Host-only and free of the package (no librtn import), so its own sensitivity test (test_layer_audit.py) runs anywhere.  The GPU
audit (test_gpu_layer_audit.py) hands it the inputs a launch really read - the device's own bf16 / f32 bits, so inputs are exact -
and the layer table of weights.conv_layers; every layer's semantics (kernel, stride, padding, BN fold, activation, what is added)
come from that table and from the model definition restated here, never from an op's descriptor, so a wrong descriptor cannot check
itself.  The references are plain float64 products over gathered input rows: torch matmuls, no convolution primitive, so they run
the same on the CPU and on the GPU.

THE BOUND.  For every compared element
    bf16 output:  |got - ref| <= 2^-8 |ref| + gamma(L) A          f32 output:  |got - ref| <= 2^-22 |ref| + gamma(L) A
with A = the float64 sum of the absolute values of everything the element adds up (sum |w x| + |bias| + |residual|) and
gamma(L) = (L + 8) 2^-24, L the longest chain of sequential f32 additions of one output.  It is NEVER scaled by the largest value
of the layer.  Derivation: every f32 add of a chain rounds once, by at most 2^-24 times a partial sum, and every partial sum is at
most A; the products of bf16 operands are exact in f32.  The "+ 8" covers the adds inside one MFMA (a tree of depth <= 5 over the
32 products of v_mfma_f32_16x16x32_bf16), the bias / residual adds of the epilogue and, for f32 operands, the one rounding of each
product (at most 2^-24 A in all).  The output rounding is the relative term: half a bf16 ulp is 2^-8 of the value at most; for f32
outputs 2^-22 is four f32 ulps (one for the store, the rest for the f32 epilogue).  ReLU and sigmoid are 1-Lipschitz and keep the
bound; the sigmoid's own evaluation (expf, add, divide, each <= 2 ulps of its result, relative error carried through 1/(1+e)) adds
SIGMOID_REL |ref|.

L PER KERNEL FAMILY (see L_TABLE): a tile's f32 accumulator takes one MFMA per K step (every bf16 forward kernel uses
v_mfma_f32_16x16x32_bf16, the fp32 path v_mfma_f32_16x16x4_f32), so a launch without a workspace adds k times into one chain, plus
the bias.  A launch WITH a workspace may cut a tile's K loop into stream-K pieces or K slices whose partial sums the owner adds in
order - one more add per piece, and a piece holds at least one K step, so the pieces never add more than the steps do: L <= 2 k + 1
there, whatever the grid.  (`split` says which case a launch is in: the audit takes it from whether the launch has a workspace -
without one there is nowhere for a partial sum to go.)  Weight and bias gradients reduce over pixels: each of `splits` ordered
pieces runs its own chain over ceil(P / splits) pixels (32 per MFMA for the weights; every 4th pixel per lane for the fused bias
sums, then <= 16 lane partials), then the pieces are added in order: L = ceil(P / (splits x step)) + splits + 1 (+ 16 for the bias).

GRADIENTS OF THE TRAINING STEP (test_gpu_backward_audit.py).  A weight gradient is one such sum over P pixels: wgrad_ref, with the
chain lengths above.  The gradient of an activation T is m (.) sum_j c_j over its n consumers, m = (T > 0) where the model puts a
ReLU on T: dgrad_ref for a consuming convolution (L_j = conv_L of its kh kw Cout products per element), the sum's own gradient for
an identity add (L_j = 0), upsample_bwd_ref for UpsampleLike + Add (L_j = the destination pixels of one source pixel), maxpool_bwd_ref
for the pool (L_j = 4 windows).  The device writes the c_j one launch after another into one buffer of the activation's dtype, so the
running sum is rounded n - 1 times before the final rounding, each time by at most REL sum_j |c_j|:
    |got - ref| <= REL |ref| + gamma(max_j L_j + n) sum_j A_j + (n - 1) REL sum_j |c_j|
The mask distributes over the sum, so the reference does not depend on where a launch applies it.

Intermediates that a fused launch rounds to bf16 but does not store (the bneck's branch2b output h1, the stem's conv1 output) are
carried as an INTERVAL: the device's f32 value lies within gamma A of the float64 one, so its bf16 rounding lies between the
roundings of the two ends.  Where those differ (a rounding midpoint inside the interval), the next layer's bound gets
sum |w_next| x (hi - lo) for those positions only; elsewhere the rounding is known exactly.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24                     # f32 unit roundoff
REL = {"bf16": 2.0 ** -8, "f32": 2.0 ** -22}
SIGMOID_REL = 2.0 ** -20           # expf + add + divide, <= 2 ulps each, doubled
FULL_ROWS = 200_000                # outputs with at most this many rows (pixels x batch) are compared whole
BN_EPS = 1e-5

# L, the longest chain of sequential f32 adds of one output, per kernel family (K = reduction length, P = pixels)
L_TABLE = {
    # rtn_conv2d_fwd generations 1..5 and the fused kernels, bf16: one K step = 32 channels of one tap
    "conv_bf16": lambda K, split: (2 if split else 1) * -(-K // 32) + 1,      # k MFMAs (+ <= k pieces / slices) + bias
    # the fp32 parity path: one accumulate per 4 channels
    "conv_f32": lambda K, split: (2 if split else 1) * -(-K // 4) + 1,
    # weight gradients: `splits` ordered pixel pieces, 32 pixels per MFMA inside a piece, then the piece adds
    "wgrad_bf16": lambda P, splits: -(-P // (32 * splits)) + splits + 1,
    "wgrad_f32": lambda P, splits: -(-P // (4 * splits)) + splits + 1,
    # bias gradient (fused into the weight-gradient launch): inside a split every lane sums every 4th pixel of its rows (the
    # generation-2 kernel's four pixel groups - the longest chain of the families: generation 1 strides 16 rows, the window kernel
    # adds 32 pixels per MFMA), then at most 16 lane partials are folded in order, then the ordered split adds
    "bgrad": lambda P, splits: -(-P // (4 * splits)) + 16 + splits + 1,
}


def gamma(L):
    return (L + 8) * U


def conv_L(K, dtype, split=True):
    return L_TABLE["conv_bf16" if dtype == "bf16" else "conv_f32"](K, split)


# ------------------------------------------------------------------------------------------------------------- weights
def fold_bn_f32(kernel_hwio, bias, bn):
    """The float32 BN fold of the model definition (frozen BN, eps 1e-5), in the product's operation order:
    scale = gamma / sqrt(var + eps), w = w * scale, b = b * scale + (beta - mean * scale)."""
    w = torch.as_tensor(np.asarray(kernel_hwio), dtype=torch.float32)
    cout = w.shape[3]
    b = torch.zeros(cout) if bias is None else torch.as_tensor(np.asarray(bias), dtype=torch.float32)
    if bn is not None:
        g, beta, mean, var = [torch.as_tensor(np.asarray(t), dtype=torch.float32) for t in bn]
        scale = g / torch.sqrt(var + BN_EPS)
        w = w * scale.view(1, 1, 1, -1)
        b = b * scale + (beta - mean * scale)
    return w, b


def layer_weights(state, layer, dtype):
    """(w [cout, kh, kw, cin] float64 holding the device's rounding of the fold, b [cout] float64 of the f32 fold) of one
    weights.conv_layers entry."""
    name, kh, kw, cin, cout, has_bias, bn = layer
    bnp = None if bn is None else [state[bn + s] for s in ("/gamma", "/beta", "/moving_mean", "/moving_variance")]
    w, b = fold_bn_f32(state[name + "/kernel"], state.get(name + "/bias") if has_bias else None, bnp)
    if dtype == "bf16":
        w = w.to(torch.bfloat16)
    return w.permute(3, 0, 1, 2).double().contiguous(), b.double()


def same_pad_before(n, k, s):
    out = -(-n // s)
    return max((out - 1) * s + k - n, 0) // 2


def tf_upsample_index(n_in, n_out):
    """UpsampleLike (legacy TF nearest, align_corners=False): src = min(floor(dst * f32(n_in / n_out)), n_in - 1) in float32."""
    r = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * r).astype(np.int64), n_in - 1)


# ------------------------------------------------------------------------------------------------------------- sampling
def sample_rows(B, H, W, seed=0, full=FULL_ROWS):
    """Flattened output rows (b * H * W + y * W + x) to compare: all of them up to `full`, else every image's four corners and the
    two ends of its middle row, every multiple of 64 with both neighbours (capped at 4096 rows), the last 256 rows and >= 2048
    random rows spread over all images."""
    M = B * H * W
    if M <= full:
        return torch.arange(M)
    hw = H * W
    pick = []
    for b in range(B):
        o = b * hw
        mid = (H // 2) * W
        pick += [o, o + W - 1, o + (H - 1) * W, o + hw - 1, o + mid, o + mid + W - 1]
    seams = np.arange(0, M, 64)
    seams = seams[::-(-3 * len(seams) // 4096)]      # every k-th multiple when there are more: 64 k rows apart
    pick += list(np.concatenate([seams - 1, seams, seams + 1]))
    pick += list(range(M - 256, M))
    g = np.random.default_rng(seed)
    per = -(-2048 // B)
    for b in range(B):
        pick += list(b * hw + g.integers(0, hw, per))
    rows = np.unique(np.clip(np.asarray(pick, np.int64), 0, M - 1))
    return torch.as_tensor(rows)


# ------------------------------------------------------------------------------------------------------------- references
def gather(x, rows, Hout, Wout, kh, kw, stride, pad):
    """Rows of the implicit GEMM: x [B,H,W,C] (any dtype) -> float64 [R, kh*kw*C], (kh, kw, c) order, zero outside the image."""
    B, H, W, Cc = x.shape
    rows = rows.to(x.device)
    b = rows // (Hout * Wout)
    r = rows % (Hout * Wout)
    oy, ox = r // Wout, r % Wout
    cols = []
    for i in range(kh):
        iy = oy * stride - pad[0] + i
        for j in range(kw):
            ix = ox * stride - pad[1] + j
            ok = ((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).unsqueeze(1)
            v = x[b, iy.clamp(0, H - 1), ix.clamp(0, W - 1)].double()
            cols.append(torch.where(ok, v, torch.zeros_like(v)))
    return torch.cat(cols, 1)


def rows_of(t, rows):
    """t [B,H,W,C] -> float64 [R, C] at flattened rows."""
    return t.reshape(-1, t.shape[-1])[rows.to(t.device)].double()


def upsample_rows(res, rows, Hout, Wout):
    """The residual an RES_UPSAMPLE epilogue adds at the output rows: res[b, iy(oy), ix(ox)] (UpsampleLike of the model)."""
    Hr, Wr = res.shape[1], res.shape[2]
    rows = rows.to(res.device)
    b = rows // (Hout * Wout)
    r = rows % (Hout * Wout)
    iy = torch.as_tensor(tf_upsample_index(Hr, Hout), device=res.device)[r // Wout]
    ix = torch.as_tensor(tf_upsample_index(Wr, Wout), device=res.device)[r % Wout]
    return res[b, iy, ix].double()


def conv_ref(terms, bias=None, res=None, relu=False, sigmoid=False, chunk_elems=1 << 25):
    """terms: [(patch_fn, w)], each patch_fn(lo, hi) -> float64 [r, K] rows lo:hi of one operand, w [cout, K] float64 - the sum of
    several products (the dual op's two sources) is one output.  res: float64 [R, cout] or None.  Returns (ref, A) float64 [R, cout]:
    the activation of sum + bias + res and the sum of the absolute values of everything added."""
    R = res.shape[0] if res is not None else terms[0][2]
    refs, As = [], []
    K = max(t[1].shape[1] for t in terms)
    step = max(64, chunk_elems // max(K, 1))
    for lo in range(0, R, step):
        hi = min(R, lo + step)
        acc = a = None
        for fn, w, *_ in terms:
            p = fn(lo, hi)
            s = p @ w.t()
            sa = (p.abs().float() @ w.abs().float().t()).double()      # a bound term: float32 is ample
            acc = s if acc is None else acc + s
            a = sa if a is None else a + sa
        if bias is not None:
            acc = acc + bias
            a = a + bias.abs()
        if res is not None:
            acc = acc + res[lo:hi]
            a = a + res[lo:hi].abs()
        if relu:
            acc = acc.clamp_min(0)
        if sigmoid:
            acc = torch.sigmoid(acc)
        refs.append(acc)
        As.append(a)
    return torch.cat(refs), torch.cat(As)


def conv_rows_ref(x, rows, Hout, Wout, w, stride, pad, bias=None, res=None, relu=False, sigmoid=False):
    """One ordinary layer at the given output rows: w [cout, kh, kw, cin] float64."""
    cout, kh, kw, cin = w.shape
    fn = lambda lo, hi: gather(x, rows[lo:hi], Hout, Wout, kh, kw, stride, pad)
    return conv_ref([(fn, w.reshape(cout, -1).to(x.device), len(rows))], bias=None if bias is None else bias.to(x.device),
                    res=res, relu=relu, sigmoid=sigmoid)


def bf16_interval(v, slack, relu=True):
    """(lo, hi) float64: the bf16 roundings of the ends of [v - slack, v + slack] after ReLU - where a device value computed
    within `slack` of v rounds to."""
    f = (lambda t: t.clamp_min(0)) if relu else (lambda t: t)
    lo = f(v - slack).float().to(torch.bfloat16).double()
    hi = f(v + slack).float().to(torch.bfloat16).double()
    return lo, hi


def maxpool_rows(x, rows, Hout, Wout):
    """MaxPool 3x3 / 2 TF 'same' (-inf padding) of x [B,H,W,C] at flattened output rows: exact (a maximum does not round)."""
    B, H, W, Cc = x.shape
    pt, pl = same_pad_before(H, 3, 2), same_pad_before(W, 3, 2)
    p = gather(x, rows, Hout, Wout, 3, 3, 2, (pt, pl)).view(len(rows), 9, Cc)
    rows = rows.to(x.device)
    r = rows % (Hout * Wout)
    oy, ox = r // Wout, r % Wout
    for t in range(9):
        iy, ix = oy * 2 - pt + t // 3, ox * 2 - pl + t % 3
        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
        p[:, t][~ok] = -math.inf
    return p.max(1).values


def wgrad_ref(x, dy, kh, kw, stride, pad, out_rows=None):
    """dW[n, (kh, kw, c)] = sum over (b, oy, ox) of dy[b, oy, ox, n] x[b, oy*s - pt + i, ox*s - pl + j, c] for the output rows
    `out_rows` (default all) - an exact float64 sum over every pixel of every image - and A = the same sum of absolute values.
    Also the bias gradient sum dy over all pixels and its A."""
    B, Ho, Wo, N = dy.shape
    rows = torch.arange(B * Ho * Wo)
    P = gather(x, rows, Ho, Wo, kh, kw, stride, pad)
    D = dy.reshape(-1, N).double()
    if out_rows is not None:
        D = D[:, out_rows]
    return D.t() @ P, D.abs().t() @ P.abs(), D.sum(0), D.abs().sum(0)


def dgrad_ref(dy, w, Hin, Win, stride, pad):
    """Data gradient of a convolution at its input [B, Hin, Win, cin]: for every tap (i, j)
        dx[b, oy*s - pt + i, ox*s - pl + j, :] += dy[b, oy, ox, :] @ w[:, i, j, :]
    with positions outside the image dropped.  dy [B, Ho, Wo, cout] (any dtype), w [cout, kh, kw, cin] float64.  One matmul and one
    masked index-add per tap.  Returns (dx, A) float64 on dy's device, A the same sum over absolute values."""
    B, Ho, Wo, N = dy.shape
    cout, kh, kw, cin = w.shape
    assert cout == N, (cout, N)
    dev = dy.device
    w = w.to(dev)
    D = dy.reshape(-1, N).double()
    Da = D.abs()
    r = torch.arange(B * Ho * Wo, device=dev)
    b, oy, ox = r // (Ho * Wo), (r % (Ho * Wo)) // Wo, r % Wo
    dx = torch.zeros(B * Hin * Win, cin, dtype=torch.float64, device=dev)
    A = torch.zeros_like(dx)
    for i in range(kh):
        iy = oy * stride - pad[0] + i
        for j in range(kw):
            ix = ox * stride - pad[1] + j
            ok = (iy >= 0) & (iy < Hin) & (ix >= 0) & (ix < Win)
            tgt = (b * Hin * Win + iy * Win + ix)[ok]
            dx.index_add_(0, tgt, D[ok] @ w[:, i, j, :])
            A.index_add_(0, tgt, Da[ok] @ w[:, i, j, :].abs())
    return dx.view(B, Hin, Win, cin), A.view(B, Hin, Win, cin)


def upsample_bwd_ref(d_dst, Hs, Ws):
    """Gradient of UpsampleLike at its source [B, Hs, Ws, C]: every destination pixel sends its gradient to the source pixel
    tf_upsample_index reads it from (the scatter-add inverse of upsample_rows).  Returns (d_src, A) float64 on d_dst's device."""
    B, Hd, Wd, Cc = d_dst.shape
    dev = d_dst.device
    iy = torch.as_tensor(tf_upsample_index(Hs, Hd), device=dev)
    ix = torch.as_tensor(tf_upsample_index(Ws, Wd), device=dev)
    r = torch.arange(B * Hd * Wd, device=dev)
    tgt = (r // (Hd * Wd)) * Hs * Ws + iy[(r % (Hd * Wd)) // Wd] * Ws + ix[r % Wd]
    g = d_dst.reshape(-1, Cc).double()
    out = []
    for gg in (g, g.abs()):
        out.append(torch.zeros(B * Hs * Ws, Cc, dtype=torch.float64, device=dev).index_add_(0, tgt, gg).view(B, Hs, Ws, Cc))
    return out[0], out[1]


def pool_window_taps(xin):
    """The nine taps of every MaxPool 3x3 / 2 TF 'same' window of xin [B,H,W,C], in scan order: views [B,Ho,Wo,C] float64, -inf
    outside the image."""
    B, H, W, Cc = xin.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    pt, pl = same_pad_before(H, 3, 2), same_pad_before(W, 3, 2)
    xpad = torch.full((B, H + 4, W + 4, Cc), -math.inf, dtype=torch.float64, device=xin.device)
    xpad[:, pt:pt + H, pl:pl + W] = xin.double()
    return [xpad[:, t // 3:t // 3 + 2 * Ho - 1:2, t % 3:t % 3 + 2 * Wo - 1:2] for t in range(9)]


def maxpool_bwd_ref(dy, xin, mode, pool_out=None, arg=None):
    """Gradient of MaxPool 3x3 / 2 TF 'same' at its input [B,H,W,C]: every window sends dy to its FIRST maximum in scan order
    (kh, kw) - TensorFlow's tie rule - or to the tap `arg` [B,Ho,Wo,C] (kh * 3 + kw) where the caller has established the winners.  mode 1: dx = 0 where the input (a ReLU output) is <= 0; mode 2: a window passes its gradient
    only when the POOLED tensor `pool_out` (what the kernel reads as its mask) is > 0 there.  Returns (dx, A) float64 on dy's device:
    A = the same routing of |dy|, at most four terms per input pixel."""
    B, H, W, Cc = xin.shape
    Ho, Wo = dy.shape[1], dy.shape[2]
    pt, pl = same_pad_before(H, 3, 2), same_pad_before(W, 3, 2)
    dev = dy.device
    if arg is None:
        best = torch.full((B, Ho, Wo, Cc), -math.inf, dtype=torch.float64, device=dev)
        arg = torch.zeros(B, Ho, Wo, Cc, dtype=torch.uint8, device=dev)
        for t, v in enumerate(pool_window_taps(xin)):
            take = v > best                      # strict: the first maximum in scan order keeps its place
            best = torch.where(take, v, best)
            arg[take] = t
        del best
    g = dy.double()
    if mode == 2:
        g = torch.where(pool_out.to(dev) > 0, g, torch.zeros_like(g))
    out = []
    for gg in (g, g.abs()):
        dpad = torch.zeros(B, H + 4, W + 4, Cc, dtype=torch.float64, device=dev)
        for t in range(9):
            i, j = t // 3, t % 3
            dpad[:, i:i + 2 * Ho - 1:2, j:j + 2 * Wo - 1:2] += torch.where(arg == t, gg, torch.zeros_like(gg))
        out.append(dpad[:, pt:pt + H, pl:pl + W])
    dx, A = out
    if mode == 1:
        keep = xin.to(dev) > 0
        dx, A = torch.where(keep, dx, torch.zeros_like(dx)), torch.where(keep, A, torch.zeros_like(A))
    return dx, A


# ------------------------------------------------------------------------------------------------------------- comparison
def compare_interval(got, lo, hi):
    """got must lie in [lo, hi] (float64 tensors of one shape): worst distance outside / half-width (0 inside), violations."""
    g = got.double().to(lo.device)
    out = torch.maximum(lo - g, g - hi).clamp_min(0)
    out = torch.where(torch.isfinite(g), out, torch.full_like(out, math.inf))
    half = ((hi - lo) / 2).clamp_min(1e-300)
    ratio = torch.where(out > 0, 1 + out / half, torch.zeros_like(out))
    nbad = int((out > 0).sum())
    return {"worst": float(ratio.max()) if ratio.numel() else 0.0, "bad": nbad, "where": None, "n": int(g.numel())}


def compare(got, ref, A, L, out_dtype, extra=None, sigmoid=False):
    """Worst err / bound over the elements and the number of violations.  got: any dtype, same shape as ref."""
    g = got.double().to(ref.device)
    rel = REL[out_dtype] + (SIGMOID_REL if sigmoid else 0.0)
    bnd = rel * ref.abs() + gamma(L) * A.to(ref.device)
    if extra is not None:
        bnd = bnd + extra
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, math.inf))
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    nbad = int((ratio > 1).sum())
    where = None
    if nbad:
        flat = int(ratio.reshape(-1).argmax())
        where = divmod(flat, ref.shape[-1]) if ref.dim() > 1 else (flat, 0)
    return {"worst": worst, "bad": nbad, "where": where, "n": int(ref.numel())}
