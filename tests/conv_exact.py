"""Exact-operand cases for the convolution kernels (no GPU): small-integer operands, the float64 reference of every kernel family
and fusion, and the conditions that make an equality test on them meaningful.

Method.  Inputs in [-3, 3], filters in [-2, 2] (ternary for the 1x1 filters of the fused chains), integer biases of the order of
+-600.  Every product and every partial sum is then an integer below 2^24, exact in f32 in ANY order of the additions, so a kernel
may differ from the float64 reference only in the roundings the header documents: the output must equal the reference rounded
once, bit for bit.  Each case carries its `stages`: one record per rounding point with the exact value in front of the rounding,
the bound  sum |x| |w| + |bias| + |residual|  of the sums that lead to it, and the format it is rounded to.  Case.check() asserts

  exactness        every stage's bound is below 2^24;
  rounding         of every compared bf16 (and e4m3) tensor at least 5 % of the elements are not representable before the final
                   rounding and at least 2 % are exact ties (for bf16: odd integers in (256, 512), ...), where round-to-nearest-even,
                   round-half-away and truncation all differ - this is what the wide bias is for;
  not degenerate   after a ReLU between 20 % and 80 % of the elements are non-zero; every mask tensor holds zeros of both signs,
                   positive and negative values;

and that the reference changes when the final rounding is replaced by truncation.  A case that misses one is a bug of the test,
not a pass.  tests/test_conv_exact_cases.py runs check() on every case without a GPU; tests/test_gpu_conv_exact.py (and the
register-epilogue tests of tests/test_gpu_conv.py) compare the kernels with the cases' `want` tensors by torch.equal."""
import functools
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

BIAS = 600                      # integer biases are drawn from [-BIAS, BIAS]
F8 = torch.float8_e4m3fn
LEVELS2 = [(12, 11), (2, 3)]    # 264 + 12 rows at batch 2: two tiles at every tile height, a group boundary inside the second
HEAD_LEVELS = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]


# ------------------------------------------------------------------------------------------------ number formats
def bf16(x):
    """Round to nearest even to bf16 (torch's cast), back in float64."""
    return x.to(torch.bfloat16).to(torch.float64)


def _f32_bits(x):
    f = x.to(torch.float32)
    assert torch.equal(f.to(torch.float64), x), "not exact in f32"
    return f.contiguous().view(torch.int32)


def trunc_bf16(x):
    """The bf16 value a truncating store would write (the low 16 bits of the f32 dropped)."""
    return (_f32_bits(x) & -65536).view(torch.float32).to(torch.float64)


def e4m3(x):
    """clamp to +-448 and round to nearest even to e4m3 (torch's float8_e4m3fn cast), back in float64."""
    return torch.clamp(x, -448.0, 448.0).to(torch.float32).to(F8).to(torch.float64)


def e4m3_bytes(x):
    return torch.clamp(x, -448.0, 448.0).to(torch.float32).to(F8).view(torch.uint8)


def trunc_e4m3(x):
    """The e4m3 value of the same clamp with the rounding replaced by truncation toward zero (one code down where RNE went up)."""
    v = torch.clamp(x, -448.0, 448.0)
    codes = v.to(torch.float32).to(F8).view(torch.uint8).to(torch.int16)
    r = codes.to(torch.uint8).view(F8).to(torch.float64)
    up = r.abs() > v.abs()
    return torch.where(up, codes - 1, codes).to(torch.uint8).view(F8).to(torch.float64)


def rounding_shares(pre, fmt):
    """(share of elements not representable in `fmt`, share that are exact ties between two neighbours) of the exact tensor."""
    if fmt == "bf16":
        low = _f32_bits(pre) & 0xFFFF
        return float((low != 0).double().mean()), float((low == 0x8000).double().mean())
    assert fmt == "e4m3"
    v = torch.clamp(pre, -448.0, 448.0)
    r = e4m3(v)
    other = 2 * v - r                                   # the mirror image of the chosen neighbour: a tie when that is a code too
    return float((r != v).double().mean()), float(((r != v) & (e4m3(other) == other)).double().mean())


# Floors of the share of exact ties.  bf16: 2 %.  e4m3 keeps three mantissa bits: of the integers (times a power of two) of one binade
# exactly 8 are ties whatever the binade, so outputs spread evenly over +-1200 hold 7 binades x 8 ties per sign, 4.7 %, and 2.3 % behind
# a ReLU that zeroes half of them - the floor for e4m3 is half of that expectation.
TIE_FLOOR = {"bf16": 0.02, "e4m3": 0.01}
ROUND = {"bf16": bf16, "e4m3": e4m3, "f32": lambda x: x}
TRUNC = {"bf16": trunc_bf16, "e4m3": trunc_e4m3}


class Stage(NamedTuple):
    name: str
    pre: torch.Tensor           # exact float64 value in front of the stage's rounding (after residual, mask and ReLU)
    bound: torch.Tensor         # sum |x| |w| + |bias| + |residual| of every element
    relu: bool
    fmt: str                    # "bf16", "e4m3" or "f32" (no rounding at all)

    @property
    def want(self):
        return ROUND[self.fmt](self.pre)

    def check(self):
        assert float(self.bound.max()) < 2 ** 24, "%s: a partial sum may reach %g" % (self.name, float(self.bound.max()))
        assert torch.equal(self.pre.to(torch.float32).to(torch.float64), self.pre), "%s: not exact in f32" % self.name
        if self.fmt != "f32":
            nonrep, ties = rounding_shares(self.pre, self.fmt)
            assert nonrep >= 0.05 and ties >= TIE_FLOOR[self.fmt], "%s: %.1f %% need rounding, %.1f %% ties" % (self.name, 100 * nonrep, 100 * ties)
            assert not torch.equal(TRUNC[self.fmt](self.pre), self.want), "%s: truncation gives the same tensor" % self.name
        if self.relu:
            nz = float((self.pre != 0).double().mean())
            assert 0.2 <= nz <= 0.8, "%s: %.1f %% non-zero after the ReLU" % (self.name, 100 * nz)


def check_mask(act):
    """Zeros of both signs (neither passes), positive and negative values."""
    z = act == 0
    assert bool((z & torch.signbit(act)).any()) and bool((z & ~torch.signbit(act)).any()) and bool((act > 0).any()) and bool((act < 0).any())


class Case:
    """Base: `stages` (list of Stage) and `masks` (list of mask tensors) are filled by the subclass."""
    name = ""

    def check(self):
        assert self.stages
        for s in self.stages:
            s.check()
        for m in self.masks:
            check_mask(m)

    def stats(self):
        return [(s.name, s.fmt) + (rounding_shares(s.pre, s.fmt) if s.fmt != "f32" else (0.0, 0.0)) + (float(s.bound.max()),) for s in self.stages]


# ------------------------------------------------------------------------------------------------ reference pieces
def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def ternary(g, *shape):
    """Sparse ternary 1x1 filters of the fused chains: +-1 with probability 1/8 each.  The second and third products of a chain multiply
    outputs of the stage before, already of the order of the bias; the sparse filters keep those sums within a few thousand, where
    bf16 still has a tie every 16 or 32 integers."""
    return ints(g, -1, 1, *shape) * (ints(g, 0, 7, *shape) < 3).double()


def geometry(H, W, k, stride, pad):
    """(Hout, Wout, pad_top, pad_left); pad "same" is TF's: pad_before = floor(pad_total / 2)."""
    if pad == "same":
        Ho, Wo = -(-H // stride), -(-W // stride)
        return Ho, Wo, max((Ho - 1) * stride + k - H, 0) // 2, max((Wo - 1) * stride + k - W, 0) // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, pad, pad


def ref_conv(x, w_hwio, bias, stride, pad_t, pad_l, Hout, Wout):
    """x (B,H,W,C) f64, taps outside the image are zero; output extent given."""
    kh, kw = w_hwio.shape[0], w_hwio.shape[1]
    H, W = x.shape[1], x.shape[2]
    pb = max((Hout - 1) * stride + kh - pad_t - H, 0)
    pr = max((Wout - 1) * stride + kw - pad_l - W, 0)
    xp = F.pad(x.permute(0, 3, 1, 2), (pad_l, pr, pad_t, pb))
    y = F.conv2d(xp, w_hwio.permute(3, 2, 0, 1), None, stride=stride)[:, :, :Hout, :Wout]
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    return y.permute(0, 2, 3, 1).contiguous()


def ref_conv_transpose(dy, w_hwio, stride, pad_t, pad_l, H, W):
    """Adjoint of ref_conv in x: dy (B,Ho,Wo,Cout) f64 -> (B,H,W,Cin)."""
    full = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w_hwio.permute(3, 2, 0, 1), stride=stride)      # row i of `full` is input row i - pad_t
    full = F.pad(full, (0, max(W + pad_l - full.shape[3], 0), 0, max(H + pad_t - full.shape[2], 0)))
    return full[:, :, pad_t:pad_t + H, pad_l:pad_l + W].permute(0, 2, 3, 1).contiguous()


def upsample_nearest_legacy(src, oh, ow):
    ih, iw = src.shape[1], src.shape[2]
    ys = np.minimum(np.floor(np.arange(oh, dtype=np.float32) * (np.float32(ih) / np.float32(oh))).astype(np.int64), ih - 1)
    xs = np.minimum(np.floor(np.arange(ow, dtype=np.float32) * (np.float32(iw) / np.float32(ow))).astype(np.int64), iw - 1)
    return src[:, torch.as_tensor(ys)][:, :, torch.as_tensor(xs)]


def mask_tensor(g, *shape):
    """A forward activation in [-1, 3] (60 % positive) with the special values of the existing mask tests in its first pixel."""
    act = ints(g, -1, 3, *shape)
    act[0, 0, 0, :8] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 0.5, 0.0], dtype=torch.float64)
    return bf16(act)


def epilogue(y, o, keep, res, mask, relu):
    """[mask] [+ other] [mask] [ReLU] in the order the flags define: RTN_CONV_MASK_PRE masks the convolution before the add."""
    if mask == "pre":
        y = y * keep
    if res:
        y = y + o
    if mask == "post":
        y = y * keep
    return torch.relu(y) if relu else y


class Level(NamedTuple):
    H: int; W: int; Ho: int; Wo: int; pt: int; pl: int
    x: torch.Tensor             # the launch's input (integers; for fp8 the values the e4m3 bytes stand for are x * s_x)
    x2: torch.Tensor            # second source of the dual 1x1 or None
    other: torch.Tensor         # residual tensor (always drawn; read when the case has a residual)
    act: torch.Tensor           # mask tensor (always drawn)
    stage: Stage                # on the pixels the launch writes


class ConvCase(Case):
    """One rtn_conv2d_fwd / rtn_conv1x1_dual_fwd / rtn_conv2d_fp8_fwd / rtn_conv2d_fwd_fp8out launch.
    dtype: "bf16" | "f32" | "fp8" operands; out: None (the operand type; bf16 for fp8) | "f32" | "e4m3".
    res: None | "same" | "up" (a coarser (Ho+1)/2 x ((Wo+1)/2 + 1) level); mask: None | "post" | "pre"; out_step 2: the rows land on
    every second pixel of a (2 Ho - 1) x (2 Wo - 1) grid that `other` and `act` live on; src2 = (channels, step): the dual 1x1."""

    def __init__(self, levels, cin, cout, k, stride=1, pad="same", dtype="bf16", out=None, relu=False, res=None, mask=None, out_step=1,
                 src2=None, concat=False, B=2, seed=0, s_x=1.0, s_w=1.0, out_scale=1.0):
        self.levels_hw, self.cin, self.cout, self.k, self.stride, self.pad, self.dtype, self.B = levels, cin, cout, k, stride, pad, dtype, B
        self.relu, self.res, self.mask, self.out_step, self.src2, self.concat = relu, res, mask, out_step, src2, concat
        self.s_x, self.s_w, self.out_scale = s_x, s_w, out_scale
        self.fmt = out or {"bf16": "bf16", "f32": "f32", "fp8": "bf16"}[dtype]
        g = torch.Generator().manual_seed(seed)
        self.w = ints(g, -2, 2, k, k, cin, cout)
        self.bias = ints(g, -BIAS, BIAS, cout)
        self.w2 = ints(g, -2, 2, src2[0], cout) if src2 else None
        if dtype == "fp8":                                 # the scaled operands must be e4m3 codes
            assert torch.equal(e4m3(self.w * s_w), self.w * s_w) and torch.equal(e4m3(torch.arange(-3.0, 4.0).double() * s_x), torch.arange(-3.0, 4.0).double() * s_x)
        self.levels, self.masks = [], []
        for H, W in levels:
            Ho, Wo, pt, pl = geometry(H, W, k, stride, pad)
            x = ints(g, -3, 3, B, H, W, cin)
            y = ref_conv(x, self.w, self.bias, stride, pt, pl, Ho, Wo)
            bound = ref_conv(x.abs(), self.w.abs(), self.bias.abs(), stride, pt, pl, Ho, Wo)
            x2 = None
            if src2:
                c2, step = src2
                x2 = ints(g, -3, 3, B, (Ho - 1) * step + 1, (Wo - 1) * step + 1, c2)
                y = y + torch.einsum("bhwc,cn->bhwn", x2[:, ::step, ::step], self.w2)
                bound = bound + torch.einsum("bhwc,cn->bhwn", x2[:, ::step, ::step].abs(), self.w2.abs())
            Hg, Wg = (Ho - 1) * out_step + 1, (Wo - 1) * out_step + 1
            other = ints(g, -3, 3, *((B, (Ho + 1) // 2, (Wo + 1) // 2 + 1, cout) if res == "up" else (B, Hg, Wg, cout)))
            act = mask_tensor(g, B, Hg, Wg, cout)
            o = upsample_nearest_legacy(other, Ho, Wo) if res == "up" else other[:, ::out_step, ::out_step]
            pre = epilogue(y, o, act[:, ::out_step, ::out_step] > 0, res, mask, relu)
            if res:
                bound = bound + o.abs()
            if self.fmt == "e4m3":
                pre = torch.clamp(pre * out_scale, -448.0, 448.0)
            self.levels.append(Level(H, W, Ho, Wo, pt, pl, x, x2, other, act, Stage("out %dx%d" % (H, W), pre, bound, relu, self.fmt)))
            if mask:
                self.masks.append(act)
        if concat:                                         # the head outputs are ONE tensor [B][cells of all levels][cout]
            cat = lambda ts: torch.cat([t.reshape(B, -1, cout) for t in ts], 1)
            self.stages = [Stage("out", cat([lv.stage.pre for lv in self.levels]), cat([lv.stage.bound for lv in self.levels]), relu, self.fmt)]
        else:
            self.stages = [lv.stage for lv in self.levels]


class DgradCase(Case):
    """rtn_pack_dgrad_weights + rtn_conv2d_dgrad of the forward layer (H, W, cin -> cout, k, stride, pad): dX = conv-transpose of the
    integer dY in float64, then [mask] [+ other] [mask] and one rounding to bf16.  mode: "res" | "mask" | "res+mask_pre".  The gradient
    has no bias; what brings the sums into the range where bf16 rounds is the accumulated gradient `other` (bf16-representable integers
    of the order of +-600), and for "mask", which reads no other tensor, a bias of that range on the descriptor.
    stride 2: k = 1 scatters with out_step 2 (the pixels off the stride grid keep what the buffer held), k = 3 runs on the
    zero-inserted dY."""

    def __init__(self, H, W, cin, cout, k, stride, pad, mode, B=2, seed=0):
        self.H, self.W, self.cin, self.cout, self.k, self.stride, self.mode, self.B = H, W, cin, cout, k, stride, mode, B
        self.Ho, self.Wo, self.pt, self.pl = geometry(H, W, k, stride, pad)
        g = torch.Generator().manual_seed(seed)
        self.w = ints(g, -2, 2, k, k, cin, cout)
        self.dy = ints(g, -3, 3, B, self.Ho, self.Wo, cout)
        self.other = bf16(ints(g, -BIAS, BIAS, B, H, W, cin))
        self.act = mask_tensor(g, B, H, W, cin)
        self.bias = None if "res" in mode else ints(g, -BIAS, BIAS, cin)
        dx = ref_conv_transpose(self.dy, self.w, stride, self.pt, self.pl, H, W)
        bound = ref_conv_transpose(self.dy.abs(), self.w.abs(), stride, self.pt, self.pl, H, W)
        if self.bias is not None:
            dx, bound = dx + self.bias, bound + self.bias.abs()
        pre = epilogue(dx, self.other, self.act > 0, "res" in mode, "pre" if "pre" in mode else ("post" if "mask" in mode else None), False)
        if "res" in mode:
            bound = bound + self.other.abs()
        self.step = 2 if (stride == 2 and k == 1) else 1
        s = self.step
        self.stages = [Stage("dx", pre[:, ::s, ::s].contiguous(), bound[:, ::s, ::s].contiguous(), False, "bf16")]
        self.masks = [self.act] if "mask" in mode else []


class HeadDgradCase(Case):
    """rtn_pack_dgrad_weights + ONE grouped rtn_conv2d_dgrad of a head-output layer (3x3 'same', cin -> cout) over the pyramid levels:
    the integer dY of every level lies in the concatenated [B][cells of all levels][cp] tensor, cout columns of it and zeros up to
    cp (what rtn_pad_cast_rows leaves there), and the launch runs at Crun = cp.  Modes, bias and `other` as in DgradCase; the levels'
    dX are compared as one tensor [B][cells][cin] (the 1 x 1 level alone is too small for the rounding shares)."""

    def __init__(self, levels, cin, cout, cp, mode, B=2, seed=0):
        self.levels_hw, self.cin, self.cout, self.cp, self.mode, self.B, self.k = levels, cin, cout, cp, mode, B, 3
        g = torch.Generator().manual_seed(seed)
        self.w = ints(g, -2, 2, 3, 3, cin, cout)
        self.bias = None if "res" in mode else ints(g, -BIAS, BIAS, cin)
        self.dy, self.other, self.act, pres, bounds = [], [], [], [], []
        for H, W in levels:
            dy = ints(g, -3, 3, B, H, W, cout)
            other = bf16(ints(g, -BIAS, BIAS, B, H, W, cin))
            act = mask_tensor(g, B, H, W, cin)
            dx = ref_conv_transpose(dy, self.w, 1, 1, 1, H, W)
            bound = ref_conv_transpose(dy.abs(), self.w.abs(), 1, 1, 1, H, W)
            if self.bias is not None:
                dx, bound = dx + self.bias, bound + self.bias.abs()
            pre = epilogue(dx, other, act > 0, "res" in mode, "pre" if "pre" in mode else ("post" if "mask" in mode else None), False)
            if "res" in mode:
                bound = bound + other.abs()
            self.dy.append(dy); self.other.append(other); self.act.append(act)
            pres.append(pre.reshape(B, H * W, cin)); bounds.append(bound.reshape(B, H * W, cin))
        self.stages = [Stage("dx", torch.cat(pres, 1), torch.cat(bounds, 1), False, "bf16")]
        self.masks = list(self.act) if "mask" in mode else []


class BottleneckCase(Case):
    """rtn_bottleneck64_fwd, identity (proj = False) or projection-shortcut form: ReLU-like inputs in [0, 3], 3x3 filters in [-2, 2],
    ternary 1x1 filters; h1, x_out and a_out are rounded to bf16 exactly where the header says (h1 and x_out before they are
    multiplied again)."""

    def __init__(self, B, H, W, proj=False, seed=0):
        self.B, self.H, self.W, self.proj = B, H, W, proj
        g = torch.Generator().manual_seed(seed)
        self.a = ints(g, 0, 3, B, H, W, 64)
        self.x = bf16(ints(g, 0, BIAS // 2, B, H, W, 256))                 # identity shortcut: a ReLU output (bf16-representable)
        self.p = ints(g, 0, 3, B, H, W, 64)                                # projection form: the block input
        self.w2b = ints(g, -2, 2, 64, 3, 3, 64)                            # [out][kh][kw][in]
        self.w2c = ternary(g, 256, 128 if proj else 64)               # projection form: [branch2c | branch1] along K
        self.w2a = ternary(g, 64, 256)
        self.b2b, self.b2c, self.b2a = ints(g, -BIAS, BIAS, 64), ints(g, -BIAS, BIAS, 256), ints(g, -BIAS, BIAS, 64)
        conv = lambda a, w, b: F.conv2d(a.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, padding=1).permute(0, 2, 3, 1)
        h1 = Stage("h1", torch.relu(conv(self.a, self.w2b, self.b2b)), conv(self.a.abs(), self.w2b.abs(), self.b2b.abs()), True, "bf16")
        wc = self.w2c[:, :64]
        pre, bound = h1.want @ wc.T + self.b2c, h1.want.abs() @ wc.abs().T + self.b2c.abs()
        if proj:
            pre, bound = pre + self.p @ self.w2c[:, 64:].T, bound + self.p @ self.w2c[:, 64:].abs().T
        else:
            pre, bound = pre + self.x, bound + self.x
        xo = Stage("x_out", torch.relu(pre), bound, True, "bf16")
        ao = Stage("a_out", torch.relu(xo.want @ self.w2a.T + self.b2a), xo.want @ self.w2a.abs().T + self.b2a.abs(), True, "bf16")
        self.h1, self.x_out, self.a_out = h1, xo, ao
        self.stages, self.masks = [h1, xo, ao], []


class ChainCase(Case):
    """rtn_chain1x1_fwd (128, 512, 128) on `pixels` rows: x_out rounded to bf16 before the second product."""

    def __init__(self, pixels, seed=0):
        self.pixels = pixels
        g = torch.Generator().manual_seed(seed)
        self.h = ints(g, 0, 3, pixels, 128)
        self.x = bf16(ints(g, 0, BIAS // 2, pixels, 512))
        self.w2c, self.w2a = ternary(g, 512, 128), ternary(g, 128, 512)
        self.b2c, self.b2a = ints(g, -BIAS, BIAS, 512), ints(g, -BIAS, BIAS, 128)
        xo = Stage("x_out", torch.relu(self.h @ self.w2c.T + self.b2c + self.x), self.h @ self.w2c.abs().T + self.b2c.abs() + self.x, True, "bf16")
        ao = Stage("a_out", torch.relu(xo.want @ self.w2a.T + self.b2a), xo.want @ self.w2a.abs().T + self.b2a.abs(), True, "bf16")
        self.x_out, self.a_out = xo, ao
        self.stages, self.masks = [xo, ao], []


def pool_tfsame_idx(x):
    """3x3 / 2 TF-'same' max-pool of x (B,H,W,C): (pooled, idx) with idx = kh * 3 + kw of the FIRST maximum in scan order among the
    taps inside the image (the rule maxpool_fwd_idx_kernel documents: TF MaxPoolGrad's choice)."""
    B, H, W, Cc = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    pt, pl = max((Ho - 1) * 2 + 3 - H, 0) // 2, max((Wo - 1) * 2 + 3 - W, 0) // 2
    xp = F.pad(x, (0, 0, pl, 2 * Wo + 2, pt, 2 * Ho + 2), value=float("-inf"))
    best = torch.full((B, Ho, Wo, Cc), float("-inf"), dtype=x.dtype)
    idx = torch.full((B, Ho, Wo, Cc), 255, dtype=torch.uint8)
    for kh in range(3):
        for kw in range(3):
            tap = xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2]
            win = tap > best                               # strictly greater: an equal later tap never replaces the first
            best = torch.where(win, tap, best)
            idx = torch.where(win, torch.full_like(idx, kh * 3 + kw), idx)
    return best, idx


class PoolCase(Case):
    """rtn_maxpool3x3s2_tfsame_fwd_idx on integer ReLU-like values in [0, 3]: almost every window holds its maximum several times."""

    def __init__(self, H, W, Cc=64, B=2, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.x = ints(g, 0, 3, B, H, W, Cc)
        self.pool, self.idx = pool_tfsame_idx(self.x)
        self.stages, self.masks = [], []

    def check(self):
        assert int(self.idx.max()) <= 8 and len(torch.unique(self.idx)) >= 6
        # the tap idx names lies inside the image and holds the maximum, which most windows hold more than once
        B, H, W, Cc = self.x.shape
        Ho, Wo = self.pool.shape[1], self.pool.shape[2]
        pt, pl = max((Ho - 1) * 2 + 3 - H, 0) // 2, max((Wo - 1) * 2 + 3 - W, 0) // 2
        oy, ox = torch.arange(Ho).view(1, -1, 1, 1), torch.arange(Wo).view(1, 1, -1, 1)
        iy, ix = oy * 2 - pt + (self.idx // 3).long(), ox * 2 - pl + (self.idx % 3).long()
        assert bool(((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).all())
        picked = self.x[torch.arange(B).view(-1, 1, 1, 1), iy, ix, torch.arange(Cc).view(1, 1, 1, -1)]
        assert torch.equal(picked, self.pool)
        xp = F.pad(self.x, (0, 0, pl, 2 * Wo + 2, pt, 2 * Ho + 2), value=float("-inf"))
        holders = sum((xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] == self.pool).long() for kh in range(3) for kw in range(3))
        assert float((holders >= 2).double().mean()) > 0.5


class StemCase(Case):
    """The fused stem at kernel level: a bf16 image of integers in [-3, 3], 7x7 / 2 convolution behind ZeroPadding(3) with filters in
    [-2, 2] and a wide bias, ReLU, ONE rounding to bf16, the 3x3 / 2 TF-'same' max-pool with its winning taps, then res2a_branch2a
    (ternary 1x1, bias, ReLU, rounding)."""

    def __init__(self, H, W, B=2, seed=0):
        self.H, self.W, self.B = H, W, B
        g = torch.Generator().manual_seed(seed)
        self.img = ints(g, -3, 3, B, H, W, 3)
        self.w = ints(g, -2, 2, 7, 7, 3, 64)                               # HWIO, as a checkpoint holds it
        self.bias = ints(g, -BIAS, BIAS, 64)
        self.w2a = ints(g, -1, 1, 1, 1, 64, 64)                            # HWIO
        self.b2a = ints(g, -BIAS, BIAS, 64)
        H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        c1 = Stage("conv1", torch.relu(ref_conv(self.img, self.w, self.bias, 2, 3, 3, H1, W1)),
                   ref_conv(self.img.abs(), self.w.abs(), self.bias.abs(), 2, 3, 3, H1, W1), True, "bf16")
        self.pool1, self.pool_idx = pool_tfsame_idx(c1.want)
        wa = self.w2a[0, 0]                                                # [in][out]
        ao = Stage("a_out", torch.relu(self.pool1 @ wa + self.b2a), self.pool1 @ wa.abs() + self.b2a.abs(), True, "bf16")
        self.conv1, self.a_out = c1, ao
        self.stages, self.masks = [c1, ao], []

    def check(self):
        super().check()
        nz = float((self.pool1 != 0).double().mean())
        assert 0.2 <= nz <= 0.8, "pool1: %.1f %% non-zero" % (100 * nz)
        assert len(torch.unique(self.pool_idx)) >= 6                       # ties and borders spread the winners over the taps


# ------------------------------------------------------------------------------------------------ the register-epilogue forms
EPI_MODES = ["none", "res", "mask", "mask_pre", "res+mask", "res+mask_pre"]
EPI_FORMS = {
    # name: (impl, k, cin, cout, levels, form)
    "h8": (4, 3, 64, 136, LEVELS2, None),                  # generation 4 full width: 264 + 12 rows = two tiles at both tile heights, a group
                                                           # boundary inside the second; columns 136..255 of the tile are never stored
    "h8-128": (4, 3, 64, 72, LEVELS2, None),               # ... its 128-column instance (8-byte accesses)
    "g8": (5, 1, 128, 256, [(11, 13)], None),              # generation 5 full width: 286 rows = 3 / 2 tiles, the last one part full
    "g8-128": (5, 1, 128, 128, [(11, 13)], None),          # ... its narrow instance
    "h8-kslice": (4, 3, 64, 136, [(12, 11)], "kslice"),    # generation 4, three K slices (one kernel row each) through the f32 slabs
    "g8-scatter": (5, 1, 128, 256, [(5, 4)], "scatter"),   # generation 5: rows land on every second pixel of a 9 x 7 grid (out_step 2)
    "g8-up": (5, 1, 128, 256, [(7, 9)], "up"),             # ... residual = the coarser level (4 x 5: ratios 0.571 / 0.556)
    "g8-sk": (5, 1, 128, 256, [(11, 13)], "sk"),           # ... stream-K: two K steps per tile, tiles cut between workgroups
}


@functools.lru_cache(maxsize=None)
def epi_exact_operands(form):
    """Small-integer operands of one EPI_FORMS entry and the float64 convolution + bias of every level, computed once per form:
    inputs and `other` in [-3, 3], filters in [-2, 2], bias in [-600, 600] - every partial sum is an integer below 2^24, exact in f32
    in any order, so the only rounding on the device is the final one to bf16, and the wide bias makes that rounding matter: more
    than 5 % of the outputs are not representable before it (tests/test_conv_exact_cases.py asserts it for every mode)."""
    impl, k, cin, cout, levels, kind = EPI_FORMS[form]
    g = torch.Generator().manual_seed(4000 + sorted(EPI_FORMS).index(form))
    w = ints(g, -2, 2, k, k, cin, cout)
    bias = ints(g, -BIAS, BIAS, cout)
    B, lv = 2, []
    for H, W in levels:
        x = ints(g, -3, 3, B, H, W, cin)
        Hg, Wg = (2 * H - 1, 2 * W - 1) if kind == "scatter" else (H, W)         # the grid `out`, `other` and `act` live on
        other = ints(g, -3, 3, *((B, (H + 1) // 2, (W + 1) // 2, cout) if kind == "up" else (B, Hg, Wg, cout)))
        act = mask_tensor(g, B, Hg, Wg, cout)
        pad = (k - 1) // 2
        lv.append((x, other, act, ref_conv(x, w, bias, 1, pad, pad, H, W), ref_conv(x.abs(), w.abs(), bias.abs(), 1, pad, pad, H, W)))
    return w, bias, lv


def epi_stages(form, mode, relu):
    """[(step, Stage)] per level of one EPI_FORMS entry in one epilogue mode: the float64 reference on the written pixels,
    [mask] [+ other] [mask], ReLU, one rounding to bf16."""
    impl, k, cin, cout, levels, kind = EPI_FORMS[form]
    w, bias, lv = epi_exact_operands(form)
    step = 2 if kind == "scatter" else 1
    out = []
    for (H, W), (x, other, act, y, bound) in zip(levels, lv):
        o = upsample_nearest_legacy(other, H, W) if kind == "up" else other[:, ::step, ::step]
        pre = epilogue(y, o, act[:, ::step, ::step] > 0, "res" in mode, "pre" if "pre" in mode else ("post" if "mask" in mode else None), bool(relu))
        out.append((step, Stage("%s %s relu=%d %dx%d" % (form, mode, relu, H, W), pre, bound + (o.abs() if "res" in mode else 0), bool(relu), "bf16")))
    return out


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_conv_exact.py
def _fwd(**kw):
    return functools.partial(ConvCase, **kw)


CASES = {}


def _add(name, factory):
    assert name not in CASES, name
    CASES[name] = factory


for _dt in ("bf16", "f32"):
    for _relu in (0, 1):
        for _res in (None, "same", "up"):
            # 36 K chunks, two tiles, a group boundary inside the second tile, N not a tile multiple
            _add("gen123/3x3/%s/relu%d/res-%s" % (_dt, _relu, _res),
                 _fwd(levels=LEVELS2, cin=256, cout=136, k=3, dtype=_dt, relu=bool(_relu), res=_res, seed=11))
        _add("gen123/1x1s2/%s/relu%d" % (_dt, _relu), _fwd(levels=[(9, 13)], cin=256, cout=128, k=1, stride=2, pad=0, dtype=_dt, relu=bool(_relu), seed=12))
        _add("gen123/3x3s2/%s/relu%d" % (_dt, _relu), _fwd(levels=[(9, 12)], cin=128, cout=64, k=3, stride=2, dtype=_dt, relu=bool(_relu), seed=13))
        # tail split: 5 row tiles x 4 column tiles of 64 = 20 tiles on 18 slots; 7 x 3 = 21 tiles on 19 slots; split-K: 32 K steps
        _add("tail/3x3/%s/relu%d" % (_dt, _relu), _fwd(levels=[(20, 21)], cin=256, cout=256, k=3, dtype=_dt, relu=bool(_relu), B=3, seed=21))
        _add("tail/1x1res/%s/relu%d" % (_dt, _relu), _fwd(levels=[(31, 28)], cin=512, cout=192, k=1, pad=0, dtype=_dt, relu=bool(_relu), res="same", seed=22))
        _add("splitk/1x1/%s/relu%d" % (_dt, _relu), _fwd(levels=[(6, 7)], cin=2048, cout=64, k=1, pad=0, dtype=_dt, relu=bool(_relu), seed=23))
for _relu in (0, 1):
    for _cin, _cout in ((256, 136), (128, 72)):
        for _mode, _kw in (("none", {}), ("res", {"res": "same"}), ("res+mask_pre", {"res": "same", "mask": "pre"})):
            _add("gen4/%d-%d/%s/relu%d" % (_cin, _cout, _mode, _relu), _fwd(levels=LEVELS2, cin=_cin, cout=_cout, k=3, relu=bool(_relu), seed=31, **_kw))
    _add("gen4/kslice/relu%d" % _relu, _fwd(levels=[(12, 11)], cin=256, cout=136, k=3, relu=bool(_relu), seed=32))
    for _cout in (256, 128):
        _add("gen5/512-%d/relu%d" % (_cout, _relu), _fwd(levels=[(11, 13)], cin=512, cout=_cout, k=1, pad=0, relu=bool(_relu), seed=41))
        _add("gen5/512-%d/s2/relu%d" % (_cout, _relu), _fwd(levels=[(9, 13)], cin=512, cout=_cout, k=1, stride=2, pad=0, relu=bool(_relu), seed=42))
        _add("gen5/512-%d/up/relu%d" % (_cout, _relu), _fwd(levels=[(11, 13)], cin=512, cout=_cout, k=1, pad=0, relu=bool(_relu), res="up", seed=43))
        _add("gen5/512-%d/scatter/relu%d" % (_cout, _relu),
             _fwd(levels=[(6, 7)], cin=512, cout=_cout, k=1, pad=0, relu=bool(_relu), res="same", mask="post", out_step=2, seed=44))
    _add("dual/step1/relu%d" % _relu, _fwd(levels=[(7, 9)], cin=128, cout=512, k=1, pad=0, relu=bool(_relu), src2=(256, 1), seed=51))
    _add("dual/step2/relu%d" % _relu, _fwd(levels=[(7, 9)], cin=128, cout=512, k=1, pad=0, relu=bool(_relu), src2=(256, 2), seed=52))     # source 2 at 13 x 17
    for _cin in (128, 256):
        for _cout in (64, 256):
            for _out in ("bf16", "e4m3"):
                _add("fp8/%d-%d/%s/relu%d" % (_cin, _cout, _out, _relu),
                     _fwd(levels=LEVELS2, cin=_cin, cout=_cout, k=3, dtype="fp8", out=_out, relu=bool(_relu), seed=111, s_x=4.0, s_w=8.0, out_scale=0.25))
    _add("fp8out/1x1/relu%d" % _relu, _fwd(levels=[(11, 13)], cin=512, cout=128, k=1, pad=0, out="e4m3", relu=bool(_relu), seed=112, out_scale=0.25))
    _add("fp8out/1x1s2/relu%d" % _relu, _fwd(levels=[(9, 13)], cin=256, cout=128, k=1, stride=2, pad=0, out="e4m3", relu=bool(_relu), seed=113, out_scale=0.25))
    _add("fp8out/3x3/relu%d" % _relu, _fwd(levels=LEVELS2, cin=256, cout=136, k=3, out="e4m3", relu=bool(_relu), seed=114, out_scale=0.25))
for _out in ("f32", "bf16"):
    _add("head/%s" % _out, _fwd(levels=HEAD_LEVELS, cin=256, cout=36, k=3, out=_out, concat=True, seed=61))
HEAD_COUTS = (27, 54, 72, 180, 270)       # K * 9 anchors for K = 3, 6, 8, 20, 30: up to 48 (generation 6), one 64 / 128 / 256 tile, two N tiles
for _cout in HEAD_COUTS:
    for _out in ("f32", "bf16"):
        _add("head%d/%s" % (_cout, _out), _fwd(levels=HEAD_LEVELS, cin=256, cout=_cout, k=3, out=_out, concat=True, seed=62))
# the head outputs' data gradient: the forward layer is 3x3 256 -> cout, dY lies in the concatenated tensor padded to cp columns
HEAD_DGRAD = ((54, 64), (72, 128), (180, 256), (270, 512))
for _mode in ("res", "mask", "res+mask_pre"):
    _add("dgrad/3x3-64-256/%s" % _mode, functools.partial(DgradCase, 9, 13, 64, 256, 3, 1, "same", _mode, seed=71))
    _add("dgrad/3x3-256-64/%s" % _mode, functools.partial(DgradCase, 9, 13, 256, 64, 3, 1, "same", _mode, seed=72))
    _add("dgrad/1x1s2/%s" % _mode, functools.partial(DgradCase, 9, 13, 256, 128, 1, 2, 0, _mode, seed=73))
    _add("dgrad/1x1s2-even/%s" % _mode, functools.partial(DgradCase, 10, 14, 256, 128, 1, 2, 0, _mode, seed=74))
    _add("dgrad/3x3s2/%s" % _mode, functools.partial(DgradCase, 9, 13, 256, 128, 3, 2, "same", _mode, seed=75))        # 2 Ho - 1 = H: every generation
    _add("dgrad/3x3s2-even/%s" % _mode, functools.partial(DgradCase, 10, 12, 256, 128, 3, 2, "same", _mode, seed=76))  # asymmetric pad
    for _cout, _cp in HEAD_DGRAD:
        _add("dgrad/head%d-%d/%s" % (_cout, _cp, _mode), functools.partial(HeadDgradCase, HEAD_LEVELS, 256, _cout, _cp, _mode, seed=77))
for _proj in (False, True):
    for _shape in ((2, 9, 13), (1, 1, 1), (3, 5, 4), (2, 41, 67)):
        _add("bneck/%s/%dx%dx%d" % ("proj" if _proj else "id", *_shape), functools.partial(BottleneckCase, *_shape, proj=_proj, seed=81))
_add("bneck/id/2x10x14", functools.partial(BottleneckCase, 2, 10, 14, seed=81))                  # the quarter forms' even extent
for _px in (1, 37, 2049):
    _add("chain/%d" % _px, functools.partial(ChainCase, _px, seed=91))
for _hw in ((33, 35), (64, 96), (67, 101)):
    _add("stem/%dx%d" % _hw, functools.partial(StemCase, *_hw, seed=101))
for _hw in ((17, 23), (16, 22)):
    _add("pool/%dx%d" % _hw, functools.partial(PoolCase, *_hw, seed=102))


@functools.lru_cache(maxsize=None)
def case(name):
    """The case `name`, built once per process (operands and reference are read-only)."""
    c = CASES[name]()
    c.name = name
    return c
