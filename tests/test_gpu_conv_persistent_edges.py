"""GPU: the edges of the three persistent conv launchers (generations 4 / 5 / 6: csrc/rtn_conv_persistent.h, rtn_conv_halo8.hip,
rtn_conv_gemm8.hip, rtn_conv_halon.hip) against a census recorded with the library of the commit BEFORE those launchers were split
into takes / choose / fill / launch.  tests/test_gpu_conv_dispatch.py holds valid Engine layers only, so it never reaches the lines
that answer "not mine"; here every base layer is a small valid layer one of the three generations takes, and every entry changes ONE
thing about it - a flag, N, a leading dimension, a stride, a pointer by 8 bytes, an element count by one, the workspace, a knob - so
that the launcher has to decline it, or take it on another path.

The record of one entry is [return code, rtn_debug_last_conv_impl, rtn_debug_last_conv_tile, rtn_debug_last_conv_streamk, the
*_workspace_bytes answer] (the three debug values -1 unless the launch returned RTN_OK, as in the dispatch test) and, for a negative
return code, the text of rtn_last_error.  Where the launch returned RTN_OK - whichever generation ended up running it - the output
must EQUAL the float64 reference of that (possibly changed) layer rounded once, and nothing else in the output buffer may have been
written: operands are the small integers of tests/conv_exact.py, so there is no tolerance.  The one exception is the sigmoid of two
head-output bases: exp is not exact (tests/conv_exact.py keeps the sigmoid head out for that reason), so those outputs are compared
with the f32 sigmoid of the exact sum within 1e-6 - four ulps of 1.0 for the expf, the add, the division and the reference's own
rounding; the results lie in [0, 1].

The fixture (tests/golden/conv_persistent_edges.json) depends on the CU count: it carries num_cus and the test skips on a device that
reports another.  `python tests/test_gpu_conv_persistent_edges.py` rewrites it from whatever library RTN_LIB_PATH names; it is
committed as the parent's library wrote it."""
import ctypes as C
import functools
import importlib
import json
import os
import sys
from typing import NamedTuple

import pytest
import torch

import conv_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_persistent_edges.json")
PKG = "retinanet-for-table-detection_amd"
pytestmark = pytest.mark.gpu
DEV = "cuda"
SLACK = 64                       # elements in front of and behind every tensor: a pointer moved by 8 bytes stays inside its allocation
FILL = -77.0
B = 2
ONE = ((12, 11),)                # single-group layers
KNOBS = ["RTN_CONV_IMPL", "RTN_CONV_H8_GRID", "RTN_CONV_H8_KSPLIT", "RTN_CONV_G8_SK", "RTN_CONV_G8_NARROW", "RTN_CONV_H8_MI",
         "RTN_CONV_G8_MI", "RTN_CONV_H8_STAGGER", "RTN_CONV_H8_HALF", "RTN_CONV_G8_N128", "RTN_CONV_H8", "RTN_CONV_G8", "RTN_CONV_HN"]


class Spec(NamedTuple):
    """A layer: what it computes (first line of fields) and how its tensors lie in memory (second line)."""
    levels: tuple; cin: int; N: int; k: int; dtype: str = "bf16"; relu: bool = False; sigmoid: bool = False; res: str = None
    mask: str = None; out_f32: bool = False; src2: tuple = None; out_step: int = 1; pad_t: int = None; pad_l: int = None; seed: int = 0
    concat: bool = False; out_ld_pad: int = 0; pix_pad: int = 0; in_img_pad: int = 0; out_img_pad: int = 0; out_off: int = 0
    res_ld_pad: int = 0; res_img_pad: int = 0


# ------------------------------------------------------------------------------------------------ bases
def bases():
    """{name: (Spec, environment, entry point)}"""
    out = {}
    h8 = {"RTN_CONV_IMPL": "4"}
    for n in (256, 128, 512):
        out["h8/n%d" % n] = (Spec(tuple(X.LEVELS2), 64, n, 3, relu=True, seed=1), h8, "fwd")
    out["h8/n256-res-maskpre"] = (Spec(tuple(X.LEVELS2), 64, 256, 3, res="same", mask="pre", seed=2), h8, "fwd")
    out["h8/fp8-n256"] = (Spec(tuple(X.LEVELS2), 128, 256, 3, dtype="fp8", relu=True, seed=3), h8, "fp8")
    out["h8/c128-kslice2"] = (Spec(ONE, 128, 256, 3, relu=True, seed=4), dict(h8, RTN_CONV_H8_KSPLIT="2"), "fwd")
    for n in (36, 4):
        for sig in (False, True):
            out["hn/n%d%s" % (n, "-sigmoid" if sig else "")] = (Spec(tuple(X.HEAD_LEVELS), 64, n, 3, out_f32=True, sigmoid=sig, concat=True, seed=5),
                                                               {"RTN_CONV_IMPL": "6"}, "fwd")
    for sk in ("0", "1"):
        g8 = {"RTN_CONV_IMPL": "5", "RTN_CONV_G8_SK": sk}
        out["g8/n256/sk" + sk] = (Spec(ONE, 64, 256, 1, seed=6), g8, "fwd")
        out["g8/n256-relu-res/sk" + sk] = (Spec(ONE, 64, 256, 1, relu=True, res="same", seed=7), g8, "fwd")
        for narrow in ("0", "1"):
            out["g8/n128-narrow%s/sk%s" % (narrow, sk)] = (Spec(ONE, 64, 128, 1, relu=True, seed=8), dict(g8, RTN_CONV_G8_NARROW=narrow), "fwd")
        out["g8/dual/sk" + sk] = (Spec(ONE, 64, 256, 1, relu=True, src2=(64, 2), seed=9), g8, "dual")
        out["g8/scatter/sk" + sk] = (Spec(ONE, 64, 256, 1, res="same", mask="post", out_step=2, seed=10), g8, "fwd")
        out["g8/up/sk" + sk] = (Spec(ONE, 64, 256, 1, relu=True, res="up", seed=11), g8, "fwd")
    return out


# ------------------------------------------------------------------------------------------------ operands and reference (CPU, once per Spec)
def geometry(s, H, W):
    pad = (s.k - 1) // 2
    return H, W, (pad if s.pad_t is None else s.pad_t), (pad if s.pad_l is None else s.pad_l)


@functools.lru_cache(maxsize=None)
def operands(s):
    """Integer operands as in conv_exact.ConvCase and, per level, the exact result (B, cells, N) in front of the final rounding."""
    g = torch.Generator().manual_seed(7000 + s.seed)
    N = max(s.N, 1)                                        # (N = 0 never launches: the tensors only have to exist)
    w, bias = X.ints(g, -2, 2, s.k, s.k, s.cin, N), X.ints(g, -X.BIAS, X.BIAS, N)
    w2 = X.ints(g, -2, 2, s.src2[0], N) if s.src2 else None
    levels = []
    for H, W in s.levels:
        Ho, Wo, pt, pl = geometry(s, H, W)
        x = X.ints(g, -3, 3, B, H, W, s.cin)
        y = X.ref_conv(x, w, bias, 1, pt, pl, Ho, Wo)
        x2 = None
        if s.src2:
            c2, step = s.src2
            x2 = X.ints(g, -3, 3, B, (Ho - 1) * step + 1, (Wo - 1) * step + 1, c2)
            y = y + torch.einsum("bhwc,cn->bhwn", x2[:, ::step, ::step], w2)
        Hg, Wg = (Ho - 1) * s.out_step + 1, (Wo - 1) * s.out_step + 1
        other = X.ints(g, -3, 3, *((B, (Ho + 1) // 2, (Wo + 1) // 2 + 1, N) if s.res == "up" else (B, Hg, Wg, N)))
        act = X.mask_tensor(g, B, Hg, Wg, N) if s.mask else None
        o = X.upsample_nearest_legacy(other, Ho, Wo) if s.res == "up" else other[:, ::s.out_step, ::s.out_step]
        pre = X.epilogue(y, o, act[:, ::s.out_step, ::s.out_step] > 0 if s.mask else None, s.res, s.mask, s.relu)
        levels.append((x, x2, other, act, pre.reshape(B, Ho * Wo, N), (Hg, Wg)))
    return w, bias, w2, levels


def wanted(s, pre):
    if s.sigmoid:
        return torch.sigmoid(pre).float().double()
    return pre if s.out_f32 else X.bf16(pre)


# ------------------------------------------------------------------------------------------------ device tensors (once per Spec)
class Buf:
    """A device tensor with SLACK elements of fill in front of and behind the part the descriptor names."""

    def __init__(self, flat, fill=5.0):
        self.raw = torch.full((flat.numel() + 2 * SLACK,), fill, dtype=flat.dtype)
        self.raw[SLACK:SLACK + flat.numel()] = flat
        self.raw = self.raw.to(DEV)
        self.elems = flat.numel()
        self.ptr = self.raw.data_ptr() + SLACK * flat.element_size()


def laid_out(t, ld, img_stride, dtype, scale=1.0):
    """t (B, H, W, C) -> flat [B][img_stride] with rows of `ld` elements per pixel; the gaps hold 5."""
    Bn, H, W, Cn = t.shape
    assert img_stride >= H * W * ld
    img = torch.full((Bn, H * W, ld), 5.0, dtype=torch.float64)
    img[:, :, :Cn] = t.reshape(Bn, H * W, Cn)
    flat = torch.full((Bn, img_stride), 5.0, dtype=torch.float64)
    flat[:, :H * W * ld] = img.reshape(Bn, -1)
    flat = flat.reshape(-1)
    if dtype == "fp8":
        return X.e4m3_bytes(flat * scale)
    return flat.to(torch.bfloat16)


class Layer:
    """Device tensors of a Spec and the descriptor that names them exactly (every *_elems is what the layer needs, no more)."""

    def __init__(self, L, s):
        self.s, self.L = s, L
        w, bias, w2, levels = operands(s)
        N = max(s.N, 1)
        wk = w.permute(3, 0, 1, 2).reshape(N, -1)
        if s.src2:
            wk = torch.cat([wk, w2.T], 1)
        self.rows = rows = -(-N // 128) * 128
        wfull = torch.zeros(rows, wk.shape[1], dtype=torch.float64)
        wfull[:N] = wk
        self.w = Buf(X.e4m3_bytes(wfull * 8.0).reshape(-1) if s.dtype == "fp8" else wfull.to(torch.bfloat16).reshape(-1))
        bd = torch.zeros(rows, dtype=torch.float32)
        bd[:N] = bias.float()
        self.bias = Buf(bd)
        self.odt = torch.float32 if s.out_f32 else torch.bfloat16
        self.ld = ld = s.N + s.out_ld_pad
        self.pix = s.cin + s.pix_pad
        self.groups = []
        total = sum(H * W for H, W in s.levels)
        if s.concat:                                       # head-output style: every level into one [B][total][ld] tensor
            self.out_img = total * ld + s.out_img_pad
            self.out = Buf(torch.full(((B - 1) * self.out_img + s.out_off + max(total - 1, 0) * ld + s.N,), FILL, dtype=self.odt), fill=FILL)
        row0 = 0
        for (H, W), (x, x2, other, act, pre, (Hg, Wg)) in zip(s.levels, levels):
            Ho, Wo, pt, pl = geometry(s, H, W)
            g = {"H": H, "W": W, "Hg": Hg, "Wg": Wg, "pt": pt, "pl": pl, "pre": pre}
            g["in_img"] = H * W * self.pix + s.in_img_pad
            g["x"] = Buf(laid_out(x, self.pix, g["in_img"], s.dtype, 4.0)[:(B - 1) * g["in_img"] + H * W * self.pix])
            if s.concat:
                g["out"], g["out_img"], g["off"] = self.out, self.out_img, row0 * ld + s.out_off
            else:
                g["out_img"], g["off"] = Hg * Wg * ld + s.out_img_pad, s.out_off
                g["out"] = Buf(torch.full(((B - 1) * g["out_img"] + s.out_off + ((Hg - 1) * Wg + Wg - 1) * ld + s.N,), FILL, dtype=self.odt), fill=FILL)
            row0 += H * W
            if s.res:
                g["res_ld"] = N + s.res_ld_pad
                g["res_img"] = other.shape[1] * other.shape[2] * g["res_ld"] + s.res_img_pad
                flat = laid_out(other, g["res_ld"], g["res_img"], "bf16")
                g["res"] = Buf(flat[:(B - 1) * g["res_img"] + (other.shape[1] * other.shape[2] - 1) * g["res_ld"] + N])
                g["Hres"], g["Wres"] = other.shape[1], other.shape[2]
            if s.mask:
                g["mask"] = Buf(laid_out(act, N, Hg * Wg * N, "bf16"))
            if s.src2:
                g["x2"] = Buf(laid_out(x2, s.src2[0], x2.shape[1] * x2.shape[2] * s.src2[0], "bf16"))
                g["H2"], g["W2"] = x2.shape[1], x2.shape[2]
            self.groups.append(g)

    def descriptor(self):
        L, s = self.L, self.s
        d = L.ConvDesc()
        d.ngroups, d.batch, d.dtype = len(self.groups), B, L.RTN_FP8 if s.dtype == "fp8" else L.RTN_BF16
        d.w, d.bias, d.w_rows, d.N, d.KH, d.KW = self.w.ptr, self.bias.ptr, self.rows, s.N, s.k, s.k
        d.Crun, d.pix_stride = s.cin, self.pix
        d.sy = d.sx = 1
        d.out_ld = self.ld
        d.flags = (L.CONV_RELU if s.relu else 0) | (L.CONV_SIGMOID if s.sigmoid else 0) | (L.CONV_OUT_F32 if s.out_f32 else 0) | \
            {None: 0, "same": L.CONV_RES_SAME, "up": L.CONV_RES_UPSAMPLE}[s.res] | \
            {None: 0, "post": L.CONV_RELU_MASK, "pre": L.CONV_RELU_MASK | L.CONV_MASK_PRE}[s.mask]
        s2 = None
        for gi, g in enumerate(self.groups):
            grp = L.ConvGroup()
            grp.in_, grp.in_elems, grp.in_img_stride, grp.in_row_stride = g["x"].ptr, g["x"].elems, g["in_img"], g["W"] * self.pix
            grp.Hin, grp.Win, grp.Hout, grp.Wout = g["H"], g["W"], g["H"], g["W"]
            d.pad_t, d.pad_l = g["pt"], g["pl"]
            grp.out, grp.out_elems, grp.out_img_stride, grp.out_off = g["out"].ptr, g["out"].elems, g["out_img"], g["off"]
            if s.out_step > 1:
                grp.out_step, grp.out_pix_w = s.out_step, g["Wg"]
            if s.res:
                grp.res, grp.res_elems, grp.res_img_stride, grp.res_ld = g["res"].ptr, g["res"].elems, g["res_img"], g["res_ld"]
                grp.Hres, grp.Wres = g["Hres"], g["Wres"]
            if s.mask:
                grp.mask, grp.mask_elems, grp.mask_img_stride, grp.mask_ld = g["mask"].ptr, g["mask"].elems, g["Hg"] * g["Wg"] * max(s.N, 1), max(s.N, 1)
            if s.src2:
                c2, step = s.src2
                s2 = L.ConvSrc2()
                s2.in_, s2.in_elems, s2.in_img_stride, s2.in_row_stride, s2.pix_stride = g["x2"].ptr, g["x2"].elems, g["H2"] * g["W2"] * c2, g["W2"] * c2, c2
                s2.Hin, s2.Win, s2.C, s2.step = g["H2"], g["W2"], c2, step
            d.g[gi] = grp
        return d, s2

    def refill(self):
        for g in self.groups:
            g["out"].raw.fill_(FILL)

    def check_output(self, d, what):
        """Every level at the place the descriptor `d` names equals the reference; every other element of the buffers kept the fill."""
        s = self.s
        written = {}
        for gi, g in enumerate(self.groups):
            grp = d.g[gi]
            raw = g["out"].raw
            start = (grp.out - raw.data_ptr()) // raw.element_size()
            H, W = g["H"], g["W"]
            oy, ox = torch.arange(H).view(-1, 1), torch.arange(W).view(1, -1)
            pix = (oy * s.out_step * g["Wg"] + ox * s.out_step).reshape(-1) if s.out_step > 1 else torch.arange(H * W)
            idx = start + (torch.arange(B).view(-1, 1, 1) * grp.out_img_stride + grp.out_off + pix.view(1, -1, 1) * d.out_ld + torch.arange(s.N).view(1, 1, -1))
            host = raw.cpu()
            got, want = host[idx].double(), wanted(s, g["pre"][:, :, :s.N])
            if s.sigmoid:
                err = float((got - want).abs().max())
                assert err <= 1e-6, "%s level %dx%d: sigmoid output off by %.3g" % (what, H, W, err)
            else:
                assert torch.equal(got, want), "%s level %dx%d: %d of %d elements differ from the float64 reference rounded once" % (
                    what, H, W, int((got != want).sum()), got.numel())
            m = written.setdefault(id(raw), (host, torch.zeros(raw.numel(), dtype=torch.bool)))[1]
            m[idx.reshape(-1)] = True
        for host, m in written.values():
            assert bool((host[~m] == FILL).all()), "%s: %d elements outside the levels were written" % (what, int((host[~m] != FILL).sum()))


# ------------------------------------------------------------------------------------------------ mutations
def _gen(env):
    return int(env["RTN_CONV_IMPL"])


def _each_group(d, n, fn):
    for i in range(n):
        g = d.g[i]
        fn(g)
        d.g[i] = g


def _bump(field, by=8):
    def f(g):
        setattr(g, field, (getattr(g, field) or 0) + by)
    return f


def mutations(s, env):
    """[(name, kind, argument)] that apply to the base (s, env).  kind "spec": argument = the changed Spec (another layer, with its
    own reference); "desc": argument(d, s2) changes the descriptor of the base (the reference stays: whatever runs it must still compute
    the base layer, reading the output where the descriptor now says); "ws": argument in ("null", "off8", "short") changes the
    workspace after it was sized and attached; "env": argument = the environment to launch under."""
    gen, ng = _gen(env), len(s.levels)
    m = [("base", "desc", lambda d, s2: None)]
    # a flag outside the launcher's set: generations 4 / 5 have no f32 store, generation 6 no residual
    if gen == 6:
        m.append(("flag-res-same", "desc", lambda d, s2: setattr(d, "flags", d.flags | 0x04)))
    else:
        m.append(("flag-out-f32", "spec", s._replace(out_f32=True)))
    if not s.mask:
        m.append(("mask-pre-alone", "desc", lambda d, s2: setattr(d, "flags", d.flags | 0x40)))
    # N one below and one above each N range, and N % 8 != 0
    if gen == 4:
        ns = (128, 264) if s.dtype == "fp8" else (64, 2056)
    elif gen == 6:
        ns = (0, 49)
    else:
        ns = (120, 136) if s.N == 128 else (248, 2304)
    for n in ns + ((s.N + 4,) if gen != 6 else ()):
        m.append(("N=%d" % n, "spec", s._replace(N=n)))
    m.append(("out_ld+4", "spec", s._replace(out_ld_pad=4)))
    m.append(("pix_stride+64", "spec", s._replace(pix_pad=64)))
    m.append(("pad_l=KW", "spec", s._replace(pad_l=s.k)))
    m.append(("pad_t=KH", "spec", s._replace(pad_t=s.k)))
    # pointers by 8 bytes, element counts one short
    for f in ("in_", "out") + (("res",) if s.res else ()) + (("mask",) if s.mask else ()):
        m.append((f.strip("_") + "+8B", "desc", lambda d, s2, f=f: _each_group(d, ng, _bump(f))))
        m.append((f.strip("_") + "_elems-1", "desc", lambda d, s2, f=f.strip("_") + "_elems": _each_group(d, ng, _bump(f, -1))))
    m.append(("w+8B", "desc", lambda d, s2: setattr(d, "w", d.w + 8)))
    m.append(("bias+8B", "desc", lambda d, s2: setattr(d, "bias", d.bias + 8)))
    if s.src2:
        m.append(("src2+8B", "desc", lambda d, s2: setattr(s2, "in_", s2.in_ + 8)))
        m.append(("src2_elems-1", "desc", lambda d, s2: setattr(s2, "in_elems", s2.in_elems - 1)))
        m.append(("src2-step-leaves", "desc", lambda d, s2: setattr(s2, "step", s2.step + 1)))
    m.append(("out_off=8", "spec", s._replace(out_off=8)))
    m.append(("in_img_stride-padded", "spec", s._replace(in_img_pad=s.levels[0][1] * s.cin)))
    m.append(("out_img_stride-padded", "spec", s._replace(out_img_pad=3 * s.N)))
    if s.res:
        m.append(("res_ld+4", "spec", s._replace(res_ld_pad=4)))
        m.append(("res_img_stride-padded", "spec", s._replace(res_img_pad=2 * s.N)))
    m += [("ws-" + k, "ws", k) for k in ("null", "off8", "short")]          # (dropped by the census where the base asks for no workspace)
    m.append(("H8_GRID=3", "env", dict(env, RTN_CONV_H8_GRID="3")))
    m.append(("unforced", "env", {k: v for k, v in env.items() if k != "RTN_CONV_IMPL"}))
    return m


# ------------------------------------------------------------------------------------------------ the census
def run_entry(L, h, layer, entry, env, desc_fn, ws_kind, what):
    lib = L.lib
    d, s2 = layer.descriptor()
    desc_fn(d, s2)
    os.environ.update(env)
    try:
        if entry == "dual":
            ws = int(lib.rtn_conv1x1_dual_workspace_bytes(h.raw, C.byref(d), C.byref(s2)))
        else:
            ws = int(lib.rtn_conv2d_workspace_bytes(h.raw, C.byref(d)))                    # (an fp8 descriptor has no scratch: 0)
        if ws_kind and ws == 0:
            return None
        if ws > 0:
            t = torch.empty(ws + 16, dtype=torch.uint8, device=DEV)
            h.check(lib.rtn_conv_workspace_init(h.raw, t.data_ptr(), ws))
            d.workspace, d.workspace_bytes = t.data_ptr(), ws
            if ws_kind == "null":
                d.workspace, d.workspace_bytes = None, 0
            elif ws_kind == "off8":
                d.workspace = t.data_ptr() + 8
            elif ws_kind == "short":
                d.workspace_bytes = ws - 1
        layer.refill()
        if entry == "dual":
            rc = lib.rtn_conv1x1_dual_fwd(h.raw, C.byref(d), C.byref(s2))
        elif entry == "fp8":
            q = L.ConvFp8(acc_scale=1.0 / 32.0, out_scale=1.0, out_dtype=L.RTN_BF16)      # operands scaled by 4 and 8: e4m3 codes
            rc = lib.rtn_conv2d_fp8_fwd(h.raw, C.byref(d), C.byref(q))
        else:
            rc = lib.rtn_conv2d_fwd(h.raw, C.byref(d))
        torch.cuda.synchronize()
    finally:
        for k in env:
            del os.environ[k]
    if rc != 0:
        rec = [int(rc), -1, -1, -1, ws]
        return rec + [lib.rtn_last_error(h.raw).decode("utf-8", "replace")] if rc < 0 else rec
    layer.check_output(d, what)
    return [0, int(lib.rtn_debug_last_conv_impl(h.raw)), int(lib.rtn_debug_last_conv_tile(h.raw)), int(lib.rtn_debug_last_conv_streamk(h.raw)), ws]


def census(L, h, failures=None):
    """`failures`: a list that collects the output mismatches instead of the first one being raised (the recording run prints them all)."""
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    layers, records = {}, {}

    def layer_of(s):
        if s not in layers:
            layers[s] = Layer(L, s)
        return layers[s]

    try:
        for name, (s, env, entry) in bases().items():
            for mname, kind, arg in mutations(s, env):
                what = "%s | %s" % (name, mname)
                try:
                    rec = run_entry(L, h, layer_of(arg if kind == "spec" else s), entry, arg if kind == "env" else env,
                                    arg if kind == "desc" else (lambda d, s2: None), arg if kind == "ws" else None, what)
                except AssertionError as e:
                    if failures is None:
                        raise
                    failures.append(str(e))
                    continue
                if rec is not None:
                    records[what] = rec
            layers.clear()
    finally:
        os.environ.update(saved)
    return {"num_cus": torch.cuda.get_device_properties(0).multi_processor_count, "entries": len(records), "records": records}


def test_persistent_launcher_edges_match_the_recorded_census(pkg, handle):
    with open(FIXTURE) as f:
        want = json.load(f)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != want["num_cus"]:
        pytest.skip("the census was recorded on %d CUs, this device has %d" % (want["num_cus"], cus))
    got = census(pkg._lib, handle)
    assert sorted(got["records"]) == sorted(want["records"])
    bad = ["%s: got %s, recorded %s" % (k, got["records"][k], v) for k, v in want["records"].items() if got["records"][k] != v]
    print("persistent launcher edges: %d entries compared, %d differ" % (len(want["records"]), len(bad)))
    assert len(got["records"]) == want["entries"] == len(want["records"])
    assert not bad, "[rc, impl, tile, stream-K, workspace bytes, error text] moved:\n" + "\n".join(bad[:40])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    hd = pkg.Handle(0)
    hd.set_stream(torch.cuda.current_stream().cuda_stream)
    wrong = []
    c = census(pkg._lib, hd, wrong)
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as f:                             # one line per entry
        f.write('{"num_cus": %d,\n"entries": %d,\n"records": {\n' % (c["num_cus"], c["entries"]))
        f.write(",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in c["records"].items()) + "\n}}\n")
    taken = sum(1 for r in c["records"].values() if r[0] == 0)
    print("\n".join(wrong))
    assert not wrong, "%d launches returned RTN_OK with a wrong output" % len(wrong)
    print("wrote %s: %d entries (%d launched and compared with the reference), num_cus %d, library %s" % (path, c["entries"], taken, c["num_cus"], pkg.LIB_PATH))
