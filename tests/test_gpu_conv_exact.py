"""GPU: every convolution kernel family and fusion on exact operands (tests/conv_exact.py), compared with the float64 reference by
torch.equal - no tolerance, no share of elements left out.

The operands are small integers, so every product and every partial sum is exact in f32 in any order, and the only roundings a
kernel may apply are the ones include/rtn.h documents: one to bf16 (or e4m3) on the way out, and in the fused kernels one per
intermediate tensor that the separate launches would have stored.  tests/test_conv_exact_cases.py shows without a GPU that every
case used here has sums below 2^24, exercises the final rounding (>= 5 % of each compared tensor not representable before it,
>= 2 % exact ties) and would change under truncation.  Where a knob forces a kernel, the launch must really have been that kernel.

What stays on a tolerance elsewhere: the sigmoid head (exp is not exact; tests/test_gpu_conv.py) and every random-operand test, the
check on realistic magnitudes.

The head outputs at 27, 54, 72, 180 and 270 channels (3 to 30 classes) run under the default dispatch and every forced generation and
tile width, in the engine's dense layout and with pad columns and gap rows that must keep their fill; their data gradient reads the
padded concatenated dY at Crun = 64 ... 512, and rtn_pad_cast_rows is compared alone.

The module runs in a few seconds, so no knob combination of the matrix is cut.  K slices (RTN_CONV_H8_KSPLIT=3) exist only for the
full-width single-level layer without residual or mask, so they have a test of their own at (12, 11); every other generation-4 case
pins RTN_CONV_H8_KSPLIT=1."""
import ctypes as C

import pytest
import torch

import conv_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -77.0


def _to_dev(x, dtype, scale=1.0):
    if dtype == "fp8":
        return X.e4m3_bytes(x * scale).to(DEV).contiguous()
    return x.to(torch.bfloat16 if dtype == "bf16" else torch.float32).to(DEV).contiguous()


def _from_dev(t, fmt):
    return (t.cpu().view(X.F8) if fmt == "e4m3" else t.cpu()).to(torch.float64)


def assert_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError("%s: %d of %d elements differ from the float64 reference rounded once; first at %s (got %r, want %r); "
                             "last-axis indices %s" % (what, len(bad), got.numel(), bad[0].tolist(), float(got[tuple(bad[0])]),
                                                       float(want[tuple(bad[0])]), sorted(set(bad[:, -1].tolist()))[:24]))


def launch_conv(pkg, handle, c, entry="fwd", pad_cols=0, gap_rows=0):
    """One launch of a ConvCase through `entry` ("fwd", "dual", "fp8", "fp8out"); compares every level with the reference and checks
    the never-written columns / pixels.  Returns the descriptor (its workspace fields tell whether a K split was planned).
    Concatenated cases: out_ld = cout + pad_cols, and gap_rows rows of out_ld elements in front of the first level, between two levels
    and behind the last one of every image; the pad columns and the gap rows must keep the buffer's fill."""
    L = pkg._lib
    tdt = {"bf16": torch.bfloat16, "f32": torch.float32, "fp8": torch.uint8}[c.dtype]
    odt = {"bf16": torch.bfloat16, "f32": torch.float32, "e4m3": torch.uint8}[c.fmt]
    B, cin, cout, k = c.B, c.cin, c.cout, c.k
    wk = c.w.permute(3, 0, 1, 2).reshape(cout, -1)
    if c.src2:
        wk = torch.cat([wk, c.w2.T], 1)                   # the second layer's filters behind the first's along K
    rows = -(-cout // 128) * 128
    wfull = torch.zeros(rows, wk.shape[1], dtype=torch.float64)
    wfull[:cout] = wk
    wd = _to_dev(wfull, c.dtype, c.s_w)
    bd = torch.zeros(rows, dtype=torch.float32)
    bd[:cout] = c.bias.float()
    bd = bd.to(DEV)
    d = L.ConvDesc()
    d.ngroups, d.batch, d.dtype = len(c.levels), B, {"bf16": L.RTN_BF16, "f32": L.RTN_F32, "fp8": L.RTN_FP8}[c.dtype]
    d.w, d.bias, d.w_rows, d.N, d.KH, d.KW = wd.data_ptr(), bd.data_ptr(), rows, cout, k, k
    d.Crun = d.pix_stride = cin
    d.sy = d.sx = c.stride
    d.out_ld = ld = cout + pad_cols
    d.flags = (L.CONV_RELU if c.relu else 0) | {None: 0, "same": L.CONV_RES_SAME, "up": L.CONV_RES_UPSAMPLE}[c.res] | \
        {None: 0, "post": L.CONV_RELU_MASK, "pre": L.CONV_RELU_MASK | L.CONV_MASK_PRE}[c.mask] | \
        (L.CONV_OUT_F32 if (c.fmt == "f32" and c.dtype == "bf16") else 0)
    fill = 7 if c.fmt == "e4m3" else SENTINEL
    keep, outs, s2 = [wd, bd], [], None
    if c.concat:                                           # head-output style: all levels into one (B, total, cout) tensor
        total = sum(lv.Ho * lv.Wo + gap_rows for lv in c.levels) + gap_rows
        big = torch.full((B, total * ld + 8), fill, dtype=odt, device=DEV)
        off = gap_rows * ld
    for gi, lv in enumerate(c.levels):
        xd = _to_dev(lv.x, c.dtype, c.s_x)
        grp = L.ConvGroup()
        grp.in_, grp.in_elems, grp.in_img_stride, grp.in_row_stride = xd.data_ptr(), xd.numel(), lv.H * lv.W * cin, lv.W * cin
        grp.Hin, grp.Win, grp.Hout, grp.Wout = lv.H, lv.W, lv.Ho, lv.Wo
        d.pad_t, d.pad_l = lv.pt, lv.pl                    # the same for every level of the grouped cases (stride 1)
        Hg, Wg = lv.act.shape[1], lv.act.shape[2]
        if c.concat:
            grp.out, grp.out_elems, grp.out_img_stride, grp.out_off = big.data_ptr(), big.numel(), total * ld + 8, off
            outs.append((off // ld, lv.Ho * lv.Wo))
            off += (lv.Ho * lv.Wo + gap_rows) * ld
        else:
            od = torch.full((B, Hg, Wg, cout), fill, dtype=odt, device=DEV)
            grp.out, grp.out_elems, grp.out_img_stride = od.data_ptr(), od.numel(), Hg * Wg * cout
            outs.append(od)
        if c.out_step > 1:
            grp.out_step, grp.out_pix_w = c.out_step, Wg
        if c.res:
            rd = _to_dev(lv.other, c.dtype)
            grp.res, grp.res_elems, grp.res_img_stride, grp.res_ld = rd.data_ptr(), rd.numel(), rd.numel() // B, cout
            grp.Hres, grp.Wres = rd.shape[1], rd.shape[2]
            keep.append(rd)
        if c.mask:
            ad = _to_dev(lv.act, c.dtype)
            grp.mask, grp.mask_elems, grp.mask_img_stride, grp.mask_ld = ad.data_ptr(), ad.numel(), Hg * Wg * cout, cout
            keep.append(ad)
        if c.src2:
            c2, step = c.src2
            x2d = _to_dev(lv.x2, c.dtype)
            Hs, Ws = lv.x2.shape[1], lv.x2.shape[2]
            s2 = L.ConvSrc2()
            s2.in_, s2.in_elems, s2.in_img_stride, s2.in_row_stride, s2.pix_stride = x2d.data_ptr(), x2d.numel(), Hs * Ws * c2, Ws * c2, c2
            s2.Hin, s2.Win, s2.C, s2.step = Hs, Ws, c2, step
            keep.append(x2d)
        d.g[gi] = grp
        keep.append(xd)
    if entry == "fp8":
        qd = L.ConvFp8(acc_scale=1.0 / (c.s_x * c.s_w), out_scale=c.out_scale, out_dtype=L.RTN_FP8 if c.fmt == "e4m3" else L.RTN_BF16)
        handle.check(L.lib.rtn_conv2d_fp8_fwd(handle.raw, C.byref(d), C.byref(qd)))
    elif entry == "fp8out":
        L.attach_conv_workspace(handle, d)
        handle.check(L.lib.rtn_conv2d_fwd_fp8out(handle.raw, C.byref(d), c.out_scale))
    elif entry == "dual":
        assert d.w_rows == d.N
        L.attach_conv_workspace(handle, d, s2)
        handle.check(L.lib.rtn_conv1x1_dual_fwd(handle.raw, C.byref(d), C.byref(s2)))
    else:
        L.attach_conv_workspace(handle, d)
        handle.check(L.lib.rtn_conv2d_fwd(handle.raw, C.byref(d)))
    torch.cuda.synchronize()
    if c.concat:
        flat = _from_dev(big, c.fmt)
        assert torch.all(flat[:, total * ld:] == fill), c.name + ": wrote behind the image's last row"
        rows = flat[:, :total * ld].reshape(B, total, ld)
        written = torch.zeros(total, ld, dtype=torch.bool)
        for row0, cells in outs:
            written[row0:row0 + cells, :cout] = True
        stray = (rows != fill) & ~written
        assert not bool(stray.any()), "%s: %d elements outside the levels' slices were written, first at %s" % (c.name, int(stray.sum()), stray.nonzero()[0].tolist())
        assert_equal(torch.cat([rows[:, row0:row0 + cells, :cout] for row0, cells in outs], 1), c.stages[0].want, c.name)
    else:
        s = c.out_step
        for lv, od in zip(c.levels, outs):
            got = _from_dev(od, c.fmt)
            if s > 1:                                      # off the stride grid nothing is written
                rest = torch.ones(got.shape[1], got.shape[2], dtype=torch.bool)
                rest[::s, ::s] = False
                assert torch.all(got[:, rest] == fill)
            assert_equal(got[:, ::s, ::s], lv.stage.want, "%s level %dx%d" % (c.name, lv.H, lv.W))
    d._keep = keep
    return d


def last_impl(pkg, handle):
    return pkg._lib.lib.rtn_debug_last_conv_impl(handle.raw)


def sk_timeouts(pkg, handle, d):
    n = C.c_uint32(123)
    handle.check(pkg._lib.lib.rtn_debug_conv_sync_timeouts(handle.raw, d.workspace, C.byref(n)))
    return int(n.value)


# ------------------------------------------------------------------------------------------------ 1. generations 1, 2, 3
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("res", [None, "same", "up"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("impl", [1, 2, 3])
def test_generations_1_2_3_on_the_3x3_layer(pkg, handle, monkeypatch, impl, dtype, res, relu):
    """cin 256 -> 136 over [(12, 11), (2, 3)]: 36 K chunks, two tiles, a group boundary inside the second, N not a tile multiple; the
    residual of the same extent or upsampled from a coarser (H+1)/2 x ((W+1)/2 + 1) level.  f32 has no rounding at all."""
    monkeypatch.setenv("RTN_CONV_IMPL", str(impl))
    launch_conv(pkg, handle, X.case("gen123/3x3/%s/relu%d/res-%s" % (dtype, relu, res)))
    assert last_impl(pkg, handle) == impl


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("layer", ["1x1s2", "3x3s2"])
@pytest.mark.parametrize("impl", [1, 2])
def test_generations_1_2_on_the_stride_2_layers(pkg, handle, monkeypatch, impl, layer, dtype, relu):
    """1x1 stride-2 'valid' 256 -> 128 at (9, 13); 3x3 stride-2 'same' 128 -> 64 at (9, 12): TF's asymmetric padding (1 above, 0 left)."""
    monkeypatch.setenv("RTN_CONV_IMPL", str(impl))
    launch_conv(pkg, handle, X.case("gen123/%s/%s/relu%d" % (layer, dtype, relu)))
    assert last_impl(pkg, handle) == impl


# ------------------------------------------------------------------------------------------------ 2. tail split and split-K
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("impl,layer,slots", [(2, "3x3", 18), (3, "3x3", 18), (2, "1x1res", 19)])
def test_tail_split_and_unsplit_launch_equal_the_reference(pkg, handle, monkeypatch, impl, layer, slots, dtype, relu):
    """20 (21) tiles of 256 x 64 on 18 (19) pretended slots: the last 2 tiles go to K-slice workgroups and a finish launch.  The split
    launch and the unsplit one both EQUAL the reference, hence each other; the split must really have been planned (it is what asks
    for the slabs)."""
    monkeypatch.setenv("RTN_CONV_IMPL", str(impl))
    monkeypatch.setenv("RTN_CONV_BN2", "64")
    monkeypatch.setenv("RTN_CONV_TAIL_SLOTS", str(slots))
    c = X.case("tail/%s/%s/relu%d" % (layer, dtype, relu))
    d = launch_conv(pkg, handle, c)
    assert last_impl(pkg, handle) == impl and d.workspace_bytes > 0 and d.workspace, "the tail split was not planned"
    assert pkg._lib.lib.rtn_debug_last_conv_tile(handle.raw) & 0xFFFF == 64
    monkeypatch.setenv("RTN_CONV_TAIL", "0")
    d = launch_conv(pkg, handle, c)
    assert last_impl(pkg, handle) == impl and d.workspace_bytes == 0


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_split_k_and_unsplit_launch_equal_the_reference(pkg, handle, monkeypatch, dtype, relu):
    """Generation 1's split-K for tiny-M, long-K layers: 2048 -> 64 at (6, 7), 32 K steps in 4 slices through caller-owned slabs."""
    monkeypatch.setenv("RTN_CONV_IMPL", "1")
    c = X.case("splitk/1x1/%s/relu%d" % (dtype, relu))
    for splitk in ("4", "0"):
        monkeypatch.setenv("RTN_CONV_SPLITK", splitk)
        d = launch_conv(pkg, handle, c)
        assert last_impl(pkg, handle) == 1 and (d.workspace_bytes > 0) == (splitk == "4")


# ------------------------------------------------------------------------------------------------ 3. generation 4
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("mode", ["none", "res", "res+mask_pre"])
@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("stagger", [0, 1])
@pytest.mark.parametrize("mi", [3, 4])
@pytest.mark.parametrize("shape", ["256-136", "128-72"])
def test_generation_4_with_rings_that_wrap(pkg, handle, monkeypatch, shape, mi, stagger, grid, mode, relu):
    """Four (two) K chunks per tap, so the A and B rings wrap inside a tile; one or two workgroups walk both tiles and both levels."""
    monkeypatch.setenv("RTN_CONV_IMPL", "4")
    monkeypatch.setenv("RTN_CONV_H8_MI", str(mi))
    monkeypatch.setenv("RTN_CONV_H8_STAGGER", str(stagger))
    monkeypatch.setenv("RTN_CONV_H8_GRID", str(grid))
    monkeypatch.setenv("RTN_CONV_H8_KSPLIT", "1")
    launch_conv(pkg, handle, X.case("gen4/%s/%s/relu%d" % (shape, mode, relu)))
    assert last_impl(pkg, handle) == 4
    assert pkg._lib.lib.rtn_debug_last_conv_tile(handle.raw) == ((64 * mi) << 16) | (256 if shape == "256-136" else 128)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("stagger", [0, 1])
@pytest.mark.parametrize("mi", [3, 4])
def test_generation_4_k_slices(pkg, handle, monkeypatch, mi, stagger, grid, relu):
    """cin 256 -> 136 at (12, 11): three K slices (one kernel row of four chunks each) through the f32 slabs, added in slice order by
    ksplit_finish_kernel (csrc/rtn_conv_ksplit.hip), and the same layer unsliced."""
    monkeypatch.setenv("RTN_CONV_IMPL", "4")
    monkeypatch.setenv("RTN_CONV_H8_MI", str(mi))
    monkeypatch.setenv("RTN_CONV_H8_STAGGER", str(stagger))
    monkeypatch.setenv("RTN_CONV_H8_GRID", str(grid))
    c = X.case("gen4/kslice/relu%d" % relu)
    slabs = 3 * 2 * 12 * 11 * 256 * 4                      # three f32 slabs [M = 264][256]
    for ks in ("3", "1"):
        monkeypatch.setenv("RTN_CONV_H8_KSPLIT", ks)
        d = launch_conv(pkg, handle, c)
        assert last_impl(pkg, handle) == 4
        assert (d.workspace_bytes >= slabs) == (ks == "3"), "K slices: %s asked for, workspace %d" % (ks, d.workspace_bytes)


# ------------------------------------------------------------------------------------------------ 4. generation 5
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("sk", [0, 1])
@pytest.mark.parametrize("mi", [2, 3])
@pytest.mark.parametrize("cout", [256, 128])
def test_generation_5_with_8_k_steps(pkg, handle, monkeypatch, cout, mi, sk, relu):
    """512 -> 256 and 512 -> 128 (the narrow instance) at (11, 13): 8 K steps, 286 rows = 3 / 2 tiles; stream-K where the shape allows."""
    monkeypatch.setenv("RTN_CONV_IMPL", "5")
    monkeypatch.setenv("RTN_CONV_G8_MI", str(mi))
    monkeypatch.setenv("RTN_CONV_H8_GRID", "2")
    monkeypatch.setenv("RTN_CONV_G8_SK", str(sk))
    d = launch_conv(pkg, handle, X.case("gen5/512-%d/relu%d" % (cout, relu)))
    assert last_impl(pkg, handle) == 5
    if not sk:
        assert pkg._lib.lib.rtn_debug_last_conv_tile(handle.raw) == ((64 * mi) << 16) | cout
    assert (pkg._lib.lib.rtn_debug_last_conv_streamk(handle.raw) > 0) == (sk == 1 and cout == 256)      # the narrow instance has no stream-K form
    if sk == 1 and cout == 256:
        assert sk_timeouts(pkg, handle, d) == 0


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("sk", [0, 1])
@pytest.mark.parametrize("mi", [2, 3])
@pytest.mark.parametrize("form", ["s2", "up", "scatter"])
@pytest.mark.parametrize("cout", [256, 128])
def test_generation_5_other_forms(pkg, handle, monkeypatch, cout, form, mi, sk, relu):
    """Stride-2 'valid' sampling at (9, 13); the residual upsampled from a coarser level; out_step 2 scatter with residual and mask
    on the stride grid (the pixels between keep the buffer's fill)."""
    monkeypatch.setenv("RTN_CONV_IMPL", "5")
    monkeypatch.setenv("RTN_CONV_G8_MI", str(mi))
    monkeypatch.setenv("RTN_CONV_H8_GRID", "2")
    monkeypatch.setenv("RTN_CONV_G8_SK", str(sk))
    d = launch_conv(pkg, handle, X.case("gen5/512-%d/%s/relu%d" % (cout, form, relu)))
    assert last_impl(pkg, handle) == 5
    streamk = sk == 1 and cout == 256 and form != "scatter"                # neither the narrow instance nor the scatter / mask forms
    assert (pkg._lib.lib.rtn_debug_last_conv_streamk(handle.raw) > 0) == streamk
    if streamk:
        assert sk_timeouts(pkg, handle, d) == 0


# ------------------------------------------------------------------------------------------------ 5. dual-source 1x1
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("sk", [0, 1])
@pytest.mark.parametrize("step", [1, 2])
def test_dual_source_1x1(pkg, handle, monkeypatch, step, sk, relu):
    """rtn_conv1x1_dual_fwd: c1 128 + c2 256 -> 512 at (7, 9); step 2 samples the second source at (13, 17)."""
    monkeypatch.setenv("RTN_CONV_IMPL", "5")
    monkeypatch.setenv("RTN_CONV_H8_GRID", "2")
    monkeypatch.setenv("RTN_CONV_G8_SK", str(sk))
    d = launch_conv(pkg, handle, X.case("dual/step%d/relu%d" % (step, relu)), entry="dual")
    assert last_impl(pkg, handle) == 5
    assert (pkg._lib.lib.rtn_debug_last_conv_streamk(handle.raw) > 0) == (sk == 1)
    if sk:
        assert sk_timeouts(pkg, handle, d) == 0


def test_dual_source_1x1_on_generation_2(pkg, handle, monkeypatch):
    """... and the per-tap kernel's walk over the second source (what the layer takes when generation 5 does not apply)."""
    monkeypatch.setenv("RTN_CONV_IMPL", "2")
    for step in (1, 2):
        launch_conv(pkg, handle, X.case("dual/step%d/relu1" % step), entry="dual")
        assert last_impl(pkg, handle) == 2


# ------------------------------------------------------------------------------------------------ 6. head output without sigmoid
@pytest.mark.parametrize("out,impl", [("f32", 0), ("f32", 6), ("f32", 2), ("f32", 1), ("bf16", 0), ("bf16", 2), ("bf16", 1)])
def test_head_output_concat(pkg, handle, monkeypatch, out, impl):
    """cout 36 into the concatenation of [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)], f32 (RTN_CONV_OUT_F32: no rounding at all) or bf16:
    the default path, the persistent head-output kernel (generation 6, f32 output only) and generations 1 / 2."""
    if impl:
        monkeypatch.setenv("RTN_CONV_IMPL", str(impl))
    launch_conv(pkg, handle, X.case("head/%s" % out))
    if impl:
        assert last_impl(pkg, handle) == impl


def head_output_runs(cout, out):
    """[(RTN_CONV_IMPL or 0, RTN_CONV_BN2 or 0, generation that must run, tile width that must run or None)] of a head-output launch:
    what csrc/rtn_conv.hip documents.  Generation 6 takes up to 48 channels with f32 output; generation 4 wants dense outputs and
    generation 5 a 1x1 layer, so a forced 4 goes to the shared-halo kernel and a forced 5 / 6 that does not apply to the per-tap
    kernel.  RTN_CONV_BN2 is honoured up to N rounded up to 64 columns; the cost model picks 64 on grids this small."""
    gen6 = cout <= 48 and out == "f32"
    runs = [(0, 0, (2, 6) if gen6 else (2,), 64),(1, 0, (1,), 64 if cout <= 64 else 128), (4, 0, (3,), 64), (5, 0, (2,), 64),
            (6, 0, (6,) if gen6 else (2,), None if gen6 else 64)]
    for impl in (2, 3):
        runs += [(impl, bn, (impl,), bn or 64) for bn in (0, 64, 128, 256) if bn <= -(-cout // 64) * 64]
    return runs


@pytest.mark.parametrize("out", ["f32", "bf16"])
@pytest.mark.parametrize("cout", X.HEAD_COUTS)
def test_head_output_concat_at_many_classes(pkg, handle, monkeypatch, cout, out):
    """cout = 9 K for K = 3, 6, 8, 20, 30 into the concatenation of the five levels: above 48 channels generation 6 never runs, not
    even when asked for; 72 fills a 128-wide tile, 180 a 256-wide one and 270 needs a second N tile in every generation.  Every run in
    the dense layout the engine uses (out_ld = cout) and with 16 pad columns and 3 gap rows around every level, all of which must
    keep the fill: an N tile that stores past column cout - 1, or a row tile past its level's last cell, lands there."""
    c = X.case("head%d/%s" % (cout, out))
    ran = []
    for impl, bn, gens, width in head_output_runs(cout, out):
        for k, v in (("RTN_CONV_IMPL", impl), ("RTN_CONV_BN2", bn)):
            if v:
                monkeypatch.setenv(k, str(v))
            else:
                monkeypatch.delenv(k, raising=False)
        for pad_cols, gap_rows in ((0, 0), (16, 3)):
            launch_conv(pkg, handle, c, pad_cols=pad_cols, gap_rows=gap_rows)
            got, tile = last_impl(pkg, handle), pkg._lib.lib.rtn_debug_last_conv_tile(handle.raw) & 0xFFFF
            ran.append((impl, bn, got, tile))
            assert got in gens, "RTN_CONV_IMPL=%d RTN_CONV_BN2=%d ran generation %d, expected %s" % (impl, bn, got, gens)
            assert cout <= 48 or got != 6
            if width is not None and got != 6:
                assert tile == width, "RTN_CONV_IMPL=%d RTN_CONV_BN2=%d ran on %d-wide tiles, expected %d" % (impl, bn, tile, width)
    print("head%d/%s (forced, BN2, generation, tile width): %s" % (cout, out, ran))


# ------------------------------------------------------------------------------------------------ 7. data gradient
def launch_dgrad(pkg, handle, c, impl):
    L = pkg._lib
    B, H, W, cin, cout, k = c.B, c.H, c.W, c.cin, c.cout, c.k
    wf = torch.zeros(-(-cout // 128) * 128, k * k * cin, dtype=torch.float64)
    wf[:cout] = c.w.permute(3, 0, 1, 2).reshape(cout, -1)
    wf = wf.to(torch.bfloat16).to(DEV).contiguous()
    rows_d = (256 if cin > 128 else 128) if impl == 4 else (cin if impl == 5 else -(-cin // 128) * 128)
    wd = torch.zeros(rows_d, k * k * cout, dtype=torch.bfloat16, device=DEV)
    handle.check(L.lib.rtn_pack_dgrad_weights(handle.raw, wf.data_ptr(), wd.data_ptr(), L.RTN_BF16, cout, wf.shape[0], k, k, cin, cout, rows_d))
    dyd = c.dy.to(torch.bfloat16).to(DEV).contiguous()
    d = L.ConvDesc()
    d.ngroups, d.batch, d.dtype = 1, B, L.RTN_BF16
    d.w, d.w_rows, d.N, d.KH, d.KW = wd.data_ptr(), rows_d, cin, k, k
    d.Crun = d.pix_stride = cout
    d.sy = d.sx = 1
    d.out_ld = cin
    d.flags = (L.CONV_RES_SAME if "res" in c.mode else 0) | (L.CONV_RELU_MASK if "mask" in c.mode else 0) | (L.CONV_MASK_PRE if "pre" in c.mode else 0)
    keep = [wd, dyd]
    if c.bias is not None:
        bd = torch.zeros(rows_d, dtype=torch.float32)
        bd[:cin] = c.bias.float()
        bd = bd.to(DEV)
        d.bias = bd.data_ptr()
        keep.append(bd)
    grp = L.ConvGroup()
    src, Hs, Ws = dyd, c.Ho, c.Wo
    if c.stride == 1:
        d.pad_t, d.pad_l = k - 1 - c.pt, k - 1 - c.pl
        grp.Hout, grp.Wout = H, W
    elif k == 1:
        grp.Hout, grp.Wout = c.Ho, c.Wo
        grp.out_step, grp.out_pix_w = 2, W
    else:
        Hu, Wu = 2 * c.Ho - 1, 2 * c.Wo - 1
        src = torch.full((B, Hu, Wu, cout), 5.0, dtype=torch.bfloat16, device=DEV)
        handle.check(L.lib.rtn_zero_insert2(handle.raw, dyd.data_ptr(), src.data_ptr(), L.RTN_BF16, B, c.Ho, c.Wo, cout, Hu, Wu))
        keep.append(src)
        Hs, Ws = Hu, Wu
        d.pad_t, d.pad_l = k - 1 - c.pt, k - 1 - c.pl
        grp.Hout, grp.Wout = H, W
    grp.in_, grp.in_elems, grp.in_img_stride, grp.in_row_stride = src.data_ptr(), src.numel(), Hs * Ws * cout, Ws * cout
    grp.Hin, grp.Win = Hs, Ws
    prefill = c.other if "res" in c.mode else torch.full((B, H, W, cin), SENTINEL, dtype=torch.float64)
    dxd = prefill.to(torch.bfloat16).to(DEV).contiguous()                  # in place: the accumulated gradient is the residual
    actd = c.act.to(torch.bfloat16).to(DEV).contiguous()
    grp.out, grp.out_elems, grp.out_img_stride = dxd.data_ptr(), dxd.numel(), H * W * cin
    if "res" in c.mode:
        grp.res, grp.res_elems, grp.res_img_stride, grp.res_ld = dxd.data_ptr(), dxd.numel(), H * W * cin, cin
    if "mask" in c.mode:
        grp.mask, grp.mask_elems, grp.mask_img_stride, grp.mask_ld = actd.data_ptr(), actd.numel(), H * W * cin, cin
    d.g[0] = grp
    L.attach_conv_workspace(handle, d)
    handle.check(L.lib.rtn_conv2d_dgrad(handle.raw, C.byref(d)))
    torch.cuda.synchronize()
    got = dxd.cpu().double()
    s = c.step
    if s > 1:                                              # off the stride grid the buffer keeps what it held
        rest = torch.ones(H, W, dtype=torch.bool)
        rest[::s, ::s] = False
        assert torch.equal(got[:, rest], X.bf16(prefill)[:, rest])
    assert_equal(got[:, ::s, ::s], c.stages[0].want, c.name)


DGRAD = [("3x3-64-256", (1, 2)), ("3x3-256-64", (1, 2, 4)), ("1x1s2", (1, 2, 5)), ("1x1s2-even", (1, 2, 5)), ("3x3s2", (1, 2, 4)), ("3x3s2-even", (1, 2))]


@pytest.mark.parametrize("mode", ["res", "mask", "res+mask_pre"])
@pytest.mark.parametrize("layer,impl", [(name, impl) for name, impls in DGRAD for impl in impls])
def test_data_gradient(pkg, handle, monkeypatch, layer, impl, mode):
    """rtn_pack_dgrad_weights + rtn_conv2d_dgrad against the float64 conv-transpose of the integer dY.  cin != cout, so a transposition
    error of the pack shows.  Generation 4 takes the stride-1 3x3 gradients with more than 64 channels and an input of the output's
    extent (the zero-inserted dY of an odd H x W), generation 5 the 1x1 scatter."""
    monkeypatch.setenv("RTN_CONV_IMPL", str(impl))
    monkeypatch.setenv("RTN_CONV_H8_GRID", "2")
    launch_dgrad(pkg, handle, X.case("dgrad/%s/%s" % (layer, mode)), impl)
    assert last_impl(pkg, handle) == impl


def launch_head_dgrad(pkg, handle, c, impl):
    """The grouped launch the trainer builds for a head-output layer: dY of the five levels inside one [B][cells][cp] tensor whose
    columns cout .. cp - 1 are zero, Crun = cp, the forward weights packed for Cout_run = cp, one dX tensor per level."""
    L = pkg._lib
    B, cin, cout, cp, k = c.B, c.cin, c.cout, c.cp, 3
    wf = torch.zeros(-(-cout // 128) * 128, k * k * cin, dtype=torch.float64)
    wf[:cout] = c.w.permute(3, 0, 1, 2).reshape(cout, -1)
    wf = wf.to(torch.bfloat16).to(DEV).contiguous()
    rows_d = 256 if impl == 4 else -(-cin // 128) * 128
    wd = torch.full((rows_d, k * k * cp), 9.0, dtype=torch.bfloat16, device=DEV)     # the pack must write the zeros of channels cout .. cp - 1 itself
    handle.check(L.lib.rtn_pack_dgrad_weights(handle.raw, wf.data_ptr(), wd.data_ptr(), L.RTN_BF16, cout, wf.shape[0], k, k, cin, cp, rows_d))
    total = sum(H * W for H, W in c.levels_hw)
    dyp = torch.zeros(B, total, cp, dtype=torch.float64)
    off = 0
    for (H, W), dy in zip(c.levels_hw, c.dy):
        dyp[:, off:off + H * W, :cout] = dy.reshape(B, H * W, cout)
        off += H * W
    dyd = dyp.to(torch.bfloat16).to(DEV).contiguous()
    d = L.ConvDesc()
    d.ngroups, d.batch, d.dtype = len(c.levels_hw), B, L.RTN_BF16
    d.w, d.w_rows, d.N, d.KH, d.KW = wd.data_ptr(), rows_d, cin, k, k
    d.Crun = d.pix_stride = cp
    d.sy = d.sx = 1
    d.pad_t = d.pad_l = 1
    d.out_ld = cin
    d.flags = (L.CONV_RES_SAME if "res" in c.mode else 0) | (L.CONV_RELU_MASK if "mask" in c.mode else 0) | (L.CONV_MASK_PRE if "pre" in c.mode else 0)
    keep = [wd, dyd]
    if c.bias is not None:
        bd = torch.zeros(rows_d, dtype=torch.float32)
        bd[:cin] = c.bias.float()
        bd = bd.to(DEV)
        d.bias = bd.data_ptr()
        keep.append(bd)
    outs, off = [], 0
    for gi, (H, W) in enumerate(c.levels_hw):
        grp = L.ConvGroup()
        grp.in_, grp.in_elems = dyd.data_ptr() + off * cp * 2, dyd.numel() - off * cp      # as bplan.dgrad_group points a level into the tensor
        grp.in_img_stride, grp.in_row_stride = total * cp, W * cp
        grp.Hin, grp.Win, grp.Hout, grp.Wout = H, W, H, W
        prefill = c.other[gi] if "res" in c.mode else torch.full((B, H, W, cin), SENTINEL, dtype=torch.float64)
        dxd = prefill.to(torch.bfloat16).to(DEV).contiguous()
        grp.out, grp.out_elems, grp.out_img_stride = dxd.data_ptr(), dxd.numel(), H * W * cin
        if "res" in c.mode:
            grp.res, grp.res_elems, grp.res_img_stride, grp.res_ld = dxd.data_ptr(), dxd.numel(), H * W * cin, cin
        if "mask" in c.mode:
            actd = c.act[gi].to(torch.bfloat16).to(DEV).contiguous()
            grp.mask, grp.mask_elems, grp.mask_img_stride, grp.mask_ld = actd.data_ptr(), actd.numel(), H * W * cin, cin
            keep.append(actd)
        d.g[gi] = grp
        outs.append(dxd)
        off += H * W
    L.attach_conv_workspace(handle, d)
    handle.check(L.lib.rtn_conv2d_dgrad(handle.raw, C.byref(d)))
    torch.cuda.synchronize()
    assert_equal(torch.cat([o.cpu().double().reshape(B, -1, cin) for o in outs], 1), c.stages[0].want, c.name)


@pytest.mark.parametrize("mode", ["res", "mask", "res+mask_pre"])
@pytest.mark.parametrize("impl", [0, 1, 2, 4])
@pytest.mark.parametrize("cout,cp", X.HEAD_DGRAD)
def test_data_gradient_of_the_head_outputs(pkg, handle, monkeypatch, cout, cp, impl, mode):
    """dX of the 3x3 256 -> cout head-output layer from the padded concatenated dY: Crun = 64, 128, 256 and 512 (6, 8, 20 and 30 classes).
    The default dispatch must take one of the 256-row generations; generations 1, 2 and 4 where forced."""
    if impl:
        monkeypatch.setenv("RTN_CONV_IMPL", str(impl))
    monkeypatch.setenv("RTN_CONV_H8_GRID", "2")
    launch_head_dgrad(pkg, handle, X.case("dgrad/head%d-%d/%s" % (cout, cp, mode)), impl)
    got = last_impl(pkg, handle)
    print("head dgrad cout %d Crun %d %s: forced %d ran generation %d" % (cout, cp, mode, impl, got))
    assert got == impl if impl else got in (2, 3, 4)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("cin,cp", [(9, 64), (36, 64), (54, 64), (72, 128), (180, 256), (270, 512)])
def test_pad_cast_rows_alone(pkg, handle, dtype, cin, cp):
    """rtn_pad_cast_rows on 2 x 129 + 1 = 259 rows (no multiple of 256): the kept columns are torch's round-to-nearest-even cast of the
    f32 input bit for bit (ties, values that overflow bf16's mantissa, both zeros, a subnormal), the pad columns are exact +0, and
    nothing behind the last row is written."""
    L = pkg._lib
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    rows = 259
    g = torch.Generator().manual_seed(cin)
    src = torch.randn(rows, cin, generator=g) * 3.0
    src[0, :8] = torch.tensor([257.0, 259.0, 1.00390625, -1.01171875, 0.0, -0.0, 1e-40, 3.3895313892515355e38])     # ties both ways, zeros, a subnormal, rounds to bf16 max
    raw = torch.full((rows * cp + 64,), SENTINEL, dtype=tdt, device=DEV)
    srcd = src.to(DEV).contiguous()
    handle.check(L.lib.rtn_pad_cast_rows(handle.raw, srcd.data_ptr(), raw.data_ptr(), L.RTN_BF16 if dtype == "bf16" else L.RTN_F32, rows, cin, cp))
    torch.cuda.synchronize()
    got = raw.cpu()
    assert torch.all(got[rows * cp:] == SENTINEL)
    got = got[:rows * cp].view(rows, cp)
    bits = (lambda t: t.contiguous().view(torch.int16)) if dtype == "bf16" else (lambda t: t.contiguous().view(torch.int32))
    assert torch.equal(bits(got[:, :cin]), bits(src.to(tdt)))
    assert torch.all(bits(got[:, cin:]) == 0)


# ------------------------------------------------------------------------------------------------ 8. rtn_bottleneck64_fwd
def launch_bottleneck(pkg, handle, c, a_out=True, h1_out=False, quarter=None):
    """quarter: None | "store" (x_out_step 2 with a_out) | "compute" (x_out_step = x_in_step = 2, no a_out)."""
    L = pkg._lib
    B, H, W = c.B, c.H, c.W
    t16 = lambda t: t.to(torch.bfloat16).to(DEV).contiguous()
    f32 = lambda t: t.float().to(DEV)
    ad, wbd, wcd, wad = t16(c.a), t16(c.w2b.reshape(64, 576)), t16(c.w2c), t16(c.w2a)
    bbd, bcd, bad = f32(c.b2b), f32(c.b2c), f32(c.b2a)
    q = 2 if quarter else 1
    xin = t16(c.x[:, ::2, ::2] if quarter == "compute" else c.x)
    pd = t16(c.p)
    Hx, Wx = (H + q - 1) // q, (W + q - 1) // q
    guard = 64
    raw = torch.full((B * Hx * Wx * 256 + guard,), -7.0, dtype=torch.bfloat16, device=DEV)
    xout = raw[:B * Hx * Wx * 256].view(B, Hx, Wx, 256)
    aout = torch.full((B, H, W, 64), -7.0, dtype=torch.bfloat16, device=DEV)
    h1o = torch.full((B, H, W, 64), -7.0, dtype=torch.bfloat16, device=DEV)
    d = L.BottleneckDesc()
    d.a_in, d.a_in_elems = ad.data_ptr(), ad.numel()
    d.x_out, d.x_out_elems = xout.data_ptr(), xout.numel()
    d.w2b, d.b2b, d.w2c, d.b2c = wbd.data_ptr(), bbd.data_ptr(), wcd.data_ptr(), bcd.data_ptr()
    d.batch, d.H, d.W, d.mid, d.dtype = B, H, W, 64, L.RTN_BF16
    if c.proj:
        d.p_in, d.p_in_elems, d.wproj, d.w2c_ld = pd.data_ptr(), pd.numel(), wcd.data_ptr() + 128, 128
    else:
        d.x_in, d.x_in_elems = xin.data_ptr(), xin.numel()
    if a_out:
        d.a_out, d.a_out_elems, d.w2a, d.b2a = aout.data_ptr(), aout.numel(), wad.data_ptr(), bad.data_ptr()
    if h1_out:
        d.h1_out, d.h1_out_elems = h1o.data_ptr(), h1o.numel()
    if quarter:
        d.x_out_step = 2
        d.x_in_step = 2 if quarter == "compute" else 0
    handle.check(L.lib.rtn_bottleneck64_fwd(handle.raw, C.byref(d)))
    torch.cuda.synchronize()
    what = "%s a_out=%d h1_out=%d quarter=%s" % (c.name, a_out, h1_out, quarter)
    assert torch.all(raw[xout.numel():] == -7.0), what + ": wrote past x_out"
    assert_equal(xout.cpu().double(), c.x_out.want[:, ::q, ::q], what + " x_out")
    if a_out:
        assert_equal(aout.cpu().double(), c.a_out.want, what + " a_out")
    else:
        assert torch.all(aout == -7.0)
    if h1_out:
        assert_equal(h1o.cpu().double(), c.h1.want, what + " h1_out")
    else:
        assert torch.all(h1o == -7.0)


@pytest.mark.parametrize("a_out,h1_out", [(True, False), (False, False), (True, True), (False, True)])
@pytest.mark.parametrize("shape,grid", [("2x9x13", 0), ("1x1x1", 0), ("3x5x4", 0), ("2x41x67", 2)])
@pytest.mark.parametrize("form", ["id", "proj"])
def test_bottleneck64(pkg, handle, monkeypatch, form, shape, grid, a_out, h1_out):
    """Identity and projection-shortcut forms, with and without the next block's branch2a and the h1 output: x_out, a_out and h1_out
    each EQUAL the float64 chain with h1, x_out and a_out rounded to bf16 where the header says.  RTN_BNECK_GRID=2: many strips per wave."""
    if grid:
        monkeypatch.setenv("RTN_BNECK_GRID", str(grid))
    launch_bottleneck(pkg, handle, X.case("bneck/%s/%s" % (form, shape)), a_out=a_out, h1_out=h1_out)


@pytest.mark.parametrize("nt", ["1", "0"])
@pytest.mark.parametrize("shape", ["2x9x13", "2x10x14"])
def test_bottleneck64_quarter_forms(pkg, handle, monkeypatch, shape, nt):
    """Store-quarter (everything computed, x_out kept at the even pixels) and compute-quarter (only the even pixels computed from the
    compact shortcut), odd and even extents, compact stores with and without the streaming hint."""
    monkeypatch.setenv("RTN_BNECK_COMPACT_NT", nt)
    c = X.case("bneck/id/%s" % shape)
    launch_bottleneck(pkg, handle, c, a_out=True, quarter="store")
    launch_bottleneck(pkg, handle, c, a_out=False, quarter="compute")


# ------------------------------------------------------------------------------------------------ 9. rtn_chain1x1_fwd
@pytest.mark.parametrize("pixels,grid", [(1, 0), (37, 0), (2049, 0), (2049, 2)])
def test_chain1x1(pkg, handle, monkeypatch, pixels, grid):
    """(128, 512, 128) on 1, 37 and 2049 pixels, the last also on 2 workgroups (several passes each, the filter stream wraps): both
    outputs EQUAL the reference with x_out rounded to bf16 before the second product."""
    L = pkg._lib
    if grid:
        monkeypatch.setenv("RTN_CHAIN_GRID", str(grid))
    c = X.case("chain/%d" % pixels)
    t16 = lambda t: t.to(torch.bfloat16).to(DEV).contiguous()
    hd, xd, wcd, wad = t16(c.h), t16(c.x), t16(c.w2c), t16(c.w2a)
    bcd, bad = c.b2c.float().to(DEV), c.b2a.float().to(DEV)
    xraw = torch.full((pixels * 512 + 64,), -7.0, dtype=torch.bfloat16, device=DEV)
    araw = torch.full((pixels * 128 + 64,), -7.0, dtype=torch.bfloat16, device=DEV)
    xout, aout = xraw[:pixels * 512].view(pixels, 512), araw[:pixels * 128].view(pixels, 128)
    d = L.ChainDesc()
    d.h_in, d.h_in_elems, d.x_in, d.x_in_elems = hd.data_ptr(), hd.numel(), xd.data_ptr(), xd.numel()
    d.x_out, d.x_out_elems, d.a_out, d.a_out_elems = xout.data_ptr(), xout.numel(), aout.data_ptr(), aout.numel()
    d.w2c, d.b2c, d.w2a, d.b2a = wcd.data_ptr(), bcd.data_ptr(), wad.data_ptr(), bad.data_ptr()
    d.pixels, d.mid, d.out, d.next, d.dtype = pixels, 128, 512, 128, L.RTN_BF16
    handle.check(L.lib.rtn_chain1x1_fwd(handle.raw, C.byref(d)))
    torch.cuda.synchronize()
    assert torch.all(xraw[pixels * 512:] == -7.0) and torch.all(araw[pixels * 128:] == -7.0)
    assert_equal(xout.cpu().double(), c.x_out.want, c.name + " x_out")
    assert_equal(aout.cpu().double(), c.a_out.want, c.name + " a_out")


# ------------------------------------------------------------------------------------------------ 10. fused stem and the indexed pool
@pytest.mark.parametrize("hw,grid", [((33, 35), 0), ((64, 96), 0), ((67, 101), 1)])
def test_fused_stem_at_kernel_level(pkg, handle, monkeypatch, hw, grid):
    """rtn_stem_pack of a bf16 image of integers, then rtn_stem_conv_pool and rtn_stem_conv_pool_branch2a (filters packed the way the
    engine packs them): pool1, a_out and pool_idx EQUAL the float64 7x7 / 2 convolution + bias + ReLU rounded once, pooled 3x3 / 2
    TF-'same' with the first maximum in kh * 3 + kw scan order among the in-image taps, and the 1x1 + ReLU rounded.  Integer ReLU
    outputs are full of ties.  RTN_STEM_GRID=1: one workgroup walks every tile."""
    import importlib
    L = pkg._lib
    Wt = importlib.import_module(pkg.__name__ + ".weights")
    if grid:
        monkeypatch.setenv("RTN_STEM_GRID", str(grid))
    c = X.case("stem/%dx%d" % hw)
    B, H, W = c.B, c.H, c.W
    H1, W1 = (H + 1) // 2, (W + 1) // 2
    H2, W2 = (H1 + 1) // 2, (W1 + 1) // 2
    Hp, Wp = max(H + 6, 2 * (H1 - 1) + 8), max(W + 6, 2 * (W1 - 1) + 8)
    Wp += Wp & 1
    img = c.img.to(torch.bfloat16).to(DEV).contiguous()
    xp = torch.zeros(B * Hp * Wp * 4 + 64, dtype=torch.bfloat16, device=DEV)      # + 64: the last pixel's 32-element run stays in bounds
    handle.check(L.lib.rtn_stem_pack(handle.raw, img.data_ptr(), L.RTN_BF16, xp.data_ptr(), L.RTN_BF16, B, H, W, Hp, Wp))
    wk, bk = Wt.pack_stem(c.w.float().numpy(), c.bias.float().numpy(), None, torch.bfloat16, DEV)
    wa, ba = Wt.pack_conv(c.w2a.float().numpy(), c.b2a.float().numpy(), None, torch.bfloat16, DEV)
    new = lambda ch, dt, fill: torch.full((B, H2, W2, ch), fill, dtype=dt, device=DEV)
    pool_a = new(64, torch.bfloat16, SENTINEL)
    handle.check(L.lib.rtn_stem_conv_pool(handle.raw, xp.data_ptr(), Hp, Wp, wk.data_ptr(), wk.shape[0], bk.data_ptr(), pool_a.data_ptr(), B, H, W))
    torch.cuda.synchronize()
    assert_equal(pool_a.cpu().double(), c.pool1, c.name + " pool1 (rtn_stem_conv_pool)")
    for with_a, with_idx in ((True, True), (True, False), (False, True)):
        pool_b, a_out, idx = new(64, torch.bfloat16, SENTINEL), new(64, torch.bfloat16, SENTINEL), new(64, torch.uint8, 99)
        handle.check(L.lib.rtn_stem_conv_pool_branch2a(handle.raw, xp.data_ptr(), Hp, Wp, wk.data_ptr(), wk.shape[0], bk.data_ptr(), pool_b.data_ptr(),
                                                       B, H, W, wa.data_ptr() if with_a else None, ba.data_ptr() if with_a else None,
                                                       a_out.data_ptr() if with_a else None, idx.data_ptr() if with_idx else None))
        torch.cuda.synchronize()
        what = "%s a_out=%d pool_idx=%d" % (c.name, with_a, with_idx)
        assert_equal(pool_b.cpu().double(), c.pool1, what + " pool1")
        if with_a:
            assert_equal(a_out.cpu().double(), c.a_out.want, what + " a_out")
        else:
            assert torch.all(a_out == SENTINEL)
        if with_idx:
            assert_equal(idx.cpu(), c.pool_idx, what + " pool_idx")
        else:
            assert torch.all(idx == 99)


@pytest.mark.parametrize("hw", [(17, 23), (16, 22)])
def test_indexed_pool_takes_the_first_maximum(pkg, handle, hw):
    """rtn_maxpool3x3s2_tfsame_fwd_idx on integers in [0, 3] (C = 64; odd extent: pad 1 / 1, even: 0 / 1): most windows hold their maximum more
    than once, and the recorded tap must be the first in kh * 3 + kw order among the taps inside the image."""
    L = pkg._lib
    c = X.case("pool/%dx%d" % hw)
    B, H, W, Cc = c.x.shape
    xd = c.x.to(torch.bfloat16).to(DEV).contiguous()
    out = torch.full(tuple(c.pool.shape), SENTINEL, dtype=torch.bfloat16, device=DEV)
    idx = torch.full(tuple(c.pool.shape), 99, dtype=torch.uint8, device=DEV)
    handle.check(L.lib.rtn_maxpool3x3s2_tfsame_fwd_idx(handle.raw, xd.data_ptr(), out.data_ptr(), idx.data_ptr(), L.RTN_BF16, B, H, W, Cc))
    torch.cuda.synchronize()
    assert_equal(out.cpu().double(), c.pool, c.name + " pooled")
    assert_equal(idx.cpu(), c.idx, c.name + " idx")


# ------------------------------------------------------------------------------------------------ 11. fp8
FP8_ENVS = [{"RTN_CONV_BN2": "256", "RTN_CONV_HALO": "2"}, {"RTN_CONV_BN2": "128", "RTN_CONV_HALO": "2"}, {"RTN_CONV_BN2": "64", "RTN_CONV_HALO": "2"},
            {"RTN_CONV_BN2": "256"}, {"RTN_CONV_BN2": "128"}, {"RTN_CONV_IMPL": "4"}]


@pytest.mark.parametrize("env,cin,cout", [(e, cin, cout) for e in FP8_ENVS for cin in (128, 256) for cout in (64, 256) if cout == 256 or "RTN_CONV_IMPL" not in e],
                         ids=lambda v: "-".join("%s%s" % (k[9:], x) for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_fp8_conv_code_distance_zero(pkg, handle, monkeypatch, env, cin, cout):
    """rtn_conv2d_fp8_fwd under the kernel-instance knob sets of test_fp8_conv_every_kernel_instance, and forced onto the persistent
    kernel's fp8 instance (which takes 129..256 output channels): integer operands times power-of-two scales are e4m3 codes, the
    accumulator times acc_scale is the exact integer sum, so the bf16 output and the e4m3 output EQUAL torch's cast of the float64
    reference - code distance 0 everywhere."""
    for kk, v in env.items():
        monkeypatch.setenv(kk, v)
    for out, relu in (("bf16", 1), ("e4m3", 0), ("bf16", 0), ("e4m3", 1)):
        launch_conv(pkg, handle, X.case("fp8/%d-%d/%s/relu%d" % (cin, cout, out, relu)), entry="fp8")
        if "RTN_CONV_IMPL" in env:
            assert last_impl(pkg, handle) == 4


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("layer,impl", [("1x1", 1), ("1x1", 2), ("1x1s2", 1), ("1x1s2", 2), ("3x3", 1), ("3x3", 2), ("3x3", 3)])
def test_bf16_conv_with_e4m3_output(pkg, handle, monkeypatch, layer, impl, relu):
    """rtn_conv2d_fwd_fp8out on generations 1 - 3 (the persistent generations decline a layer with e4m3 output): the e4m3 bytes EQUAL
    torch's cast of the float64 reference times out_scale."""
    monkeypatch.setenv("RTN_CONV_IMPL", str(impl))
    launch_conv(pkg, handle, X.case("fp8out/%s/relu%d" % (layer, relu)), entry="fp8out")
    assert last_impl(pkg, handle) == impl


def test_e4m3_output_never_runs_on_the_persistent_generations(pkg, handle, monkeypatch):
    """... and asking for generation 5 / 4 falls through to the kernels that have the e4m3 store (include/rtn.h says so)."""
    for layer, impl, takes in (("1x1", 5, 2), ("3x3", 4, 3)):
        monkeypatch.setenv("RTN_CONV_IMPL", str(impl))
        launch_conv(pkg, handle, X.case("fp8out/%s/relu1" % layer), entry="fp8out")
        assert last_impl(pkg, handle) == takes
