"""The quarter forms of rtn_bottleneck64_fwd (x_out_step / x_in_step = 2, include/rtn.h) and the engine variant built on them
(Engine.skip_unread_c2): stage 3 reads C2 at its even pixels only, so res2b stores and res2c computes only that quarter.  Nothing
is approximated - every check here is bit equality with the dense form."""
import ctypes as C
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096           # sentinel elements behind the *_elems of every compact buffer
SENTINEL = -7.0        # no output of a ReLU


def _block(L, B, H, W, seed):
    """Random operands of one identity block on the device, and a descriptor of the dense form with the next block's branch2a."""
    g = torch.Generator().manual_seed(seed)
    dev = torch.device("cuda")
    t16 = lambda t: t.to(torch.bfloat16).to(dev).contiguous()
    t = {"a": t16(torch.relu(torch.randn(B, H, W, 64, generator=g))), "x": t16(torch.relu(torch.randn(B, H, W, 256, generator=g))),
         "w2b": t16(torch.randn(64, 576, generator=g) / 24.0), "w2c": t16(torch.randn(256, 64, generator=g) / 8.0),
         "w2a": t16(torch.randn(64, 256, generator=g) / 16.0)}
    for name, n in (("b2b", 64), ("b2c", 256), ("b2a", 64)):
        t[name] = (torch.randn(n, generator=g) * 0.3).to(dev)
    return t


def _desc(L, t, B, H, W, x_in, x_out, a_out=None):
    d = L.BottleneckDesc()
    d.a_in, d.a_in_elems = t["a"].data_ptr(), t["a"].numel()
    d.x_in, d.x_in_elems = x_in.data_ptr(), x_in.numel()
    d.x_out, d.x_out_elems = x_out.data_ptr(), x_out.numel()
    d.w2b, d.b2b, d.w2c, d.b2c = t["w2b"].data_ptr(), t["b2b"].data_ptr(), t["w2c"].data_ptr(), t["b2c"].data_ptr()
    if a_out is not None:
        d.a_out, d.a_out_elems, d.w2a, d.b2a = a_out.data_ptr(), a_out.numel(), t["w2a"].data_ptr(), t["b2a"].data_ptr()
    d.batch, d.H, d.W, d.mid, d.dtype = B, H, W, 64, L.RTN_BF16
    return d


def _guarded(B, Hc, Wc):
    """A compact [B][Hc][Wc][256] tensor full of the sentinel, as a view of a buffer with GUARD more sentinel elements behind it."""
    n = B * Hc * Wc * 256
    raw = torch.full((n + GUARD,), SENTINEL, dtype=torch.bfloat16, device="cuda")
    return raw, raw[:n].view(B, Hc, Wc, 256)


# an even and an odd extent at batch 2 (odd: (H + 1) / 2 != H / 2 for rows and columns), each also with several strips per wave
# (RTN_BNECK_GRID: the cross-strip pipeline), tiny extents, and res2 of the benchmark's batch (8 x 800 x 1333 -> 200 x 334)
SHAPES = [(2, 40, 66, 0), (2, 41, 67, 0), (2, 40, 66, 2), (2, 41, 67, 3), (1, 1, 1, 0), (3, 5, 4, 0), (1, 2, 33, 0), (8, 200, 334, 0)]


@pytest.mark.parametrize("B,H,W,grid", SHAPES)
def test_quarter_forms_carry_the_bits_of_the_dense_form(pkg, handle, monkeypatch, B, H, W, grid):
    L = pkg._lib
    if grid:
        monkeypatch.setenv("RTN_BNECK_GRID", str(grid))
    run = lambda d: handle.check(L.lib.rtn_bottleneck64_fwd(handle.raw, C.byref(d)))
    t = _block(L, B, H, W, seed=H * 100 + W)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    dense_x = torch.full((B, H, W, 256), SENTINEL, dtype=torch.bfloat16, device="cuda")
    dense_a = torch.full((B, H, W, 64), SENTINEL, dtype=torch.bfloat16, device="cuda")
    run(_desc(L, t, B, H, W, t["x"], dense_x, dense_a))
    dense_nt = torch.full((B, H, W, 256), SENTINEL, dtype=torch.bfloat16, device="cuda")     # the form without a_out (res2c's)
    run(_desc(L, t, B, H, W, t["x"], dense_nt))
    torch.cuda.synchronize()
    assert torch.equal(dense_nt, dense_x) and not bool((dense_x == SENTINEL).any())
    for nt in ("1", "0"):                              # the compact stores with and without the streaming hint
        monkeypatch.setenv("RTN_BNECK_COMPACT_NT", nt)
        # ---- store-quarter: everything computed, a_out whole, x_out only at the even pixels
        raw, xq = _guarded(B, Hc, Wc)
        aq = torch.full((B, H, W, 64), SENTINEL, dtype=torch.bfloat16, device="cuda")
        d = _desc(L, t, B, H, W, t["x"], xq, aq)
        d.x_out_step = 2
        run(d)
        torch.cuda.synchronize()
        assert torch.equal(xq, dense_x[:, ::2, ::2]), "store-quarter x_out: %d elements differ" % int((xq != dense_x[:, ::2, ::2]).sum())
        assert torch.equal(aq, dense_a)
        assert bool((raw[xq.numel():] == SENTINEL).all()), "store-quarter wrote past x_out_elems"
        # ---- compute-quarter: only the even pixels computed, shortcut and output compact
        raw2, yq = _guarded(B, Hc, Wc)
        xin_raw, xin = _guarded(B, Hc, Wc)
        xin.copy_(t["x"][:, ::2, ::2])
        d = _desc(L, t, B, H, W, xin, yq)
        d.x_out_step = d.x_in_step = 2
        run(d)
        torch.cuda.synchronize()
        assert torch.equal(yq, dense_x[:, ::2, ::2]), "compute-quarter x_out: %d elements differ" % int((yq != dense_x[:, ::2, ::2]).sum())
        assert not bool((yq == SENTINEL).any())
        assert bool((raw2[yq.numel():] == SENTINEL).all()), "compute-quarter wrote past x_out_elems"
        assert bool((xin_raw[xin.numel():] == SENTINEL).all())
        if grid:                                       # several strips per wave: the result repeats
            first = yq.clone()
            for _ in range(3):
                run(d)
            torch.cuda.synchronize()
            assert torch.equal(first, yq)


def test_quarter_forms_reject_every_other_combination(pkg, handle):
    L = pkg._lib
    B, H, W = 2, 9, 13
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    t = _block(L, B, H, W, seed=5)
    call = lambda d: L.lib.rtn_bottleneck64_fwd(handle.raw, C.byref(d))
    xq, yq = _guarded(B, Hc, Wc)[1], _guarded(B, Hc, Wc)[1]
    xd = torch.empty(B, H, W, 256, dtype=torch.bfloat16, device="cuda")
    ad, h1 = [torch.empty(B, H, W, 64, dtype=torch.bfloat16, device="cuda") for _ in range(2)]

    def desc(xo, xi, tail, x_in=None, x_out=None):
        d = _desc(L, t, B, H, W, t["x"] if x_in is None else x_in, xd if x_out is None else x_out, ad if tail else None)
        d.x_out_step, d.x_in_step = xo, xi
        return d
    # the two forms themselves, and the steps that mean "dense"
    assert call(desc(2, 0, True, x_out=yq)) == 0 and call(desc(2, 1, True, x_out=yq)) == 0
    assert call(desc(2, 2, False, x_in=xq, x_out=yq)) == 0
    assert call(desc(1, 1, True)) == 0 and call(desc(0, 1, False)) == 0
    # x_in_step = 2 without x_out_step = 2
    assert call(desc(0, 2, False, x_in=xq)) == -1 and call(desc(1, 2, True, x_in=xq)) == -1
    # store-quarter without a_out, compute-quarter with it
    assert call(desc(2, 0, False, x_out=yq)) == -1 and call(desc(2, 2, True, x_in=xq, x_out=yq)) == -1
    # steps other than 0, 1, 2
    assert call(desc(3, 0, True)) == -1 and call(desc(2, -2, True, x_out=yq)) == -1 and call(desc(4, 4, False)) == -1
    # a step with h1_out
    for d in (desc(2, 0, True, x_out=yq), desc(2, 2, False, x_in=xq, x_out=yq)):
        d.h1_out, d.h1_out_elems = h1.data_ptr(), h1.numel()
        assert call(d) == -1
    # a step with the projection form
    wcat = torch.zeros(256, 128, dtype=torch.bfloat16, device="cuda")
    for d in (desc(2, 0, True, x_out=yq), desc(2, 2, False, x_in=xq, x_out=yq)):
        d.p_in, d.p_in_elems = t["a"].data_ptr(), t["a"].numel()
        d.w2c, d.wproj, d.w2c_ld = wcat.data_ptr(), wcat.data_ptr() + 128, 128
        assert call(d) == -1
    # the *_elems of a stepped tensor describe the compact tensor
    d = desc(2, 0, True, x_out=yq)
    d.x_out_elems = yq.numel() - 1
    assert call(d) == -4
    d = desc(2, 2, False, x_in=xq, x_out=yq)
    d.x_in_elems = xq.numel() - 1
    assert call(d) == -4
    torch.cuda.synchronize()


def _engine(pkg, backbone="resnet50"):
    E = importlib.import_module(pkg.__name__ + ".engine")
    Wt = importlib.import_module(pkg.__name__ + ".weights")
    state = Wt.init_state(backbone, 1, 9, seed=0, randomize_bn=True, cls_bias=-2.0, tame=True)
    eng = E.Engine(backbone, 1, 9, dtype="bf16", device=0)
    eng.load_state(state)
    return eng


# C2 is 40 x 56 and 37 x 53; ResNet-101 has the same stage 2 and takes the same path
@pytest.mark.parametrize("backbone,canvas,in_flight", [("resnet50", (160, 224), 1), ("resnet50", (146, 210), 1), ("resnet50", (160, 224), 2),
                                                       ("resnet50", (146, 210), 2), ("resnet101", (146, 210), 2)])
def test_detect_is_the_same_with_and_without_the_unread_quarters(pkg, backbone, canvas, in_flight):
    eng = _engine(pkg, backbone)
    B = 2
    g = torch.Generator().manual_seed(canvas[1])
    xs = [(torch.rand(B, canvas[0], canvas[1], 3, generator=g) * 2 - 1).cuda() for _ in range(3)]
    eng.in_flight = in_flight
    got = {}
    for knob in (False, True):
        eng.join()
        torch.cuda.synchronize()
        eng.skip_unread_c2 = knob
        outs = []
        for x in xs:
            boxes, scores, labels = eng.detect(x)
            if in_flight > 1:
                si = eng.last_slot
                plan = eng._plan(B, canvas[0], canvas[1], slot=si + 1)
                stream = eng.slot_stream(si)
            else:
                plan, stream = eng._plan(B, canvas[0], canvas[1]), torch.cuda.current_stream()
            with torch.cuda.stream(stream):
                outs.append([v.clone() for v in (boxes, scores, labels, plan["regression"], plan["classification"])])
        eng.join()
        torch.cuda.synchronize()
        got[knob] = outs
        # the op list detect() ran: with the knob, the two stepped bottleneck ops and a stride-1 res3a_branch2a
        ops = eng._variant(plan, eng._fused(private=True))["ops"]
        steps = [(op[3]["x_in_step"], op[3]["x_out_step"]) for op in ops if op[0] == "bneck" and not op[3].get("proj")]
        r3a = [op for op in ops if op[0] == "conv" and op[2] == "res3a_branch2a"][0]
        if knob:
            assert eng._fused(private=True)[6] == 1 and eng._fused()[6] == 0
            assert steps == [(1, 2), (2, 2)] and r3a[3]["stride"] == 1 and int(r3a[1].sy) == 1
        else:
            assert steps == [(1, 1), (1, 1)] and r3a[3]["stride"] == 2
        assert [op[0] for op in ops] == [op[0] for op in eng.active_ops(plan)]       # the same launches, one for one
    assert int((got[True][0][1] >= 0).sum()) > 0                   # there are detections to compare
    for a, b in zip(got[False], got[True]):
        for name, u, v in zip(("boxes", "scores", "labels", "regression", "classification"), a, b):
            assert torch.equal(u, v), name
    # forward() itself keeps C2 whole: its variant is the dense one, whatever the knob
    reg, cls = eng.forward(xs[-1])
    torch.cuda.synchronize()
    assert torch.equal(reg, got[True][-1][3]) and torch.equal(cls, got[True][-1][4])
    assert all(op[3]["x_out_step"] == 1 for op in eng.active_ops(eng._plan(B, canvas[0], canvas[1])) if op[0] == "bneck" and not op[3].get("proj"))
