"""GPU tests of frozen-layer training: the backward pruned to what the trainable layers need (trainer.Trainer(trainable=...)), the
inference form of the stem / 64-channel blocks in its training forward, and the optimizer over the trainable element ranges
(rtn_sumsq_ranges, rtn_adam_clipnorm_step_ranges[_pertensor]).

The yardstick of the pruned step is the full step with the frozen layers masked by gscale (the path a non-trainable layer took
before): same losses, same bits in every trainable weight and bias gradient."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "retinanet-for-table-detection_amd"
CANVAS = (256, 384)


def mods(pkg):
    return [importlib.import_module(pkg.__name__ + "." + m) for m in ("engine", "weights", "trainer", "_lib")]


def make_batch(B, seed, canvas=CANVAS):
    g = torch.Generator().manual_seed(seed)
    raw = torch.clamp(torch.empty(B, canvas[0], canvas[1], 3).exponential_(1 / 12.0, generator=g) *
                      torch.rand(B, canvas[0], canvas[1], 3, generator=g), 0, 255).round().to(torch.uint8)
    x = R.preprocess_custom_tf(raw.numpy())
    anchors = R.anchors_for_shape(canvas + (3,))
    rng = np.random.RandomState(seed)
    gts = []
    for _ in range(B):
        n = rng.randint(1, 4)
        w, h = rng.uniform(40, canvas[1] / 2, n), rng.uniform(30, canvas[0] / 2, n)
        x1, y1 = rng.uniform(0, canvas[1] - w), rng.uniform(0, canvas[0] - h)
        gts.append(np.stack([x1, y1, x1 + w, y1 + h], axis=1))
    reg, lab = R.anchor_targets(anchors, [canvas] * B, gts, [np.zeros(len(g_)) for g_ in gts], 1)
    return torch.as_tensor(x).cuda(), torch.as_tensor(reg).cuda(), torch.as_tensor(lab).cuda()


def is_backbone(name):
    return name == "conv1" or name.startswith("res")


FROZEN = {"backbone": is_backbone, "stem_res2": lambda n: n == "conv1" or n.startswith("res2")}


def mask_frozen(tr, frozen):
    """What a non-trainable layer got before the pruned backward: its gscale slots zeroed, the full backward still run."""
    for name, lo in tr.eng.layout.items():
        if frozen(name):
            tr.gscale[lo["woff"]:lo["woff"] + lo["rows"] * lo["K"]] = 0
            tr.gscale[tr.NW + lo["boff"]:tr.NW + lo["boff"] + lo["rows"]] = 0


def layer_slices(tr, name):
    lo = tr.eng.layout[name]
    return (slice(lo["woff"], lo["woff"] + lo["rows"] * lo["K"]), slice(tr.NW + lo["boff"], tr.NW + lo["boff"] + lo["rows"]))


def frozen_mask(tr, frozen):
    m = torch.zeros(tr.NW + tr.NB, dtype=torch.bool, device=tr.grad.device)
    for name in tr.eng.layout:
        if frozen(name):
            for sl in layer_slices(tr, name):
                m[sl] = True
    return m


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("case", ["backbone", "stem_res2"])
def test_pruned_backward_matches_masked_full_backward(pkg, dtype, case):
    E, Wt, T, L = mods(pkg)
    frozen = FROZEN[case]
    state = Wt.init_state("resnet50", 1, 9, seed=4, randomize_bn=True, cls_bias=-2.0, tame=True)
    eng = E.Engine("resnet50", 1, 9, dtype=dtype)
    eng.load_state(state)
    trainable = frozenset(n for n in eng.layout if not frozen(n))
    x, reg, lab = make_batch(2, seed=41)
    ref = T.Trainer(eng, lr=1e-4, clipnorm=0.001)
    mask_frozen(ref, frozen)
    s_ref = ref.forward_backward(x, reg, lab).clone()
    torch.cuda.synchronize()
    full_key = ref.fwd_key
    tr = T.Trainer(eng, lr=1e-4, clipnorm=0.001, trainable=trainable)
    tr.record_impls = True
    s = tr.forward_backward(x, reg, lab).clone()
    torch.cuda.synchronize()
    # ---- the forward: the same bits, in the inference form below the trainable layers
    assert torch.equal(s, s_ref), (s, s_ref)
    key = tr.fwd_key
    assert key[5] == 0, key                                  # no pool taps recorded
    if dtype == "bf16":
        assert full_key[2] == 2 and full_key[5] == 1 and key[2] == 1, (full_key, key)
        assert key[:2] == full_key[:2] and key[3:5] == full_key[3:5]
    # ---- the backward plan: nothing for the frozen layers, no data gradient below the lowest trainable layer
    bp = tr.bplans[(2,) + CANVAS]
    kinds = [b[0] for b in bp["bops"]]
    assert "poolbwd" not in kinds
    launched = set(tr.impls)
    for name in eng.layout:
        if frozen(name):
            assert ("wgrad", name) not in launched and ("dgrad", name) not in launched, name
        else:
            assert ("wgrad", name) in launched, name
    if case == "backbone":
        for name in ("C3_reduced", "C4_reduced", "C5_reduced", "P6"):
            assert ("dgrad", name) not in launched, name
    else:                                                     # the backward stops at res3a's inputs
        assert ("dgrad", "res3a_branch2a") not in launched and ("dgrad", "res3a_branch1") not in launched
        assert ("dgrad", "res3a_branch2b") in launched
    n_full = len(ref.bplans[(2,) + CANVAS]["bops"])
    assert len(bp["bops"]) < n_full
    # ---- every trainable weight and bias gradient: the same bits
    for name in sorted(trainable):
        for sl in layer_slices(tr, name):
            a, b = tr.grad[sl], ref.grad[sl]
            assert torch.equal(a, b), "%s: max diff %.3e" % (name, float((a - b).abs().max()))


def adam_ranges_f64(master, m, v, grad, gscale, live, step, lr=1e-4, b1=0.9, b2=0.999, eps=1e-7, clipnorm=0.001):
    g = (grad.double() * gscale.double())[live]
    norm = math.sqrt(float((g * g).sum()))
    c = clipnorm / norm if norm > clipnorm else 1.0
    g = g * c
    m[live] = b1 * m[live] + (1 - b1) * g
    v[live] = b2 * v[live] + (1 - b2) * g * g
    lr_t = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
    master[live] = master[live] - lr_t * m[live] / (torch.sqrt(v[live]) + eps)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_frozen_steps_leave_frozen_slots_and_repeat(pkg, dtype):
    E, Wt, T, L = mods(pkg)
    state = Wt.init_state("resnet50", 1, 9, seed=6, randomize_bn=True, cls_bias=-2.0, tame=True)
    batches = [make_batch(2, seed=50 + i) for i in range(3)]
    runs = []
    for run in range(2):
        eng = E.Engine("resnet50", 1, 9, dtype=dtype)
        eng.load_state(state)
        tr = T.Trainer(eng, lr=1e-4, clipnorm=0.001, trainable=[n for n in eng.layout if not is_backbone(n)])
        fz = frozen_mask(tr, is_backbone)
        before = {k: t.clone() for k, t in (("master", tr.master), ("m", tr.m), ("v", tr.v), ("wflat", eng.wflat), ("bflat", eng.bflat))}
        wfz = torch.zeros(tr.NW, dtype=torch.bool, device=fz.device)
        wfz[:] = fz[:tr.NW]
        bfz = fz[tr.NW:]
        live = ~fz
        # float64 restatement on the device's own gradients; live = the trainable tensors' slots
        ref = {"master": tr.master.double().cpu(), "m": torch.zeros(tr.NW + tr.NB, dtype=torch.float64),
               "v": torch.zeros(tr.NW + tr.NB, dtype=torch.float64)}
        losses = []
        for step, (x, reg, lab) in enumerate(batches, 1):
            tr.forward_backward(x, reg, lab)
            torch.cuda.synchronize()
            adam_ranges_f64(ref["master"], ref["m"], ref["v"], tr.grad.cpu(), tr.gscale.cpu(), live.cpu(), step)
            tr.optimizer_step()
            losses.append(tr.norm_sums.cpu().numpy().tolist())
        torch.cuda.synchronize()
        for k, full, sel in (("master", tr.master, fz), ("m", tr.m, fz), ("v", tr.v, fz), ("wflat", eng.wflat, wfz), ("bflat", eng.bflat, bfz)):
            assert torch.equal(full[sel], before[k][sel]), "%s: a frozen slot changed" % k
        move_got = (tr.master.double().cpu() - before["master"].double().cpu())[live.cpu()]
        move_want = (ref["master"] - before["master"].double().cpu())[live.cpu()]
        assert float(move_want.abs().max()) > 1e-5                     # the trainable weights did move
        assert float((move_got - move_want).abs().max()) <= 0.05 * 1e-4
        # the forward weights of the trainable layers were re-emitted from the master copy
        lo = eng.layout["pyramid_classification_0"]
        sl = slice(lo["woff"], lo["woff"] + lo["rows"] * lo["K"])
        want_fwd = (tr.master[sl] * tr.fold[sl]).to(eng.wflat.dtype)
        assert torch.equal(eng.wflat[sl], want_fwd)
        runs.append((losses, tr.master.clone(), tr.m.clone(), tr.v.clone(), eng.wflat.clone()))
    a, b = runs
    assert a[0] == b[0]
    for i in range(1, 5):
        assert torch.equal(a[i], b[i]), "run-to-run difference in item %d" % i


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("global_clip", [True, False])
def test_trainable_none_equals_every_layer_named(pkg, dtype, global_clip):
    """One optimizer family: Trainer(trainable=None) and Trainer(trainable=<every layer>) mean the same thing and, from the same state
    and the same three batches, end with the same bits in the parameters, the moments and the forward weights."""
    E, Wt, T, L = mods(pkg)
    state = Wt.init_state("resnet50", 1, 9, seed=6, randomize_bn=True, cls_bias=-2.0, tame=True)
    batches = [make_batch(2, seed=50 + i) for i in range(3)]
    runs = []
    for named in (False, True):
        eng = E.Engine("resnet50", 1, 9, dtype=dtype)
        eng.load_state(state)
        tr = T.Trainer(eng, lr=1e-4, clipnorm=0.001, global_clip=global_clip, trainable=frozenset(eng.layout) if named else None)
        assert (tr.trainable is None) == (not named)
        w0 = tr.master.clone()
        losses = []
        for x, reg, lab in batches:
            tr.train_on_batch(x, reg, lab)
            losses.append(tr.norm_sums.cpu().numpy().tolist())
        torch.cuda.synchronize()
        assert not torch.equal(tr.master, w0)                         # the steps did move the weights
        runs.append((losses, {"master": tr.master.clone(), "m": tr.m.clone(), "v": tr.v.clone(), "wflat": eng.wflat.clone(),
                              "bflat": eng.bflat.clone()}))
    (loss_a, a), (loss_b, b) = runs
    assert loss_a == loss_b
    for k in a:
        assert torch.equal(a[k], b[k]), "%s differs between trainable=None and every layer named" % k


def random_ranges(rng, n):
    """Sorted, disjoint ranges inside [0, n): empty, one-element, unaligned and long ones, with gaps."""
    out, pos = [], int(rng.randint(0, 5))
    kinds = ["empty", "one", "short", "long", "aligned"]
    while pos < n - 10:
        k = kinds[rng.randint(len(kinds))]
        ln = {"empty": 0, "one": 1, "short": int(rng.randint(2, 9)), "long": int(rng.randint(100, 3000)),
              "aligned": 4 * int(rng.randint(1, 200))}[k]
        if k == "aligned":
            pos += (-pos) % 4
        end = min(n, pos + ln)
        out.append((pos, end))
        pos = end + int(rng.randint(0, 40)) * (rng.rand() < 0.7)
    return out


@pytest.mark.parametrize("fwd", ["bf16", "f32"])
@pytest.mark.parametrize("shift", [0, 1])
def test_range_kernels_against_float64(pkg, handle, fwd, shift):
    """rtn_sumsq_ranges (total and per range), rtn_adam_clipnorm_step_ranges and _pertensor on random ranges; every slot outside
    the ranges holds its sentinel afterwards.  shift=1 offsets every buffer by one element (the element-wise path)."""
    E, Wt, T, L = mods(pkg)
    rng = np.random.RandomState(7 + shift)
    n = 20011
    rs = random_ranges(rng, n)
    assert any(a == b for a, b in rs) and any(b - a == 1 for a, b in rs) and any(a % 4 for a, b in rs)
    tab, nr, span = L.ranges_table(rs, "cuda")
    inside = torch.zeros(n, dtype=torch.bool)
    for a, b in rs:
        inside[a:b] = True
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(shift)

    def buf(vals, dt=torch.float32):
        t = torch.empty(n + 4, dtype=dt, device=dev)
        v = t[shift:shift + n]
        v.copy_(vals.to(dt))
        return t, v
    SENT = -12345.0
    gr = torch.randn(n, generator=g) * 1e-3
    gs = torch.where(torch.rand(n, generator=g) < 0.1, torch.zeros(n), torch.rand(n, generator=g) + 0.5)
    fo = torch.rand(n, generator=g) + 0.5
    w0 = torch.randn(n, generator=g)
    m0 = torch.randn(n, generator=g) * 1e-4
    v0 = torch.rand(n, generator=g) * 1e-8
    (_, g_d), (_, s_d), (_, f_d) = buf(gr), buf(gs), buf(fo)
    ins = inside
    sent = torch.full((n,), SENT)
    (_, w_d), (_, m_d), (_, v_d) = buf(torch.where(ins, w0, sent)), buf(torch.where(ins, m0, sent)), buf(torch.where(ins, v0, sent))
    fdt = torch.bfloat16 if fwd == "bf16" else torch.float32
    (_, wf_d) = buf(torch.full((n,), 7.0), fdt)
    # g / gscale / fold outside the ranges must not be read: poison them
    g_d[~ins.cuda()] = float("nan")
    s_d[~ins.cuda()] = float("nan")
    f_d[~ins.cuda()] = float("nan")
    ws = torch.empty(L.lib.rtn_sumsq_workspace_bytes(), dtype=torch.uint8, device=dev)
    tot = torch.zeros(1, dtype=torch.float64, device=dev)
    each = torch.zeros(nr, dtype=torch.float64, device=dev)
    handle.check(L.lib.rtn_sumsq_ranges(handle.raw, g_d.data_ptr(), s_d.data_ptr(), n, tab.data_ptr(), nr, span, tot.data_ptr(),
                                        each.data_ptr(), ws.data_ptr(), ws.numel()))
    torch.cuda.synchronize()
    a = (gr * gs).double()                                        # the product in f32, as the kernels form it
    want_each = torch.tensor([float((a[x:y] ** 2).sum()) for x, y in rs], dtype=torch.float64)
    want_tot = float(want_each.sum())
    assert abs(float(tot) - want_tot) <= 1e-12 * want_tot
    assert torch.allclose(each.cpu(), want_each, rtol=1e-12, atol=0)
    tot2 = torch.zeros(1, dtype=torch.float64, device=dev)           # deterministic: the same bits again
    handle.check(L.lib.rtn_sumsq_ranges(handle.raw, g_d.data_ptr(), s_d.data_ptr(), n, tab.data_ptr(), nr, span, tot2.data_ptr(),
                                        None, ws.data_ptr(), ws.numel()))
    torch.cuda.synchronize()
    assert float(tot2) == float(tot)
    step, lr, b1, b2, eps, clip = 3, 1e-3, 0.9, 0.999, 1e-7, 0.01
    lr_t = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
    for per in (False, True):
        w_d.copy_(torch.where(ins, w0, sent).to(dev)); m_d.copy_(torch.where(ins, m0, sent).to(dev))
        v_d.copy_(torch.where(ins, v0, sent).to(dev)); wf_d.fill_(7.0)
        args = (handle.raw, w_d.data_ptr(), m_d.data_ptr(), v_d.data_ptr(), g_d.data_ptr(), s_d.data_ptr(), f_d.data_ptr(),
                wf_d.data_ptr(), L.RTN_BF16 if fwd == "bf16" else L.RTN_F32, n, tab.data_ptr(), nr, span, step, lr, b1, b2, eps)
        if per:
            handle.check(L.lib.rtn_adam_clipnorm_step_ranges_pertensor(*args, each.data_ptr(), clip, 1.0))
        else:
            handle.check(L.lib.rtn_adam_clipnorm_step_ranges(*args, tot.data_ptr(), clip, 1.0))
        torch.cuda.synchronize()
        c = torch.ones(n, dtype=torch.float64)
        for r, (x, y) in enumerate(rs):
            nrm = math.sqrt(float(want_each[r] if per else want_tot))
            c[x:y] = clip / nrm if nrm > clip else 1.0
        gg = a * c
        f32 = lambda v_: float(np.float32(v_))
        b1f, b2f = f32(b1), f32(b2)                                   # the kernels' constants: float b1, b2 and float 1 - b
        m1 = b1f * m0.double() + f32(np.float32(1) - np.float32(b1)) * gg
        v1 = b2f * v0.double() + f32(np.float32(1) - np.float32(b2)) * gg * gg
        w1 = w0.double() - lr_t * m1 / (torch.sqrt(v1) + eps)
        wc, mc, vc, fc = w_d.cpu(), m_d.cpu(), v_d.cpu(), wf_d.float().cpu()
        assert torch.all(wc[~ins] == SENT) and torch.all(mc[~ins] == SENT) and torch.all(vc[~ins] == SENT)
        assert torch.all(fc[~ins] == 7.0)
        assert float((mc[ins].double() - m1[ins]).abs().max()) <= 1e-6 * float(m1[ins].abs().max())
        assert float((vc[ins].double() - v1[ins]).abs().max()) <= 1e-6 * float(v1[ins].abs().max())
        assert float((wc[ins].double() - w1[ins]).abs().max()) <= 1e-3 * lr
        want_f = (wc * fo).to(fdt).float()
        assert torch.equal(fc[ins], want_f[ins])
    # no ranges: a no-op that still writes the (zero) norm
    tot.fill_(5.0)
    handle.check(L.lib.rtn_sumsq_ranges(handle.raw, g_d.data_ptr(), s_d.data_ptr(), n, None, 0, 0, tot.data_ptr(), None,
                                        ws.data_ptr(), ws.numel()))
    torch.cuda.synchronize()
    assert float(tot) == 0.0


def test_fully_frozen_and_set_trainable(pkg):
    """freeze(model) on the whole model: the loss is still returned, no backward kernel runs, no weight changes.  A trainer follows
    set_trainable(): new plans, the full backward back for None."""
    E, Wt, T, L = mods(pkg)
    state = Wt.init_state("resnet50", 1, 9, seed=2, randomize_bn=True, cls_bias=-2.0, tame=True)
    eng = E.Engine("resnet50", 1, 9, dtype="bf16")
    eng.load_state(state)
    x, reg, lab = make_batch(2, seed=61)
    tr = T.Trainer(eng, lr=1e-4, clipnorm=0.001, trainable=())
    w0, b0, m0 = eng.wflat.clone(), eng.bflat.clone(), tr.master.clone()
    tr.record_impls = True
    total, r_loss, c_loss = tr.train_on_batch(x, reg, lab)
    torch.cuda.synchronize()
    assert np.isfinite(total) and total > 0 and not tr.impls
    assert tr.bplans[(2,) + CANVAS]["bops"] == []
    assert torch.equal(eng.wflat, w0) and torch.equal(eng.bflat, b0) and torch.equal(tr.master, m0)
    full = T.Trainer(eng, lr=1e-4, clipnorm=0.001)
    t_full = full.forward_backward(x, reg, lab).clone()
    tr.set_trainable(None)
    assert tr.bplans == {}
    t_back = tr.forward_backward(x, reg, lab).clone()
    torch.cuda.synchronize()
    assert torch.equal(t_full, t_back) and torch.equal(tr.grad, full.grad)
    assert len(tr.bplans[(2,) + CANVAS]["bops"]) == len(full.bplans[(2,) + CANVAS]["bops"])


def _model_mods():
    sys.path.insert(0, os.path.join(ROOT, PKG))
    try:
        for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
            del sys.modules[k]
        return importlib.import_module("model.defineModel"), importlib.import_module("model.utils")
    finally:
        sys.path.pop(0)


def test_fit_generator_with_frozen_backbone_trains_the_heads_only(pkg):
    D, U = _model_mods()
    model = D.resnet_retinanet(1, modifier=U.freeze)
    model.compile(loss={'regression': None, 'classification': None}, optimizer=D.Adam(lr=1e-4, clipnorm=0.001))
    before = {k: np.array(v, copy=True) for k, v in model.get_state().items()}
    batches = []
    for i in range(2):
        x, reg, lab = make_batch(2, seed=70 + i, canvas=(128, 192))
        batches.append((x.cpu().numpy(), [reg.cpu().numpy(), lab.cpu().numpy()]))
    hist = model.fit_generator(batches, steps_per_epoch=2, epochs=1, verbose=0)
    assert np.isfinite(hist.history["loss"][0])
    after = model.get_state()
    for name in ("conv1", "res2a_branch2a", "res3d_branch2b", "res5c_branch2c"):
        assert np.array_equal(after[name + "/kernel"], before[name + "/kernel"]), name
    for name in ("pyramid_classification", "pyramid_regression_0", "P3", "C5_reduced"):
        assert not np.array_equal(after[name + "/kernel"], before[name + "/kernel"]), name
    assert not np.array_equal(after["P3/bias"], before["P3/bias"])
    # compile() re-reads the flags: the whole model trains from here on
    for l in model.backbone_view().layers:
        l.trainable = True
    model.compile(loss={'regression': None, 'classification': None}, optimizer=D.Adam(lr=1e-4, clipnorm=0.001))
    assert model._get_trainer().trainable is None
    model.fit_generator(batches[:1], steps_per_epoch=1, epochs=1, verbose=0)
    assert not np.array_equal(model.get_state()["res2a_branch2a/kernel"], before["res2a_branch2a/kernel"])


def test_full_size_frozen_backbone_step(pkg):
    """One pruned step at the benchmark canvas (800 x 1333, batch 2, bf16) against the masked full step: same bits."""
    E, Wt, T, L = mods(pkg)
    canvas = (800, 1333)
    state = Wt.init_state("resnet50", 1, 9, seed=8, randomize_bn=True, cls_bias=-2.0, tame=True)
    eng = E.Engine("resnet50", 1, 9, dtype="bf16")
    eng.load_state(state)
    x, reg, lab = make_batch(2, seed=81, canvas=canvas)
    ref = T.Trainer(eng, lr=1e-4, clipnorm=0.001)
    mask_frozen(ref, is_backbone)
    s_ref = ref.forward_backward(x, reg, lab).clone()
    g_ref = ref.grad.clone()
    torch.cuda.synchronize()
    ref.bplans = {}
    del ref
    tr = T.Trainer(eng, lr=1e-4, clipnorm=0.001, trainable=[n for n in eng.layout if not is_backbone(n)])
    s = tr.forward_backward(x, reg, lab).clone()
    torch.cuda.synchronize()
    assert torch.equal(s, s_ref)
    assert tr.fwd_key[2] == 1 and tr.fwd_key[5] == 0
    for name in eng.layout:
        if not is_backbone(name):
            for sl in layer_slices(tr, name):
                assert torch.equal(tr.grad[sl], g_ref[sl]), name
