"""GPU: every copy derived from the trained f32 master weights is the copy a reload would build, bit for bit.

An optimizer step rewrites the master copy (Trainer.master) and, from it, the forward weights (Engine.wflat / bflat, emitted by the
Adam launch itself), the backward-data filters (Trainer.wd, rtn_pack_dgrad_weights_multi over a cached table of the trainable
layers), the K-concatenated filters of the folded shortcuts (Engine._dual_weights) and the e4m3 filters with their scales
(Engine._fp8_weights); plans built before the step keep descriptors into all of them.  A checkpoint holds Trainer.get_state().

"Fresh" below is always a NEW Engine with load_state(Trainer.get_state()) - and a new Trainer on it where the training side is
compared - so every copy on that side is built from scratch out of what the file would hold.  Equality is exact by construction:
fold_bn and the Adam kernel both round master_f32 * fold_f32 to the path dtype, the master copy travels through NumPy f32
unchanged, and two engines with the same weights and batch give the same bits (test_gpu_train.py
test_training_steps_repeat_bit_for_bit).  All comparisons are on the bit patterns; none has a tolerance.

lr is 1e-3: at 1e-4 one Adam move is under half a bf16 ulp of a typical filter element and the controls would be weak."""
import functools

import pytest
import torch

from test_gpu_train import CANVAS, LAYERS, make_batch, mods

pytestmark = pytest.mark.gpu
LR, CLIPNORM, STEPS, B = 1e-3, 0.001, 3, 2
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}


def same(a, b):
    """Bit equality of two tensors (floats through their integer views: -0.0 is not 0.0, a NaN equals itself)."""
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(_INT.get(a.dtype, a.dtype)), b.view(_INT.get(b.dtype, b.dtype)))


@functools.lru_cache(maxsize=None)
def start_state(Wt):
    """The state every case starts from, built once (read only)."""
    return Wt.init_state("resnet50", 1, 9, seed=0, randomize_bn=True, cls_bias=-2.0, tame=True)


@functools.lru_cache(maxsize=None)
def batch(seed):
    """(images, regression targets, label targets) of test_gpu_train.make_batch on the device; shared and never written."""
    return tuple(torch.as_tensor(t).cuda() for t in make_batch(B, seed=seed))


def new_engine(E, state, dtype):
    eng = E.Engine("resnet50", 1, 9, dtype=dtype)
    eng.load_state(state)
    return eng


def new_trainer(T, eng, **kw):
    return T.Trainer(eng, lr=LR, clipnorm=CLIPNORM, **kw)


def train(tr, seeds):
    for seed in seeds:
        loss = tr.train_on_batch(*batch(seed))
        assert loss[0] == loss[0] and loss[0] > 0, loss


def layer_slice(eng, flat, name):
    lo = eng.layout[name]
    return flat[lo["woff"]:lo["woff"] + lo["rows"] * lo["K"]]


def assert_copies_match_fresh(E, T, tr, what):
    """(a) of the file: forward weights, master / fold / gradient scale and every backward filter of the live side against an engine
    and a trainer built from the live side's saved state.  Returns (fresh engine, fresh trainer)."""
    torch.cuda.synchronize()
    fresh = new_engine(E, tr.get_state(), tr.eng.dtype)
    ftr = new_trainer(T, fresh, global_clip=tr.global_clip)            # every layer trainable: its filters are all packed at once
    torch.cuda.synchronize()
    for attr in ("wflat", "bflat"):
        assert same(getattr(tr.eng, attr), getattr(fresh, attr)), "%s: Engine.%s is not what the saved state packs to" % (what, attr)
    for attr in ("master", "fold", "gscale"):
        assert same(getattr(tr, attr), getattr(ftr, attr)), "%s: Trainer.%s differs from a reload" % (what, attr)
    assert list(tr.wd) == list(ftr.wd) and len(tr.wd) == len(tr.eng.layout) - 1
    stale = [name for name in tr.wd if not same(tr.wd[name], ftr.wd[name])]
    assert not stale, "%s: backward filters that are not the repack of the forward weights: %s" % (what, stale)
    return fresh, ftr


# ------------------------------------------------------------------ (a) master, forward and backward weights
@pytest.mark.parametrize("global_clip", [True, False], ids=["global", "pertensor"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_copies_after_steps_are_the_reloaded_ones(pkg, dtype, global_clip):
    E, Wt, T = mods(pkg)
    tr = new_trainer(T, new_engine(E, start_state(Wt), dtype), global_clip=global_clip)
    train(tr, (41, 42, 43)[:STEPS])
    assert_copies_match_fresh(E, T, tr, "%s, %s clip, %d steps" % (dtype, "global" if global_clip else "per-tensor", STEPS))


# ------------------------------------------------------------------ (b) the controls: (a) cannot pass on weights that never moved
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_every_step_moves_the_forward_weights(pkg, dtype):
    """Adam moves every element with |g| >> eps by about lr = 1e-3, several bf16 ulps of a filter element: each audited layer's slice
    of the forward weights changes bits in each step, and the state saved one step earlier is another model."""
    E, Wt, T = mods(pkg)
    eng = new_engine(E, start_state(Wt), dtype)
    tr = new_trainer(T, eng)
    before = eng.wflat.clone()
    for step, seed in enumerate((41, 42, 43)[:STEPS]):
        if step == STEPS - 1:
            previous = tr.get_state()                      # what a checkpoint one step before the last holds
        train(tr, (seed,))
        now = eng.wflat.clone()
        still = [name for name in LAYERS if same(layer_slice(eng, before, name), layer_slice(eng, now, name))]
        assert not still, "step %d left the forward weights of %s as they were" % (step + 1, still)
        before = now
    x = batch(41)[0]
    live = [t.clone() for t in eng.forward(x)]
    old = [t.clone() for t in new_engine(E, previous, dtype).forward(x)]
    torch.cuda.synchronize()
    assert not same(live[0], old[0]) and not same(live[1], old[1]), "a model one step stale gives the live model's outputs"


# ------------------------------------------------------------------ (c) every inference path, plans built before training
def infer(eng, xs):
    """forward(xs[0]) and detect() of every page of xs, cloned once the device is idle (in_flight > 1: the detect calls overlap, each
    on a buffer set of its own)."""
    assert len(xs) <= max(1, eng.in_flight)
    out = list(eng.forward(xs[0]))
    torch.cuda.synchronize()
    out = [t.clone() for t in out]
    views = [eng.detect(x) for x in xs]
    eng.join()
    torch.cuda.synchronize()
    return out + [t.clone() for v in views for t in v]


@pytest.mark.parametrize("dtype,in_flight", [pytest.param("bf16", 1, id="bf16"), pytest.param("bf16", 2, id="bf16-two-in-flight"),
                                             pytest.param("f32", 1, id="f32")])
def test_plans_built_before_training_run_the_trained_weights(pkg, dtype, in_flight):
    E, Wt, T = mods(pkg)
    eng = new_engine(E, start_state(Wt), dtype)
    eng.in_flight = in_flight
    xs = [batch(51 + i)[0] for i in range(in_flight)]
    first = infer(eng, xs)                                 # builds the inference variants, their descriptors and the dual filters
    H, W = CANVAS
    fwd_plan = eng._plan(B, H, W)
    det_plans = [fwd_plan] if in_flight == 1 else [eng._plan(B, H, W, slot=s + 1) for s in range(in_flight)]
    variants = [(fwd_plan, False)] + [(p, True) for p in det_plans]
    built = [dict(p["variants"]) for p, _ in variants]
    tr = new_trainer(T, eng)
    train(tr, (41, 42, 43)[:STEPS])
    got = infer(eng, xs)
    fresh = new_engine(E, tr.get_state(), dtype)
    want = infer(fresh, xs[:1])
    for x in xs[1:]:                                       # the reloaded engine runs one batch at a time
        views = fresh.detect(x)
        torch.cuda.synchronize()
        want += [t.clone() for t in views]
    names = ["regression", "classification"] + ["%s of detect call %d" % (n, i) for i in range(in_flight) for n in ("boxes", "scores", "labels")]
    assert len(got) == len(want) == len(first) == len(names)
    for name, g, w in zip(names, got, want):
        assert same(g, w), "%s after training differs from a reloaded engine's" % name
    for i in [0, 1] + [3 + 3 * k for k in range(in_flight)]:      # the outputs and every call's scores moved with the weights
        assert int((got[i] >= 0).sum()) > 0 and not same(got[i], first[i]), "%s did not change with the weights" % names[i]
    # the launches that hold copies or cached descriptors did run, before and after: the variants are the ones built before training
    for (plan, private), had in zip(variants, built):
        key = eng._fused(private)
        assert key in had and plan["variants"][key] is had[key], "the inference variant was rebuilt, not reused"
        ops = eng.active_ops(plan, private=private)
        kinds = [op.kind for op in ops]
        assert "dual" in kinds                               # the folded shortcut: K-concatenated filters, summed biases
        if dtype == "bf16":
            assert "stem" in kinds and "chain" in kinds and kinds.count("bneck") == 3
            assert any(op[3].get("proj") for op in ops if op.kind == "bneck")        # res2a: the dual filters inside the fused block
            steps = sorted(op[3]["x_out_step"] for op in ops if op.kind == "bneck" and not op[3].get("proj"))
            assert key[6] == int(private) and steps == ([2, 2] if private else [1, 1])      # detect(): the quarter-C2 form
        else:
            assert not {"stem", "chain", "bneck"} & set(kinds) and kinds.count("dual") == 4


# ------------------------------------------------------------------ (d) fp8 towers and fp8 backbone
@pytest.mark.parametrize("backbone", [False, True], ids=["towers", "towers+backbone"])
def test_fp8_filters_and_plans_follow_training(pkg, backbone):
    E, Wt, T = mods(pkg)
    eng = new_engine(E, start_state(Wt), "bf16")
    x = batch(51)[0]
    eng.calibrate_fp8(x, backbone=backbone)
    first = [t.clone() for t in eng.detect(x)]             # builds the e4m3 filters and the fp8 plan
    H, W = CANVAS
    kinds = [op.kind for op in eng._plan(B, H, W)["ops"]]
    layers = eng._fp8_layers()
    assert eng._plan(B, H, W)["fp8"] and kinds.count("conv8") == len(layers) and ("convq" in kinds) == backbone
    assert set(eng._w8) == set(layers) and len(layers) == (8 + 13 + 1 if backbone else 8)
    w8_first = {n: (wq.clone(), sw) for n, (wq, sw) in eng._w8.items()}
    scales = dict(eng.fp8_scales)
    tr = new_trainer(T, eng)
    train(tr, (41, 42, 43)[:STEPS])
    assert eng.fp8_scales == scales                        # training leaves the calibration alone
    got = [t.clone() for t in eng.detect(x)]
    fresh = new_engine(E, tr.get_state(), "bf16")
    fresh.fp8_scales, fresh.fp8_backbone = dict(eng.fp8_scales), eng.fp8_backbone       # the same activation scales, not recalibrated
    want = [t.clone() for t in fresh.detect(x)]
    torch.cuda.synchronize()
    assert fresh._plan(B, H, W)["fp8"] and [op.kind for op in fresh._plan(B, H, W)["ops"]] == [op.kind for op in eng._plan(B, H, W)["ops"]]
    assert int((got[1] >= 0).sum()) > 0
    for name, g, w in zip(("boxes", "scores", "labels"), got, want):
        assert same(g, w), "fp8 %s after training differ from a reloaded engine's" % name
    assert not same(got[1], first[1])
    assert set(eng._w8) == set(fresh._w8) == set(layers)
    for name in layers:
        assert same(eng._w8[name][0], fresh._w8[name][0]), "%s: e4m3 filters are not those of the trained weights" % name
        assert eng._w8[name][1] == fresh._w8[name][1], "%s: weight scale %r, reloaded %r" % (name, eng._w8[name][1], fresh._w8[name][1])
        assert not same(eng._w8[name][0], w8_first[name][0]), "%s: e4m3 filters did not change with the weights" % name
    if backbone:
        # A weight scale is 448 / max |w| and a layer's largest bf16 element rarely moves in three steps (the towers' do not); P3's
        # does.  Its scale sits inside the fp8 plan's ops, so this is the run in which a plan kept across the steps would show.
        assert any(eng._w8[name][1] != w8_first[name][1] for name in layers), "no weight scale changed: stale plan scales would pass"


# ------------------------------------------------------------------ (e) trainable-set changes
def test_copies_follow_every_trainable_set(pkg):
    E, Wt, T = mods(pkg)
    eng = new_engine(E, start_state(Wt), "bf16")
    heads = frozenset(n for n in eng.layout if n.startswith("pyramid_"))
    assert len(heads) == 10
    tr = new_trainer(T, eng, trainable=heads)
    torch.cuda.synchronize()
    w0, wd0 = eng.wflat.clone(), {n: t.clone() for n, t in tr.wd.items()}
    # 1. heads only
    train(tr, (41, 42, 43)[:STEPS])
    assert_copies_match_fresh(E, T, tr, "heads trainable")
    for name in eng.layout:
        moved = not same(layer_slice(eng, w0, name), layer_slice(eng, eng.wflat, name))
        assert moved == (name in heads), "%s: forward weights %s" % (name, "moved though frozen" if moved else "did not move")
        if name in tr.wd:
            assert same(wd0[name], tr.wd[name]) == (name not in heads), "%s: backward filters" % name
    # 2. everything
    tr.set_trainable(None)
    w1 = eng.wflat.clone()
    train(tr, (44, 45, 46)[:STEPS])
    assert_copies_match_fresh(E, T, tr, "every layer trainable after heads only")
    assert not [n for n in LAYERS if same(layer_slice(eng, w1, n), layer_slice(eng, eng.wflat, n))]
    # 3. a few backbone layers, a stage's first block (dual-source filters) among them
    some = frozenset(["res2a_branch2c", "res2a_branch1", "res3b_branch2b", "res4a_branch2a", "res4a_branch2b", "res4a_branch2c",
                      "res4a_branch1", "res5c_branch2c"])
    tr.set_trainable(some)
    w2 = eng.wflat.clone()
    train(tr, (47, 48, 49)[:STEPS])
    assert_copies_match_fresh(E, T, tr, "a backbone subset trainable after every layer")
    for name in eng.layout:
        assert same(layer_slice(eng, w2, name), layer_slice(eng, eng.wflat, name)) == (name not in some), name
    # 4. nothing trains: nothing changes
    tr.set_trainable(frozenset())
    torch.cuda.synchronize()
    held = {a: getattr(tr, a).clone() for a in ("master", "m", "v")}
    held.update(wflat=eng.wflat.clone(), bflat=eng.bflat.clone())
    wd3 = {n: t.clone() for n, t in tr.wd.items()}
    train(tr, (50,))
    torch.cuda.synchronize()
    for a, t in held.items():
        assert same(t, getattr(eng if a in ("wflat", "bflat") else tr, a)), "%s changed in a step with no trainable layer" % a
    assert all(same(wd3[n], tr.wd[n]) for n in tr.wd)
    assert_copies_match_fresh(E, T, tr, "no layer trainable")


# ------------------------------------------------------------------ (f) the next step sees the same model
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_next_forward_backward_equals_a_reloaded_trainers(pkg, dtype):
    """Whatever copy the training forward or backward reads, listed above or not: after three steps the loss sums and the whole flat
    gradient of a new batch are those of a trainer built on the saved state.  (The optimizer state differs by design: nothing is
    compared after optimizer_step.)"""
    E, Wt, T = mods(pkg)
    tr = new_trainer(T, new_engine(E, start_state(Wt), dtype))
    train(tr, (41, 42, 43)[:STEPS])
    torch.cuda.synchronize()
    ftr = new_trainer(T, new_engine(E, tr.get_state(), dtype))
    x, reg_t, lab_t = batch(61)
    out = []
    for t in (tr, ftr):
        sums = t.forward_backward(x, reg_t, lab_t)
        torch.cuda.synchronize()
        out.append((sums.clone(), t.grad.clone()))
    (s_live, g_live), (s_new, g_new) = out
    assert float(s_live[2]) > 0 and float(g_live.abs().max()) > 0
    assert same(s_live, s_new), (s_live.tolist(), s_new.tolist())
    assert same(g_live, g_new), "gradients differ on %d elements (max %.3e)" % (int((g_live != g_new).sum()), float((g_live - g_new).abs().max()))
