"""Every gradient of one training step against float64 on the device's own tensors (tests/layer_audit.py), element by element.

One Trainer.forward_backward with the real lane schedule (weight gradients on side streams), targets from the NumPy oracle.  Then
  * the loss gradient: d_reg / d_cls of rtn_retina_loss_bwd_dev against R.smooth_l1_loss / R.focal_loss(grad=True) x p (1 - p) with
    the normalisers 1 / max(1, sums[2 | 3]) (the per-element bounds of test_retina_loss_fwd_bwd), and the padded bf16 / f32 copies the
    head convolutions read must be exactly their rounding, with zeros in the padded columns;
  * every trainable conv layer exactly once: Trainer.grad_views(name) against LA.wgrad_ref(x, dY) of the layer's device input and
    the device gradient of its output (the head layers summed over the five levels, conv1 unpacked from its 8 x 8 x 4 layout), under
    L_TABLE["wgrad_<dtype>"](P, 1) / L_TABLE["bgrad"](P, 1) - splits = 1 is the longest chain of any split count - and exact zeros
    in the padding rows / bias slots;
  * every activation with an entry in bp["grad_of"] exactly once: ref = m (.) sum_j c_j, m = (T > 0) where the model puts a ReLU on
    T, each c_j in float64 from the device's own upstream gradients (LA.dgrad_ref per consuming conv, the sum's gradient for an
    identity add, LA.upsample_bwd_ref for UpsampleLike + Add, LA.maxpool_bwd_ref for pool1), under
    REL |ref| + gamma(max_j L_j + n) sum_j A_j + (n - 1) REL sum_j |c_j|  (the n - 1 roundings of the running sum).
The graph (bottleneck blocks, identity adds, ReLU placement, the FPN with UpsampleLike + Add and relu(P6), the towers shared over
five levels, stem and pool1) is restated below from the model definition and weights.conv_layers; the plan is used only to find
the device tensor of a named activation and, through bp["grad_of"], its gradient.  Nothing is read from a backward descriptor.
The fused bf16 stem never stores conv1's output: the audit runs the plan's own conv1 launch once into that buffer after the step,
checks the stem's recorded pool taps against it and routes pool1's gradient by them (BackwardAudit.conv1_output).

Rows (ResNet-50, K = 1, tame weights, cls_bias -2; every page 1-3 boxes, the last one none):
    bf16 2x320x448 default | RTN_CONV_IMPL=4 RTN_WGRAD_WIN=1 | RTN_CONV_IMPL=5 RTN_WGRAD_DMA=2 ; bf16 3x146x210 ; f32 3x146x210.
Rows at other head widths and another backbone (2x146x210, ten boxes on the first page with labels in [0, K), every class below 8 and
class K - 1 with a positive anchor - asserted on the CPU before the step):
    bf16 K = 8 (72 classification channels, dY padded to 128) | bf16 K = 30 (270 channels, 384 weight rows, dY padded to 512: the weight
    gradient runs on 384 of the 512 columns) | f32 K = 20 (180, 256 rows, 256 columns) | bf16 ResNet-101, K = 1 (122 layers).
Each row asserts the classification output's weight rows, the padded width of its dY and the kernels its two gradients ran on.
Over the first five rows together the data-gradient kernels {1, 2, 4, 5} and the weight-gradient kernels {0, 2, 3, 4} must each have run.
No launch returned an error under the forced knobs in the training forward (a launch that did would be dropped from the row and
reported here).  Run with -s for the per-tensor table.

MEASURED on the MI355X (worst err / bound per check kind, seconds per row):
    row                        loss    wgrad   bgrad   act     seconds (step + audit)
    bf16_2x320x448             0.004   0.200   0.015   0.996   2.1
    bf16_2x320x448_gen4_win    0.004   0.218   0.016   0.996   1.1
    bf16_2x320x448_gen5_dma2   0.003   0.215   0.017   0.996   0.9
    bf16_3x146x210             0.003   0.173   0.011   0.996   0.9
    f32_3x146x210              0.003   0.309   0.073   0.125   0.9
    bf16_2x146x210_K8          0.003   0.230   0.018   0.996   1.0
    bf16_2x146x210_K30         0.003   0.235   0.015   0.996   1.0
    f32_2x146x210_K20          0.003   0.305   0.066   0.130   0.9
    bf16_2x146x210_r101        0.004   0.218   0.013   0.996   1.2
(act 0.99 in bf16 is the output rounding itself: half an ulp of a value just above a power of two is 2^-8 of it.)  Kernels that ran:
data gradients {1, 2, 4} | {2, 3, 4} | {2, 5} | {1, 2} | {1, 2}, weight gradients {3} | {3, 4} | {2, 3} | {3} | {0}; in the four new rows
data gradients {1, 2}, weight gradients {3} (f32: {0}), the classification output's own on generation 2 and kernel 3 (f32: 0).  In the
fused-stem rows 71-72 % of the live pool windows have a single possible winner.  The module takes 12 s.  With the plan's MASK_PRE choice forced on
(the identity gradient left unmasked) the audit fails at res2a_branch2c with 445110 elements out of bound."""
import importlib
import os
import time
from collections import Counter

import numpy as np
import pytest
import torch

import layer_audit as LA
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

ROWS = {
    "bf16_2x320x448": ("bf16", 2, (320, 448), {}),
    "bf16_2x320x448_gen4_win": ("bf16", 2, (320, 448), {"RTN_CONV_IMPL": "4", "RTN_WGRAD_WIN": "1"}),
    "bf16_2x320x448_gen5_dma2": ("bf16", 2, (320, 448), {"RTN_CONV_IMPL": "5", "RTN_WGRAD_DMA": "2"}),
    "bf16_3x146x210": ("bf16", 3, (146, 210), {}),
    "f32_3x146x210": ("f32", 3, (146, 210), {}),
    # (..., backbone, classes): 72, 270 and 180 classification channels, dY padded to 128, 512 and 256; ResNet-101
    "bf16_2x146x210_K8": ("bf16", 2, (146, 210), {}, "resnet50", 8),
    "bf16_2x146x210_K30": ("bf16", 2, (146, 210), {}, "resnet50", 30),
    "f32_2x146x210_K20": ("f32", 2, (146, 210), {}, "resnet50", 20),
    "bf16_2x146x210_r101": ("bf16", 2, (146, 210), {}, "resnet101", 1),
}
FIRST_ROWS = list(ROWS)[:5]
# keras_resnet: blocks per stage, and the stages whose blocks are named a, b1, b2, ... instead of a, b, c, ...
STAGE_BLOCKS = {"resnet50": (3, 4, 6, 3), "resnet101": (3, 4, 23, 3), "resnet152": (3, 8, 36, 3)}
NUMERICAL = {"resnet50": (), "resnet101": (1, 2), "resnet152": (1, 2)}
TOWERS = ("pyramid_regression", "pyramid_classification")


def mods(pkg):
    return [importlib.import_module(pkg.__name__ + "." + m) for m in ("engine", "weights", "trainer")]


def row_config(row):
    """(dtype, B, canvas, env, backbone, K) of a row."""
    r = ROWS[row]
    return r + ("resnet50", 1) if len(r) == 4 else r


def make_batch(B, canvas, seed, K=1):
    """Pages and NumPy-oracle targets as in test_gpu_train.py: 1-3 boxes per page, none on the last page.
    K > 1: min(K, 8) + 2 boxes on every other page with random labels in [0, K), the first min(K, 8) of them a permutation of the
    first classes and one more of class K - 1; checked here, on the CPU: every class in [0, min(K, 8)) and the last class have a
    positive anchor, the last page has none."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.clamp(torch.empty(B, canvas[0], canvas[1], 3).exponential_(1 / 12.0, generator=g) *
                      torch.rand(B, canvas[0], canvas[1], 3, generator=g), 0, 255).round().to(torch.uint8)
    x = R.preprocess_custom_tf(raw.numpy())
    anchors = R.anchors_for_shape(tuple(canvas) + (3,))
    rng = np.random.RandomState(seed)
    gts, shapes = [], []
    for b in range(B):
        n = 0 if b == B - 1 else (rng.randint(1, 4) if K == 1 else min(K, 8) + 2)
        w, h = (rng.uniform(30, 120, n), rng.uniform(25, 90, n)) if K == 1 else (rng.uniform(24, 70, n), rng.uniform(20, 60, n))
        x1, y1 = rng.uniform(0, canvas[1] - w), rng.uniform(0, canvas[0] - h)
        gts.append(np.stack([x1, y1, x1 + w, y1 + h], axis=1).reshape(-1, 4))
        shapes.append((canvas[0], int(rng.randint(150, canvas[1] + 1))))
    if K == 1:
        classes = [np.zeros(len(g_)) for g_ in gts]
    else:
        classes = []
        for g_ in gts:
            c = rng.randint(0, K, len(g_))
            if len(g_):
                c[:min(K, 8)] = rng.permutation(min(K, 8))
                c[min(K, 8)] = K - 1
            classes.append(c.astype(np.float64))
    reg, lab = R.anchor_targets(anchors, shapes, gts, classes, K)
    assert lab.shape[-1] == K + 1
    assert (lab[..., K] == 1).sum() > 10 and (lab[-1, :, K] == 1).sum() == 0
    per_class = ((lab[..., :K] == 1) & (lab[..., K:] == 1)).sum(axis=(0, 1))
    assert np.all(per_class[:min(K, 8)] > 0) and per_class[K - 1] > 0, per_class
    return x, reg, lab


# ---------------------------------------------------------------------------------------------- the model definition, restated
def geo(name):
    """(stride, padding, ReLU on the layer's output tensor) from model/defineModel.py and keras_resnet's bottleneck: padding is an
    int ('valid' after ZeroPadding2D(p)) or "same".  branch2c's tensor is the block output: ReLU after the Add."""
    if name == "conv1":
        return 2, 3, True
    if name.startswith("res"):
        stage, first = int(name[3]), name[4] == "a"
        if name.endswith("branch2b"):
            return 1, 1, True
        st = 2 if (first and stage > 2 and not name.endswith("branch2c")) else 1
        return st, 0, not name.endswith("branch1")
    if name in ("C5_reduced", "C4_reduced", "C3_reduced"):
        return 1, 0, False
    if name in ("P5", "P4", "P3"):
        return 1, "same", False
    if name in ("P6", "P7"):
        return 2, "same", False
    if name in TOWERS:
        return 1, "same", False                 # the outputs: the loss differentiates to the logits / regression values
    if name.startswith("pyramid_"):
        return 1, "same", True
    raise KeyError(name)


def graph(backbone="resnet50"):
    """inputs: layer -> the activation key of every group's input; cons: activation key -> its consumers.  Keys: (layer, group) for a
    conv output, "pool1", "image".  Consumers: ("conv", layer, group, premask) - premask: the conv reads relu(T), not T;
    ("add", key): T is added into `key` as is; ("up", key): UpsampleLike(T) is added into `key`; ("pool", key)."""
    inputs, cons = {}, {}

    def conv(name, src, premask=False):
        inputs[name] = list(src)
        for gi, s in enumerate(src):
            cons.setdefault(s, []).append(("conv", name, gi, premask))
        return [(name, gi) for gi in range(len(src))]

    c1, = conv("conv1", ["image"])
    cons.setdefault(c1, []).append(("pool", "pool1"))
    x = "pool1"
    feats = []
    for stage, nblocks in enumerate(STAGE_BLOCKS[backbone]):
        for block in range(nblocks):
            blk = "res%d%s" % (stage + 2, "b%d" % block if (block and stage in NUMERICAL[backbone]) else "abcdef"[block])
            a, = conv(blk + "_branch2a", [x])
            b2, = conv(blk + "_branch2b", [a])
            y, = conv(blk + "_branch2c", [b2])
            sc = conv(blk + "_branch1", [x])[0] if block == 0 else x
            cons.setdefault(sc, []).append(("add", y))
            x = y
        feats.append(x)
    C3, C4, C5 = feats[1:]
    p5r, = conv("C5_reduced", [C5])
    P5, = conv("P5", [p5r])
    p4m, = conv("C4_reduced", [C4])
    cons.setdefault(p5r, []).append(("up", p4m))
    P4, = conv("P4", [p4m])
    p3m, = conv("C3_reduced", [C3])
    cons.setdefault(p4m, []).append(("up", p3m))
    P3, = conv("P3", [p3m])
    P6, = conv("P6", [C5])
    P7, = conv("P7", [P6], premask=True)                    # C6_relu sits between P6 and P7 only: the heads read P6 itself
    for prefix in TOWERS:
        cur = [P3, P4, P5, P6, P7]
        for i in range(4):
            cur = conv("%s_%d" % (prefix, i), cur)
        conv(prefix, cur)
    return inputs, cons


class BackwardAudit:
    def __init__(self, pkg, tr, state, bp, tag):
        E, Wt, _ = mods(pkg)
        eng = tr.eng
        self.tr, self.eng, self.bp, self.plan, self.tag, self.dtype = tr, eng, bp, bp["plan"], tag, eng.dtype
        self.state = state
        self.layers = {l[0]: l for l in Wt.conv_layers(eng.backbone, eng.K, eng.A)}
        self.inputs, self.cons = graph(eng.backbone)
        assert set(self.inputs) == set(self.layers), set(self.inputs) ^ set(self.layers)
        plan = self.plan
        self.convs = {op[2]: op[3] for op in plan["ops"] if op[0] == "conv"}
        pool = [op for op in plan["ops"] if op[0] == "pool"]
        assert len(pool) == 1 and pool[0][1] is self.convs["conv1"]["ys"][0]
        self.pooled = pool[0][2]
        xi = plan["xin"]
        self.B = xi["B"]
        xp = self.convs["conv1"]["xs"][0]
        self.image = xp[:xi["B"] * xi["Hp"] * xi["Wp"] * 4].view(xi["B"], xi["Hp"], xi["Wp"], 4)[:, 3:3 + xi["H"], 3:3 + xi["W"], :3]
        self.levels = [(p.shape[1], p.shape[2]) for p in plan["pyr"]]
        self.grad_of = bp["grad_of"]
        self.seen = Counter()                   # id(forward tensor) -> times its gradient was audited
        self.covered = Counter()                # layer -> times its weight gradient was audited
        self.log = []
        self.wcache = {}

    # ---- locating device tensors
    def fwd(self, key):
        """The device tensor of a named activation."""
        if key == "image":
            return self.image
        if key == "pool1":
            return self.pooled
        return self.convs[key[0]]["ys"][key[1]]

    def grad(self, key):
        """The device gradient of a named activation, [B, H, W, channels of the layer]."""
        t = self.fwd(key)
        g = self.grad_of[id(t)]
        if isinstance(key, tuple) and key[0] in TOWERS:          # the level's cells inside [B, cells of all levels, padded channels]
            cout = self.layers[key[0]][4]
            off = sum(h * w for h, w in self.levels[:key[1]])
            Hl, Wl = self.levels[key[1]]
            return g[:, off:off + Hl * Wl, :cout].reshape(self.B, Hl, Wl, cout)
        assert g.shape == t.shape and g.dtype == t.dtype, (key, g.shape, t.shape)
        return g

    def weights(self, name):
        if name not in self.wcache:
            self.wcache[name] = LA.layer_weights(self.state, self.layers[name], self.dtype)[0].cuda()
        return self.wcache[name]

    def geometry(self, name, Hi, Wi):
        _, kh, kw = self.layers[name][:3]
        st, padk, _ = geo(name)
        pad = (LA.same_pad_before(Hi, kh, st), LA.same_pad_before(Wi, kw, st)) if padk == "same" else (padk, padk)
        return st, pad, (Hi - 1) // st + 1, (Wi - 1) // st + 1

    def record(self, kind, what, r):
        self.log.append((kind, what, r))
        print("%-24s %-6s %-40s n %9d  worst err/bound %.3f" % (self.tag, kind, what[:40], r["n"], r["worst"]))
        assert r["n"] > 0, "%s %s: a check on zero elements" % (kind, what)
        assert r["bad"] == 0, "%s %s %s: bound exceeded at %d elements, worst err/bound %.3f at %s" % (
            self.tag, kind, what, r["bad"], r["worst"], r["where"])

    # ---- the loss gradient (rtn_retina_loss_bwd_dev) and its padded copies
    def loss(self, reg_t, lab_t):
        plan, bp, eng = self.plan, self.bp, self.eng
        p = plan["classification"].cpu().numpy()
        pred = plan["regression"].cpu().numpy()
        s = self.tr.norm_sums.cpu().numpy()
        _, npos, gcls = R.focal_loss(lab_t, p, grad=True)
        _, nposr, greg = R.smooth_l1_loss(reg_t, pred, grad=True)
        assert s[2] == npos and s[3] == nposr and npos > 0, (s, npos, nposr)
        p64 = p.astype(np.float64)
        want = gcls / max(1.0, s[2]) * (p64 * (1 - p64))
        got = bp["d_cls"].cpu().numpy().astype(np.float64)
        bound = 1e-4 * np.maximum(np.abs(want), 1e-3)
        ratio = np.abs(got - want) / bound
        self.record("loss", "d_cls", {"worst": float(ratio.max()), "bad": int((ratio > 1).sum()), "n": got.size,
                                      "where": np.unravel_index(int(ratio.argmax()), ratio.shape)})
        wantr = greg / max(1.0, s[3])
        gotr = bp["d_reg"].cpu().numpy().astype(np.float64)
        ratio = np.abs(gotr - wantr) / (1e-7 + 1e-5 * np.abs(wantr))
        self.record("loss", "d_reg", {"worst": float(ratio.max()), "bad": int((ratio > 1).sum()), "n": gotr.size,
                                      "where": np.unravel_index(int(ratio.argmax()), ratio.shape)})
        assert np.abs(got).max() > 0 and np.abs(gotr).max() > 0
        cells = sum(h * w for h, w in self.levels)
        for out, d32, per in ((plan["regression"], bp["d_reg"], 4), (plan["classification"], bp["d_cls"], eng.K)):
            dyp = self.grad_of[id(out)]
            n = eng.A * per
            assert dyp.shape[:2] == (self.B, cells) and dyp.dtype == eng.tdt
            assert torch.equal(dyp[..., :n], d32.view(self.B, cells, n).to(eng.tdt)), "padded loss gradient is not the rounding of d"
            assert dyp.shape[2] > n and not bool(dyp[..., n:].any()), "padded columns of the loss gradient are not zero"
            self.seen[id(out)] += 1

    # ---- weight and bias gradients
    def wgrad(self, name):
        _, kh, kw, cin, cout, has_bias, _ = self.layers[name]
        ref = A = bref = bA = 0
        P = 0
        for gi, src in enumerate(self.inputs[name]):
            x = self.fwd(src)
            if name == "P7":
                x = torch.relu(x)
            st, pad, Ho, Wo = self.geometry(name, x.shape[1], x.shape[2])
            dy = self.grad((name, gi))
            assert dy.shape == (self.B, Ho, Wo, cout), (name, gi, dy.shape, (Ho, Wo))
            r = LA.wgrad_ref(x, dy, kh, kw, st, pad)
            ref, A, bref, bA = ref + r[0], A + r[1], bref + r[2], bA + r[3]
            P += self.B * Ho * Wo
        dW, db = self.tr.grad_views(name)
        if name == "conv1":                                     # packed 8 x 8 x 4 taps: the 7 x 7 x 3 kernel inside, channel 3 is padding
            pk = dW.view(dW.shape[0], 8, 8, 4)
            got = pk[:cout, :7, :7, :3].reshape(cout, -1)
            assert not bool(pk[..., 3].any()), "conv1: the padding channel of dW is not zero"
        else:
            got = dW[:cout]
        self.record("wgrad", name, LA.compare(got, ref, A, LA.L_TABLE["wgrad_" + self.dtype](P, 1), "f32"))
        assert not bool(dW[cout:].any()), "%s: padding rows of dW are not zero" % name
        if has_bias:
            self.record("bgrad", name, LA.compare(db[:cout], bref, bA, LA.L_TABLE["bgrad"](P, 1), "f32"))
            assert not bool(db[cout:].any()), "%s: padding rows of db are not zero" % name
        else:
            assert not bool(db.any()), "%s has no bias: its slots of the gradient must stay zero" % name
        self.covered[name] += 1

    # ---- activation gradients
    def conv1_output(self):
        """conv1's ReLU output and how pool1's gradient is routed through it.  Unfused stem (f32): the tensor is on the device, the
        reference applies TensorFlow's first-maximum rule to it (mode 1).  The fused bf16 stem never stores it and rounds its own
        f32 sums: the plan's conv1 launch, run once into the unused buffer, gives values within rounding of the stem's (each is
        the bf16 rounding of an f32 sum within gamma A of the float64 one: two ulps, 2^-6 relative, + 1e-4 for values near zero,
        covers that).  There the winning taps the stem recorded are checked against those values - wherever pooled > 0 the tap must
        hold the window's maximum within that slack, and the pooled value must be the tap's value; where a single tap qualifies this
        is the first-maximum rule itself - and the reference routes by them, masked by pooled > 0 (mode 2)."""
        c1 = self.fwd(("conv1", 0))
        if not self.tr.fwd_key[0]:
            self.pool_route = None
            return
        op = [op for op in self.plan["ops"] if op[0] == "conv" and op[2] == "conv1"][0]
        self.eng._bind_stream()
        self.eng._run_op(op, None)
        torch.cuda.synchronize()
        pool_op = [op for op in self.plan["ops"] if op[0] == "pool"][0]
        idx = pool_op[4].view(self.pooled.shape)
        taps = torch.stack(LA.pool_window_taps(c1))                     # [9, B, Ho, Wo, C]
        top = taps.max(0).values
        slack = 2.0 ** -6 * top.abs() + 1e-4
        live = self.pooled > 0
        assert bool((idx[live] < 9).all())
        at = taps.gather(0, idx.clamp(max=8).long().unsqueeze(0))[0]
        assert bool((at[live] >= (top - slack)[live]).all()), "a recorded pool tap does not hold its window's maximum"
        assert bool(((at - self.pooled.double()).abs()[live] <= slack[live]).all()), "pool1 is not the value at its recorded tap"
        single = ((taps >= (top - slack).unsqueeze(0)).sum(0) == 1) & live
        frac = float(single.sum()) / max(1, int(live.sum()))
        print("%-24s stem   %d of %d live pool windows have one possible winner (%.1f %%): first-maximum rule checked there" % (
            self.tag, int(single.sum()), int(live.sum()), 100 * frac))
        assert frac > 0.5
        self.pool_route = idx

    def activation(self, key):
        t = self.fwd(key)
        g = self.grad(key)
        B, Ht, Wt, Ct = t.shape
        relu = geo(key[0])[2] if isinstance(key, tuple) else False
        ref = A = S = None
        Lmax, n = 0, 0
        for con in self.cons[key]:
            kind = con[0]
            if kind == "conv":
                _, lname, gi, premask = con
                _, kh, kw, cin, cout, _, _ = self.layers[lname]
                st, pad, Ho, Wo = self.geometry(lname, Ht, Wt)
                dy = self.grad((lname, gi))
                assert dy.shape == (B, Ho, Wo, cout) and cin == Ct
                c, a = LA.dgrad_ref(dy, self.weights(lname), Ht, Wt, st, pad)
                if premask:
                    keep = t > 0
                    c, a = torch.where(keep, c, torch.zeros_like(c)), torch.where(keep, a, torch.zeros_like(a))
                Lj = LA.conv_L(kh * kw * cout, self.dtype)
            elif kind == "add":
                c = self.grad(con[1]).double()
                a, Lj = c.abs(), 0
            elif kind == "up":
                d = self.grad(con[1])
                c, a = LA.upsample_bwd_ref(d, Ht, Wt)
                Lj = -(-d.shape[1] // Ht) * -(-d.shape[2] // Wt)          # destination pixels of one source pixel
            elif kind == "pool":
                if self.pool_route is None:
                    c, a = LA.maxpool_bwd_ref(self.grad(con[1]), t, 1)
                else:                                                     # the fused stem: see conv1_output()
                    c, a = LA.maxpool_bwd_ref(self.grad(con[1]), t, 2, self.pooled, arg=self.pool_route)
                    relu = False
                Lj = 4                                                    # at most four windows meet in one pixel
            else:
                raise KeyError(kind)
            assert c.shape == t.shape, (key, con, c.shape)
            ref, A, S = (c, a, c.abs()) if ref is None else (ref + c, A + a, S + c.abs())
            Lmax, n = max(Lmax, Lj), n + 1
        if relu:
            keep = t > 0
            zero = torch.zeros_like(ref)
            ref, A, S = torch.where(keep, ref, zero), torch.where(keep, A, zero), torch.where(keep, S, zero)
        r = LA.compare(g.reshape(-1, Ct), ref.reshape(-1, Ct), A.reshape(-1, Ct), Lmax + n, self.dtype,
                       extra=((n - 1) * LA.REL[self.dtype] * S).reshape(-1, Ct))
        what = (key if isinstance(key, str) else "%s[%d]" % key) + " <- " + "+".join(c_[0] if c_[0] != "conv" else c_[1][:14] for c_ in self.cons[key])
        self.record("act", what, r)
        self.seen[id(t)] += 1


def run_row(pkg, row):
    dtype, B, canvas, env, backbone, K = row_config(row)
    E, Wt, T = mods(pkg)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    t0 = time.time()
    try:
        # with its CPU checks, before anything runs on the device.  K > 1, seed 13: the first seed from 11 on at which every one of the
        # ten overlapping boxes of the 146 x 210 page keeps a positive anchor of its own
        x, reg_t, lab_t = make_batch(B, canvas, seed=11 if K == 1 else 13, K=K)
        state = Wt.init_state(backbone, K, 9, seed=0, randomize_bn=True, cls_bias=-2.0, tame=True)
        eng = E.Engine(backbone, K, 9, dtype=dtype)
        eng.load_state(state)
        tr = T.Trainer(eng, lr=1e-4, clipnorm=0.001)
        assert tr.wgrad_lane, "the audit is of the real lane schedule"
        tr.record_impls = True
        tr.forward_backward(torch.as_tensor(x).cuda(), torch.as_tensor(reg_t).cuda(), torch.as_tensor(lab_t).cuda())
        torch.cuda.synchronize()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    bp = tr.bplans[(B,) + tuple(canvas)]
    au = BackwardAudit(pkg, tr, state, bp, row)
    au.loss(reg_t, lab_t)
    for name in au.layers:
        au.wgrad(name)
    au.conv1_output()
    keys = [k for k in au.cons if k != "image"]
    for key in keys:
        au.activation(key)
    # coverage: every layer once, every gradient of the plan once
    names = list(au.layers)
    assert all(au.covered[n] == 1 for n in names) and len(au.covered) == len(names), au.covered
    ids = set(au.grad_of)
    assert set(au.seen) == ids and all(v == 1 for v in au.seen.values()), (len(ids), len(au.seen), [v for v in au.seen.values() if v != 1])
    worst = {}
    for kind, _, r in au.log:
        worst[kind] = max(worst.get(kind, 0.0), r["worst"])
    impls = {k: sorted(set(v for (kk, _), v in tr.impls.items() if kk == k)) for k in ("dgrad", "wgrad")}
    dt = time.time() - t0
    print("%s: %d layers, %d gradients audited; worst err/bound %s; dgrad kernels %s, wgrad kernels %s; %.1f s" % (
        row, len(names), len(ids), ", ".join("%s %.3f" % kv for kv in sorted(worst.items())), impls["dgrad"], impls["wgrad"], dt))
    cls = TOWERS[1]
    head = {"cout": eng.layout[cls]["cout"], "rows": eng.layout[cls]["rows"], "crun": tr._dy_channels(cls), "dy_shape": tuple(bp["dyp_cls"].shape),
            "dgrad": tr.impls.get(("dgrad", cls)), "wgrad": tr.impls.get(("wgrad", cls))}
    print("%s: %s %s" % (row, cls, head))
    return {"impls": impls, "worst": worst, "seconds": dt, "head": head,
            "per_layer": {k: Counter(v for (kk, _), v in tr.impls.items() if kk == k) for k in ("dgrad", "wgrad")}}


@pytest.fixture(scope="module")
def rows_done():
    return {}


def row_result(pkg, rows_done, row):
    if row not in rows_done:
        rows_done[row] = run_row(pkg, row)
    return rows_done[row]


@pytest.mark.parametrize("row", list(ROWS))
def test_backward_audit(pkg, handle, rows_done, row):
    res = row_result(pkg, rows_done, row)
    if "RTN_CONV_IMPL" in ROWS[row][3]:
        want = int(ROWS[row][3]["RTN_CONV_IMPL"])
        assert want in res["impls"]["dgrad"], "generation %d ran no data gradient: %s" % (want, res["per_layer"]["dgrad"])
    dtype, K, head = row_config(row)[0], row_config(row)[5], res["head"]
    cout = 9 * K                                            # the classification output: weight rows, the padded width of its dY, its kernels
    assert head["cout"] == cout and head["rows"] == -(-cout // 128) * 128
    assert head["crun"] == max(64, 1 << (cout - 1).bit_length()) and head["dy_shape"][2] == head["crun"]
    # its data gradient is a grouped 3x3 launch with N = 256: the per-tap kernel, or generation 4 where the grid fills the chip (or is forced);
    # its weight gradient: the register-staged kernel in f32, an LDS-DMA or the window kernel in bf16
    assert head["dgrad"] in (2, 4) and head["wgrad"] in ((0,) if dtype == "f32" else (2, 3, 4)), head


def test_every_backward_kernel_family_ran(pkg, handle, rows_done):
    """Over the five rows together: data-gradient generations 1, 2, 4, 5 and weight-gradient kernels 0 (register-staged), 2 (256 x 256
    LDS-DMA), 3 (128 x 128 LDS-DMA) and 4 (window) each on at least one layer."""
    t0 = time.time()
    d, w = set(), set()
    for row in FIRST_ROWS:
        res = row_result(pkg, rows_done, row)
        d |= set(res["impls"]["dgrad"])
        w |= set(res["impls"]["wgrad"])
    assert {1, 2, 4, 5} <= d, d
    assert {0, 2, 3, 4} <= w, w
    print("backward audit: %.1f s over the five rows (%.1f s spent in this test)" % (
        sum(rows_done[r]["seconds"] for r in FIRST_ROWS), time.time() - t0))
