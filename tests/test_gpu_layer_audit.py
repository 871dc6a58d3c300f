"""Every launch of the benched forward plans, one at a time, against float64 on the device's own inputs (tests/layer_audit.py).

The plans run op by op on one stream (Engine.active_ops / Engine._run_op): before a launch its reads are snapshotted, after it the
reads must be unchanged and every tensor it writes is compared, element by element (all rows up to 200k rows, else the sampled
seams / corners / tail / random rows), with the per-element bound of layer_audit.py.  Layer semantics come from
weights.conv_layers and the model definition restated below, never from the descriptors; the engine's packed weights are asserted
to hold exactly bf16(fold(state)).  Per op: the kernel generation, whether stream-K ran and, for launches with a workspace, the
stream-K sync-timeout word, which must be 0.  Coverage: every layer of the network audited exactly once.

Then the concurrency that bench.py runs (in_flight = 2, two_streams) must reproduce the serial bits.
Run with -s for the per-op table."""
import ctypes as C
import importlib
import time
from collections import Counter

import pytest
import torch

import layer_audit as LA

pytestmark = pytest.mark.gpu


def mods(pkg):
    return importlib.import_module(pkg.__name__ + ".engine"), importlib.import_module(pkg.__name__ + ".weights")


def images(B, canvas, seed):
    """Normalised pages as bench.py feeds them (x / 127.5 - 1 of a synthetic distance-transform page), float32 on the device."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.clamp(torch.empty(B, canvas[0], canvas[1], 3).exponential_(1 / 12.0, generator=g) *
                      torch.rand(B, canvas[0], canvas[1], 3, generator=g), 0, 255).round()
    return (raw / 127.5 - 1.0).float().cuda()


class Auditor:
    def __init__(self, pkg, eng, state, dtype, tag):
        E, Wt = mods(pkg)
        self.L = pkg._lib
        self.eng, self.state, self.dtype, self.tag = eng, state, dtype, tag
        self.layers = {l[0]: l for l in Wt.conv_layers(eng.backbone, eng.K, eng.A)}
        self.order = [l[0] for l in Wt.conv_layers(eng.backbone, eng.K, eng.A)]
        self.wcache = {}
        self.covered = Counter()
        self.rows_log = []
        self.seed = 0
        self.split = True

    # ---- weights: the fold restated, and the engine's packed copy must hold exactly those bits
    def weights(self, name):
        if name not in self.wcache:
            layer = self.layers[name]
            w, b = LA.layer_weights(self.state, layer, self.dtype)
            _, kh, kw, cin, cout, _, _ = layer
            wk, bk = self.eng.w[name][0], self.eng.w[name][1]
            if name == "conv1":
                dev = wk.view(wk.shape[0], 8, 8, 4)
                assert torch.equal(dev[:cout, :7, :7, :3].cpu().double(), w), "conv1: packed filters are not bf16(fold)"
                rest = dev.clone()
                rest[:cout, :7, :7, :3] = 0
                assert not bool(rest.any()), "conv1: packed filters hold data outside the 7x7x3 taps"
            else:
                assert torch.equal(wk[:cout].view(cout, kh, kw, cin).cpu().double(), w), "%s: packed filters are not bf16(fold)" % name
                assert not bool(wk[cout:].any()), "%s: padding rows are not zero" % name
            assert torch.equal(bk[:cout].cpu().double(), b), "%s: bias is not the f32 fold" % name
            self.wcache[name] = (w.cuda(), b.cuda())
        return self.wcache[name]

    def L_of(self, name):
        _, kh, kw, cin, *_ = self.layers[name]
        if name == "conv1":
            return LA.conv_L(8 * 32, self.dtype, self.split)      # the packed stem: 8 kernel rows of one 32-element run each
        return LA.conv_L(kh * kw * cin, self.dtype, self.split)

    def rows(self, B, H, W):
        self.seed += 1
        return LA.sample_rows(B, H, W, seed=self.seed).cuda()

    def cover(self, *names):
        for n in names:
            assert n in self.layers, n
            self.covered[n] += 1

    # ---- per op kind
    def run(self, op, img):
        eng, L = self.eng, self.L
        reads, writes = eng._op_io(op)
        assert not (set(reads) & set(writes)), "%s reads what it writes" % (op[2] if isinstance(op[2], str) else op[0])
        snap = self._snapshot(op)
        # stream-K pieces / K slices need a workspace for their partial sums: without one a tile's K loop is one chain
        self.split = op[0] in ("conv", "dual") and bool(op[1].workspace)
        eng._run_op(op, img)
        torch.cuda.synchronize()
        impl = sk = to = None
        if op[0] in ("conv", "dual"):
            impl = int(L.lib.rtn_debug_last_conv_impl(eng.h.raw))
            sk = int(L.lib.rtn_debug_last_conv_streamk(eng.h.raw))
            if op[1].workspace:
                n = C.c_uint32(123)
                eng.h.check(L.lib.rtn_debug_conv_sync_timeouts(eng.h.raw, op[1].workspace, C.byref(n)))
                to = int(n.value)
        for t, s in snap:
            assert torch.equal(t, s), "op %s changed one of its inputs" % (op[0],)
        res = getattr(self, "a_" + op[0])(op, img)
        name = op[2] if isinstance(op[2], str) else op[0]
        worst = max((r["worst"] for r in res), default=0.0)
        nrows = sum(r.get("rows", 0) for r in res)
        rec = {"name": name, "kind": op[0], "impl": impl, "sk": sk, "timeouts": to, "rows": nrows, "worst": worst,
               "bad": [(r.get("what"), r["bad"], r["where"]) for r in res if r["bad"]]}
        self.rows_log.append(rec)
        return rec

    def _snapshot(self, op):
        ts = []
        if op[0] in ("conv",):
            ts = list(op[3]["xs"]) + [t for t in op[3]["res"] if t is not None]
        elif op[0] == "dual":
            ts = list(op[4]["xs"])
        elif op[0] in ("bneck", "chain"):
            ts = list(op[3]["xs"])
        elif op[0] == "stem":
            ts = [op[5]]
        elif op[0] in ("pool", "relu"):
            ts = [op[1]]
        return [(t, t.clone()) for t in ts]

    def _conv_check(self, what, name, x, y, rows, Ho, Wo, stride, pad, relu, res=None, sigmoid=False, out_dt=None, extra_terms=(),
                    bias=None, got=None):
        w, b = self.weights(name)
        cout, kh, kw, cin = w.shape
        fn = lambda lo, hi: LA.gather(x, rows[lo:hi], Ho, Wo, kh, kw, stride, pad)
        terms = [(fn, w.reshape(cout, -1), len(rows))] + list(extra_terms)
        ref, A = LA.conv_ref(terms, bias=b if bias is None else bias, res=res, relu=relu, sigmoid=sigmoid)
        g = LA.rows_of(y, rows)[:, :cout] if got is None else got
        Lc = LA.conv_L(sum(t[1].shape[1] for t in terms), self.dtype, self.split) if extra_terms else self.L_of(name)
        r = LA.compare(g, ref, A, Lc, out_dt or self.dtype, sigmoid=sigmoid)
        r["rows"], r["what"] = len(rows), what
        return r

    def a_pack(self, op, img):
        xp, xi = op[1], op[2]
        B, H, W, Hp, Wp = xi["B"], xi["H"], xi["W"], xi["Hp"], xi["Wp"]
        pk = xp[:B * Hp * Wp * 4].view(B, Hp, Wp, 4)
        want = torch.zeros(B, Hp, Wp, 4, dtype=xp.dtype, device=xp.device)
        want[:, 3:3 + H, 3:3 + W, :3] = img.to(xp.dtype)                # ZeroPadding2D(3), one rounding of the f32 page
        ok = torch.equal(pk, want) and not bool(xp[B * Hp * Wp * 4:].any())
        return [{"worst": 0.0 if ok else float("inf"), "bad": 0 if ok else 1, "where": None, "rows": B * Hp * Wp, "what": "packed"}]

    def _image(self, op_xp, B, H, W, Hp, Wp):
        return op_xp[:B * Hp * Wp * 4].view(B, Hp, Wp, 4)[:, 3:3 + H, 3:3 + W, :3]

    def a_conv(self, op, img):
        m = op[3]
        name = op[2]
        _, kh, kw, cin, cout, has_bias, bn = self.layers[name]
        out = []
        if m.get("stem"):                                 # conv1 on the packed page: ZeroPadding2D(3) + 7x7 / 2 'valid'
            xi = self.xin
            x = self._image(m["xs"][0], xi["B"], xi["H"], xi["W"], xi["Hp"], xi["Wp"])
            y = m["ys"][0]
            rows = self.rows(*y.shape[:3])
            out.append(self._conv_check(name, name, x, y, rows, y.shape[1], y.shape[2], 2, (3, 3), True))
            self.cover(name)
            return out
        geo = self.geo(name)
        for gi, (x, y) in enumerate(zip(m["xs"], m["ys"])):
            B, Hi, Wi, _ = x.shape
            st, padk, relu, add, sig, head_out = geo
            Ho, Wo = (Hi - 1) // st + 1, (Wi - 1) // st + 1
            if padk == "same":
                pad = (LA.same_pad_before(Hi, kh, st), LA.same_pad_before(Wi, kw, st))
            else:
                pad = (padk, padk)
            if not head_out:
                assert tuple(y.shape[1:3]) == (Ho, Wo), "%s: output %s, the model says %s" % (name, tuple(y.shape[1:3]), (Ho, Wo))
            rows = self.rows(B, Ho, Wo)
            res = None
            if add == "same":
                res = LA.rows_of(m["res"][gi], rows)
            elif add == "up":
                res = LA.upsample_rows(m["res"][gi], rows, Ho, Wo)
            got = None
            if head_out:                                  # the level's rows inside the concatenated (B, N, A * per_anchor) output
                off = sum(h * w_ for (h, w_) in self.levels[:gi]) * cout
                got = y.view(B, -1)[:, off:off + Ho * Wo * cout].reshape(B * Ho * Wo, cout)[rows]
            out.append(self._conv_check("%s[%d]" % (name, gi), name, x, y, rows, Ho, Wo, st, pad, relu, res=res, sigmoid=sig,
                                        out_dt="f32" if head_out else None, got=got))
        self.cover(name)
        return out

    def geo(self, name):
        """(stride, pad, relu, added, sigmoid, head output) of a layer, from the model definition."""
        if name.startswith("res"):
            stage, block = int(name[3]), name[4:name.index("_")]
            first = block == "a"
            st = 2 if (first and stage > 2 and (name.endswith("branch2a") or name.endswith("branch1"))) else 1
            if name.endswith("branch2a"):
                return (st, 0, True, None, False, False)
            if name.endswith("branch2b"):
                return (1, 1, True, None, False, False)
            if name.endswith("branch2c"):
                return (1, 0, True, "same", False, False)
            return (st, 0, False, None, False, False)          # branch1: BN, no activation
        if name in ("C5_reduced",):
            return (1, 0, False, None, False, False)
        if name in ("C4_reduced", "C3_reduced"):
            return (1, 0, False, "up", False, False)
        if name in ("P5", "P4", "P3"):
            return (1, "same", False, None, False, False)
        if name in ("P6", "P7"):
            return (2, "same", False, None, False, False)
        if name in ("pyramid_regression", "pyramid_classification"):
            return (1, "same", False, None, name == "pyramid_classification", True)
        if name.startswith("pyramid_"):
            return (1, "same", True, None, False, False)
        raise KeyError(name)

    def a_dual(self, op, img):
        key = op[2].split("_")[0]
        b2, x = op[4]["xs"]
        y = op[4]["ys"][0]
        n2c, n1 = key + "_branch2c", key + "_branch1"
        st = self.geo(n1)[0]
        B, Ho, Wo, _ = y.shape
        rows = self.rows(B, Ho, Wo)
        w1, b1 = self.weights(n1)
        _, b2c = self.weights(n2c)
        fn1 = lambda lo, hi: LA.gather(x, rows[lo:hi], Ho, Wo, 1, 1, st, (0, 0))
        r = self._conv_check(op[2], n2c, b2, y, rows, Ho, Wo, 1, (0, 0), True, extra_terms=[(fn1, w1.reshape(w1.shape[0], -1), len(rows))],
                             bias=b2c + b1)
        self.cover(n2c, n1)
        return [r]

    def _next2a(self, last):
        nxt = self.order[self.order.index(last) + 1]
        assert nxt.endswith("_branch2a"), nxt
        return nxt

    def _h1_interval(self, n2b, a, rows, Ho, Wo):
        """branch2b's bf16 output at `rows` as an interval (it never reaches memory in the inference form)."""
        w, b = self.weights(n2b)
        fn = lambda lo, hi: LA.gather(a, rows[lo:hi], Ho, Wo, 3, 3, 1, (1, 1))
        v, A = LA.conv_ref([(fn, w.reshape(w.shape[0], -1), len(rows))], bias=b, relu=True)
        lo, hi = LA.bf16_interval(v, LA.gamma(self.L_of(n2b)) * A)
        return v.float().to(torch.bfloat16).double(), hi - lo

    def a_bneck(self, op, img):
        m = op[3]
        n2b = op[2].split("+")[0]
        blk = n2b[:-len("_branch2b")]
        n2c, n1 = blk + "_branch2c", blk + "_branch1"
        a, x = m["xs"]
        y = m["ys"][0]
        B, Ho, Wo, C4 = y.shape
        rows = self.rows(B, Ho, Wo)
        out = []
        w2c, b2c = self.weights(n2c)
        if m["h1"]:                                       # training form: h1 is stored - audit it, then build on its bits
            h1 = m["ys"][-1]
            out.append(self._conv_check(n2b, n2b, a, h1, rows, Ho, Wo, 1, (1, 1), True))
            hmid, width = LA.rows_of(h1, rows), None
        else:
            hmid, width = self._h1_interval(n2b, a, rows, Ho, Wo)
        terms = [(lambda lo, hi: hmid[lo:hi], w2c.reshape(w2c.shape[0], -1), len(rows))]
        bias, res = b2c, None
        if m.get("proj"):
            w1, b1 = self.weights(n1)
            terms.append((lambda lo, hi: LA.rows_of(x, rows[lo:hi]), w1.reshape(w1.shape[0], -1), len(rows)))
            bias = b2c + b1
        else:
            res = LA.rows_of(x, rows)
        ref, A = LA.conv_ref(terms, bias=bias, res=res, relu=True)
        extra = None if width is None else width @ w2c.reshape(w2c.shape[0], -1).abs().t()
        r = LA.compare(LA.rows_of(y, rows), ref, A, LA.conv_L(sum(t[1].shape[1] for t in terms), "bf16", self.split), "bf16",
                       extra=extra)
        r["rows"], r["what"] = len(rows), n2c
        out.append(r)
        self.cover(n2b, n2c, *([n1] if m.get("proj") else []))
        if m["tail"]:
            n2a = self._next2a(n1 if m.get("proj") else n2c)
            out.append(self._conv_check(n2a, n2a, y, m["ys"][1], rows, Ho, Wo, 1, (0, 0), True))
            self.cover(n2a)
        return out

    def a_chain(self, op, img):
        m = op[3]
        n2c = op[2].split("+")[0]
        h, x = m["xs"]
        y, a = m["ys"]
        B, Ho, Wo, _ = y.shape
        rows = self.rows(B, Ho, Wo)
        r1 = self._conv_check(n2c, n2c, h, y, rows, Ho, Wo, 1, (0, 0), True, res=LA.rows_of(x, rows))
        n2a = self._next2a(n2c)
        r2 = self._conv_check(n2a, n2a, y, a, rows, Ho, Wo, 1, (0, 0), True)
        self.cover(n2c, n2a)
        return [r1, r2]

    def a_stem(self, op, img):
        """conv1 + ReLU (rounded to bf16 in registers) + pool1 (+ res2a_branch2a): pool1 must lie in [maxpool(lo), maxpool(hi)] of
        conv1's interval; branch2a is audited on the stored pool1."""
        pool, (B, H, W), xp, (Hp, Wp) = op[1], op[2], op[5], op[6]
        x = self._image(xp, B, H, W, Hp, Wp)
        H1, W1 = (H + 1) // 2, (W + 1) // 2
        H2, W2 = pool.shape[1], pool.shape[2]
        rows = self.rows(B, H2, W2)
        w, b = self.weights("conv1")
        # conv1 rows under every tap of every pooled row
        b_ = rows // (H2 * W2)
        r_ = rows % (H2 * W2)
        oy, ox = r_ // W2, r_ % W2
        pt, pl = LA.same_pad_before(H1, 3, 2), LA.same_pad_before(W1, 3, 2)
        lo_t, hi_t = [], []
        Lst = self.L_of("conv1")
        for t in range(9):
            iy, ix = oy * 2 - pt + t // 3, ox * 2 - pl + t % 3
            ok = (iy >= 0) & (iy < H1) & (ix >= 0) & (ix < W1)
            crow = b_ * H1 * W1 + iy.clamp(0, H1 - 1) * W1 + ix.clamp(0, W1 - 1)
            fn = lambda lo, hi, crow=crow: LA.gather(x, crow[lo:hi], H1, W1, 7, 7, 2, (3, 3))
            v, A = LA.conv_ref([(fn, w.reshape(64, -1), len(rows))], bias=b, relu=True)
            lo, hi = LA.bf16_interval(v, LA.gamma(Lst) * A)
            neg = torch.full_like(lo, -float("inf"))
            lo_t.append(torch.where(ok.unsqueeze(1), lo, neg))
            hi_t.append(torch.where(ok.unsqueeze(1), hi, neg))
        lo = torch.stack(lo_t).max(0).values
        hi = torch.stack(hi_t).max(0).values
        r = LA.compare_interval(LA.rows_of(pool, rows), lo, hi)
        r["rows"], r["what"] = len(rows), "conv1+pool1"
        out = [r]
        self.cover("conv1")
        if op[7] is not None:
            a_out = op[7][0]
            out.append(self._conv_check("res2a_branch2a", "res2a_branch2a", pool, a_out, rows, H2, W2, 1, (0, 0), True))
            self.cover("res2a_branch2a")
        return out

    def a_pool(self, op, img):
        c1, y = op[1], op[2]
        B, H2, W2, _ = y.shape
        rows = self.rows(B, H2, W2)
        want = LA.maxpool_rows(c1, rows, H2, W2)
        ok = torch.equal(LA.rows_of(y, rows), want)
        return [{"worst": 0.0 if ok else float("inf"), "bad": 0 if ok else 1, "where": None, "rows": len(rows), "what": "pool1"}]

    def a_relu(self, op, img):
        ok = torch.equal(op[2], torch.relu(op[1]))
        return [{"worst": 0.0 if ok else float("inf"), "bad": 0 if ok else 1, "where": None, "rows": op[1].numel() // op[1].shape[-1],
                 "what": "P6 relu"}]


def audit_forward(pkg, eng, state, x, tag):
    """Run the plan's active ops one at a time on the current stream, auditing each.  Returns (auditor, regression, classification)."""
    E, Wt = mods(pkg)
    B, H, W, _ = x.shape
    plan = eng._plan(B, H, W)
    eng._bind_stream()
    ops = eng.active_ops(plan)
    au = Auditor(pkg, eng, state, eng.dtype, tag)
    au.xin = plan["xin"]
    au.levels = [(p.shape[1], p.shape[2]) for p in plan["pyr"]]
    t0 = time.time()
    for op in ops:
        rec = au.run(op, x)
        print("%-5s %-44s %-5s impl %-4s sk %-4s to %-4s rows %8d  worst err/bound %.3f" % (
            tag, rec["name"][:44], rec["kind"], rec["impl"], rec["sk"], rec["timeouts"], rec["rows"], rec["worst"]))
        assert not rec["bad"], "%s %s: bound exceeded %s" % (tag, rec["name"], rec["bad"])
        assert rec["timeouts"] in (None, 0), "%s %s: %d stream-K polls timed out" % (tag, rec["name"], rec["timeouts"])
    names = [l[0] for l in Wt.conv_layers(eng.backbone, eng.K, eng.A)]
    missing = [n for n in names if au.covered[n] == 0]
    twice = [n for n in names if au.covered[n] > 1]
    print("%s coverage: %d layers, %d missing, %d audited twice; %.1f s" % (tag, len(names), len(missing), len(twice), time.time() - t0))
    assert not missing and not twice, (missing, twice)
    worst = {}
    for r in au.rows_log:
        worst[r["kind"]] = max(worst.get(r["kind"], 0.0), r["worst"])
    print("%s worst err/bound per op kind: %s" % (tag, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    return au, plan["regression"].clone(), plan["classification"].clone()


@pytest.fixture(scope="module")
def r50(pkg):
    E, Wt = mods(pkg)
    state = Wt.init_state("resnet50", 1, 9, seed=0, randomize_bn=True, cls_bias=0.0, tame=True)
    eng = E.Engine("resnet50", 1, 9, dtype="bf16")
    eng.load_state(state)
    return {"E": E, "state": state, "eng": eng, "serial": {}}


@pytest.fixture(scope="module")
def t0():
    """Start of this module's tests (not of the session): the module's own time is printed against its ~200 s budget."""
    return time.time()


def test_audit_r50_bf16_800x1333_batch8(t0, pkg, r50):
    """(a) The benched plan: every op of ResNet-50 bf16 at 8 x 800 x 1333, default selections."""
    eng = r50["eng"]
    assert eng.two_streams and eng.fuse_stem and eng.fuse_shortcut and eng.fuse_bottleneck and eng.fuse_chain
    x = images(8, (800, 1333), seed=21)
    au, reg, cls = audit_forward(pkg, eng, r50["state"], x, "r50")
    assert any(r["sk"] for r in au.rows_log if r["sk"] is not None), "no op took stream-K: that part of the audit is vacuous"
    kinds = {r["kind"] for r in au.rows_log}
    assert {"pack", "stem", "conv", "dual", "bneck", "chain", "relu"} <= kinds, kinds
    r50["serial"][21] = (reg, cls)


def test_in_flight_reproduces_the_serial_bits(pkg, r50):
    """(d) What bench.py runs: lanes on side streams (two_streams) and in_flight = 2 buffer sets, four different batches - the same
    bits as the serial pass of each, and no stream-K poll of either slot's workspaces timed out."""
    eng, L = r50["eng"], pkg._lib
    seeds = [21, 22, 23, 24]
    xs = {s: images(8, (800, 1333), seed=s) for s in seeds}
    eng.two_streams = False
    for s in seeds:
        reg, cls = eng.forward(xs[s])
        torch.cuda.synchronize()
        if s in r50["serial"]:
            assert torch.equal(reg, r50["serial"][s][0]) and torch.equal(cls, r50["serial"][s][1]), "serial forward != audited op-by-op pass"
        r50["serial"][s] = (reg.clone(), cls.clone())
    eng.two_streams = True
    for s in seeds:
        reg, cls = eng.forward(xs[s])
        torch.cuda.synchronize()
        assert torch.equal(reg, r50["serial"][s][0]) and torch.equal(cls, r50["serial"][s][1]), "two_streams forward differs (batch %d)" % s
    want_det = {}
    eng.in_flight = 1
    for s in seeds:
        bx, sc, lb = eng.detect(xs[s])
        torch.cuda.synchronize()
        want_det[s] = (bx.clone(), sc.clone(), lb.clone())
    eng.in_flight = 2
    try:
        # four detects back to back, as bench.py's steady state: the third and fourth reuse a buffer set whose previous batch may
        # still run.  Each batch's outputs are copied on its set's own stream right behind it (slot_stream: the set's next batch
        # is ordered after that work), so all four can be compared after the join.
        got = {}
        for s in seeds:
            boxes, scores, labels = eng.detect(xs[s])
            si = eng.last_slot
            plan = eng._plan(8, 800, 1333, slot=si + 1)
            with torch.cuda.stream(eng.slot_stream(si)):
                got[s] = (plan["regression"].clone(), plan["classification"].clone(), boxes.clone(), scores.clone(), labels.clone())
        eng.join()
        torch.cuda.synchronize()
        for s in seeds:
            reg, cls, bx, sc, lb = got[s]
            assert torch.equal(reg, r50["serial"][s][0]) and torch.equal(cls, r50["serial"][s][1]), "in-flight batch %d differs" % s
            assert torch.equal(bx, want_det[s][0]) and torch.equal(sc, want_det[s][1]) and torch.equal(lb, want_det[s][2]), \
                "in-flight detections of batch %d differ" % s
        for s in seeds[2:]:                                # the last two batches are still in their buffer sets
            plan = eng._plan(8, 800, 1333, slot=seeds.index(s) % 2 + 1)
            assert torch.equal(plan["regression"], r50["serial"][s][0]) and torch.equal(plan["classification"], r50["serial"][s][1])
        nws = 0
        for si in range(2):
            plan = eng._plan(8, 800, 1333, slot=si + 1)
            for op in eng.active_ops(plan):
                if op[0] in ("conv", "dual") and op[1].workspace:
                    n = C.c_uint32(123)
                    eng.h.check(L.lib.rtn_debug_conv_sync_timeouts(eng.h.raw, op[1].workspace, C.byref(n)))
                    assert n.value == 0, "%s (slot %d): %d stream-K polls timed out" % (op[2], si, n.value)
                    nws += 1
        assert nws > 0
        print("in-flight: 4 batches bit-identical to the serial pass; %d workspaces of 2 slots, 0 timeouts" % nws)
    finally:
        eng.in_flight = 1
        eng.join()
        torch.cuda.synchronize()


@pytest.mark.parametrize("cfg", ["f32_r50_800x1333", "bf16_r101_1024x1024"])
def test_audit_other_configurations(t0, pkg, cfg):
    """(b) The fp32 parity path (2 x 800 x 1333) and ResNet-101 bf16 (configs[4] shape, 2 x 1024 x 1024)."""
    E, Wt = mods(pkg)
    dtype, bb, canvas = {"f32_r50_800x1333": ("f32", "resnet50", (800, 1333)),
                         "bf16_r101_1024x1024": ("bf16", "resnet101", (1024, 1024))}[cfg]
    state = Wt.init_state(bb, 1, 9, seed=0, randomize_bn=True, cls_bias=0.0, tame=True)
    eng = E.Engine(bb, 1, 9, dtype=dtype)
    eng.load_state(state)
    x = images(2, canvas, seed=31)
    audit_forward(pkg, eng, state, x, cfg.split("_")[0] + "/" + bb[6:])
    print("layer audit module so far: %.1f s" % (time.time() - t0))


def test_poolbwd_idx_modes_at_the_benched_training_shape(t0, pkg, handle):
    """pool1's training pair at 16 x 800 x 1333 (conv1 output 16 x 400 x 667 x 64): rtn_maxpool3x3s2_tfsame_fwd_idx, then
    rtn_maxpool3x3s2_tfsame_bwd_idx in mode 1 (mask from the pool's input) and mode 2 (mask from the pooled tensor - the benched
    training default, behind the fused stem), against the float64 first-maximum reference, element by element.  Small integers make
    ties and zero windows common."""
    L = pkg._lib
    B, H, W, Cc = 16, 400, 667, 64
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    g = torch.Generator(device="cuda").manual_seed(41)
    xin = (torch.randint(-3, 4, (B, H, W, Cc), generator=g, device="cuda").clamp_min(0) * 0.5).to(torch.bfloat16)
    dy = torch.randn(B, Ho, Wo, Cc, generator=g, device="cuda").to(torch.bfloat16)
    pooled = torch.empty(B, Ho, Wo, Cc, dtype=torch.bfloat16, device="cuda")
    idx = torch.empty(B * Ho * Wo * Cc, dtype=torch.uint8, device="cuda")
    handle.check(L.lib.rtn_maxpool3x3s2_tfsame_fwd_idx(handle.raw, xin.data_ptr(), pooled.data_ptr(), idx.data_ptr(), L.RTN_BF16,
                                                       B, H, W, Cc))
    torch.cuda.synchronize()
    rows = LA.sample_rows(B, Ho, Wo, seed=5).cuda()
    assert torch.equal(LA.rows_of(pooled, rows), LA.maxpool_rows(xin, rows, Ho, Wo)), "pool1 forward differs from the maximum"
    for mode, mask in ((1, xin), (2, pooled)):
        dx = torch.full((B, H, W, Cc), float("nan"), dtype=torch.bfloat16, device="cuda")
        handle.check(L.lib.rtn_maxpool3x3s2_tfsame_bwd_idx(handle.raw, dy.data_ptr(), idx.data_ptr(), mask.data_ptr(), dx.data_ptr(),
                                                           L.RTN_BF16, B, H, W, Cc, mode))
        torch.cuda.synchronize()
        want, A = LA.maxpool_bwd_ref(dy, xin, mode, pooled)
        r = LA.compare(dx.reshape(-1, Cc), want.reshape(-1, Cc), A.reshape(-1, Cc), 4, "bf16")
        del want, A
        print("poolbwd mode %d  rows %d  worst err/bound %.3f" % (mode, B * H * W, r["worst"]))
        assert r["bad"] == 0, ("mode", mode, r)
    print("layer audit module so far: %.1f s" % (time.time() - t0))
