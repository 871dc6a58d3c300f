"""Training step of the RetinaNet path on librtn.so: forward -> focal + smooth-L1 -> backward -> clipnorm Adam.

Mirrors what the reference gets from Keras (RetinaNet.py:125-131, 280-291):
  compile(loss={'regression': smooth_l1(), 'classification': focal()}, optimizer=Adam(lr=1e-4, clipnorm=0.001))
  -> train_on_batch(inputs, [regression_batch (B,N,5), labels_batch (B,N,K+1)])
  * total loss = smooth_l1 + focal with unit weights, each normalised by max(1, #positive anchors of the MERGED batch)
    (model/losses.py:39-44,87-90; under data parallelism the counts are all-reduced first);
  * every conv kernel and every FPN/head bias trains; BatchNorm is frozen (freeze_bn=True): its scale is folded into the
    forward weights, so the gradient w.r.t. the Keras kernel is fold[n] * dL/dW_folded and Adam runs on the unfolded
    master copy;
  * clipnorm: global-norm clipping by default (standalone Keras 2.x semantics, what the reference's `import keras` resolves to);
    `global_clip=False` clips every gradient tensor by its own norm (tf.keras / Keras >= 2.4 semantics);
  * the optimizer runs over element ranges of the flat parameter vector, one per trainable weight tensor and bias vector
    (rtn_sumsq_ranges + rtn_adam_clipnorm_step_ranges[_pertensor]): the same kernels whether every layer trains or a few.

The backward graph is derived from the forward op list of engine.Engine._plan (bplan.py): every conv gets a wgrad (+ bias grad) and a
dgrad per input; ReLU, residual adds, UpsampleLike+Add, C6_relu, max-pool and the stride-2 convs are handled by epilogue
flags of the dgrad launch or by the small kernels of rtn_backward.hip.  All arithmetic is in the HIP library; PyTorch
provides memory, the stream and (optionally) torch.distributed for the gradient all-reduce.

Frozen layers (Keras `trainable = False`, Trainer(trainable=...) / set_trainable): a tensor needs a gradient iff its producer is a
trainable layer or one of its producer's inputs needs one.  The backward plan keeps a weight gradient for the trainable layers only
and a data gradient (with its zero-insert / upsample / pool backward / head pad-cast) only into tensors that need one; the optimizer's
range tables hold the trainable layers only, the all-reduce runs over their segments, and the training forward runs the
stem and the 64-channel blocks in their inference form when the backward never reads their extra outputs (Engine.train_keep).
"""
import itertools

import numpy as np
import os
import weakref

import torch

from . import _lib as L
from . import bplan as BP
from . import ops as O
from . import weights as Wt
from . import parallel as Par
from .engine import Engine, run_lanes, schedule_lanes


def _ceil128(v):
    return -(-v // 128) * 128


def merge_adjacent(ranges):
    """[(begin, end)] with every range that starts where the previous one ends joined to it.  _lib.ranges_table puts such a range
    right behind its neighbour (no alignment gap), so the joined table places every element where the separate rows did: the same
    quads per thread, the same sums, fewer rows to search."""
    out = []
    for a, b in ranges:
        if out and out[-1][1] == a:
            out[-1] = (out[-1][0], b)
        else:
            out.append((a, b))
    return out


def grad_segments(layout, NW, NB, trainable=None):
    """GradBucketer segments of the flat gradient [weights (NW) | bias slots (NB)] and the names the trainer reports for the bias
    slots.  trainable None: every weight tensor, then all bias slots as one "__biases__" segment.  Otherwise the trainable layers
    only (frozen gradients are never all-reduced): their weight tensors, then the bias slots of the trainable layers that own a
    Keras bias, one "__biases__" segment per contiguous run ("__biases__:k" when frozen layers split them)."""
    live = [(name, lo) for name, lo in layout.items() if trainable is None or name in trainable]
    segs = [(name, lo["woff"], lo["woff"] + lo["rows"] * lo["K"]) for name, lo in live]
    if trainable is None:
        return segs + [("__biases__", NW, NW + NB)], ["__biases__"]
    runs = []
    for name, lo in live:
        if lo["has_bias"]:
            a, b = NW + lo["boff"], NW + lo["boff"] + lo["rows"]
            if runs and runs[-1][1] == a:
                runs[-1][1] = b
            else:
                runs.append([a, b])
    names = ["__biases__"] if len(runs) == 1 else ["__biases__:%d" % i for i in range(len(runs))]
    return segs + [(n, a, b) for n, (a, b) in zip(names, runs)], names


class Trainer:
    WG_LANES = 3          # side streams a weight gradient may go to
    def __init__(self, engine, lr=1e-4, clipnorm=0.001, beta1=0.9, beta2=0.999, eps=1e-7, alpha=0.25, gamma=2.0, sigma=3.0,
                 process_group=None, global_clip=True, trainable=None):
        """trainable: None (every layer trains: the full backward) or the names of the conv layers that train (the rest are frozen:
        no weight gradient, no update, and no data gradient below the lowest trainable layer)."""
        self.eng = engine
        self.trainable = self._check_names(trainable)
        self.global_clip = bool(global_clip)
        self.lr, self.clipnorm, self.b1, self.b2, self.eps = lr, clipnorm, beta1, beta2, eps
        self.alpha, self.gamma, self.sigma = alpha, gamma, sigma
        self.pg = process_group
        self.wgrad_lane = os.environ.get("RTN_WGRAD_LANE", "1") != "0"   # weight gradients on side HIP streams
        self.wgrad_lanes = max(1, min(self.WG_LANES, int(os.environ.get("RTN_WGRAD_LANES", "3"))))
        self._wg_stream = None
        self.record_impls = False      # tests: {(kind, layer): kernel code} of the last backward (rtn_debug_last_*_impl)
        self.impls = {}
        self.fwd_key = None            # Engine._fused() of the last training forward (forward_backward)
        # a backward plan holds gradient buffers, descriptors into the forward plan's activations and every weight-gradient workspace
        # (row-info table + split slabs: GBs per canvas): it lives exactly as long as the engine's plan of the same canvas
        engine.on_plan_evict.append(weakref.WeakMethod(self._drop_bplan))
        self._bind_engine_state()

    def _check_names(self, names):
        if names is None:
            return None
        names = frozenset(names)
        unknown = names - set(self.eng.layout)
        if unknown:
            raise ValueError("not a conv layer of this engine: %s" % sorted(unknown))
        return names

    def set_trainable(self, names):
        """Change the trainable set (None = every layer).  The backward plans and their lane schedules, the dgrad repack table, the
        optimizer's range tables and the gradient bucketer all follow it; the weights and the optimizer state stay."""
        names = self._check_names(names)
        if names == self.trainable:
            return
        self.trainable = names
        self.bplans = {}
        self._pack_table = None
        self._ranges = None
        self._build_bucketer()

    def _is_trainable(self, name):
        return self.trainable is None or name in self.trainable

    def _drop_bplan(self, plan_key):
        if len(plan_key) == 4:                              # (B, H, W, fp8): the one-batch buffer set the backward plan points into
            self.bplans.pop(tuple(plan_key[:3]), None)

    def _bind_engine_state(self):
        """Everything derived from the engine's loaded state: the f32 master copy, fold / gradient scales, Adam moments, dgrad
        weights, the backward plans (which hold descriptors into the forward plan's activation buffers) and the gradient
        bucketer.  Engine.load_state() reallocates the flat weights and drops its plans, so a Trainer that lived through it
        starts over from the newly loaded weights with fresh optimizer state - exactly what a new Trainer would hold."""
        self._epoch = self.eng.load_epoch
        self.step_count = 0
        self.bplans = {}
        self._ranges = None
        self._init_params()
        self._build_bucketer()

    def _build_bucketer(self):
        self.bucketer = None
        segs, self.bias_names = grad_segments(self.eng.layout, self.NW, self.NB, self.trainable)
        if self.pg is not None and segs:
            self.bucketer = Par.GradBucketer(self.grad, segs, group=self.pg)

    def _check_engine_state(self):
        if self._epoch != self.eng.load_epoch:
            self._bind_engine_state()

    # ------------------------------------------------------------------ parameters
    def _init_params(self):
        eng, dev, st = self.eng, self.eng.device, self.eng.state
        NW, NB = eng.wflat.numel(), eng.bflat.numel()
        self.NW, self.NB = NW, NB
        master = torch.zeros(NW + NB, dtype=torch.float32)
        gscale = torch.zeros(NW + NB, dtype=torch.float32)
        fold = torch.ones(NW + NB, dtype=torch.float32)
        for name, lo in eng.layout.items():
            rows, K, cout = lo["rows"], lo["K"], lo["cout"]
            pack = Wt.pack_stem if name == "conv1" else Wt.pack_conv
            wu, _ = pack(st[name + "/kernel"], None, None, torch.float32, "cpu")          # unfolded kernel, same layout
            master[lo["woff"]:lo["woff"] + rows * K] = wu.reshape(-1)
            scale = torch.ones(rows)
            if lo["bn"] is not None:
                g_, v_ = [torch.as_tensor(np.asarray(st[lo["bn"] + s]), dtype=torch.float32) for s in ("/gamma", "/moving_variance")]
                scale[:cout] = g_ / torch.sqrt(v_ + Wt.BN_EPS)
            f = scale.view(rows, 1).expand(rows, K).clone()
            gs = f.clone()
            gs[cout:] = 0.0
            if name == "conv1":                      # structural zeros of the packed stem never train
                live = torch.zeros(rows, 8, 8, 4)
                live[:cout, :7, :7, :3] = 1.0
                gs = gs * live.reshape(rows, K)
            fold[lo["woff"]:lo["woff"] + rows * K] = f.reshape(-1)
            gscale[lo["woff"]:lo["woff"] + rows * K] = gs.reshape(-1)
            # bias slot: trainable only for layers that own a Keras bias
            bo = NW + lo["boff"]
            master[bo:bo + rows] = eng.bflat[lo["boff"]:lo["boff"] + rows].cpu()
            if lo["has_bias"]:
                gscale[bo:bo + cout] = 1.0
        self.master = master.to(dev)
        self.gscale = gscale.to(dev)
        self.fold = fold.to(dev)
        self.m = torch.zeros(NW + NB, dtype=torch.float32, device=dev)
        self.v = torch.zeros(NW + NB, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(NW + NB, dtype=torch.float32, device=dev)
        self.sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        self.ss_ws = torch.empty(L.lib.rtn_sumsq_workspace_bytes(), dtype=torch.uint8, device=dev)
        self.loss_sums = torch.zeros(4, dtype=torch.float64, device=dev)
        # dgrad weights (re-packed from the forward weights after every optimizer step)
        self.wd = {}
        for name, lo in eng.layout.items():
            if name == "conv1":
                continue
            crun = self._dy_channels(name)
            self.wd[name] = torch.empty(_ceil128(lo["cin"]), lo["kh"] * lo["kw"] * crun, dtype=eng.tdt, device=dev)
        self._pack_table = None
        self._repack_dgrad(every=True)
        if self.trainable is not None:               # the steps repack the trainable layers only
            self._pack_table = None

    def _dy_channels(self, name):
        """Channels of the dY tensor a layer's backward reads: Cout, or the padded width for the skinny head outputs."""
        cout = self.eng.layout[name]["cout"]
        if name in Engine.TOWERS:
            cp = 64
            while cp < cout:
                cp *= 2
            return cp
        return cout

    def _repack_dgrad(self, every=False):
        """The dgrad weights of every layer whose forward weights an optimizer step rewrites (every=True: of all layers) from the
        forward weights, one launch: rtn_pack_dgrad_weights_multi."""
        eng = self.eng
        eng._bind_stream()
        if self._pack_table is None or self._pack_table[3] != eng.wflat.data_ptr():      # (re)built when the weights were reallocated
            rows, total = [], 0
            for name, wd in self.wd.items():
                if not (every or self._is_trainable(name)):
                    continue
                lo = eng.layout[name]
                rows.append([eng.w[name][0].data_ptr(), wd.data_ptr(), lo["cout"], lo["kh"], lo["kw"], lo["cin"], self._dy_channels(name),
                             wd.shape[0], total, 0])
                total += wd.numel()
            self._pack_table = (torch.tensor(rows, dtype=torch.int64, device=eng.device), len(rows), total, eng.wflat.data_ptr())
        table, n, total, _ = self._pack_table
        if n == 0:
            return
        eng.h.check(L.lib.rtn_pack_dgrad_weights_multi(eng.h.raw, table.data_ptr(), n, total, eng.rdt))

    def get_state(self):
        """The Keras-named state of the trained model: the engine's loaded state with every kernel (HWIO) and every Keras bias taken
        from the f32 master copy; the frozen BatchNorm arrays are the loaded ones.  A new dict of new arrays: what a checkpoint holds,
        and what Engine.load_state() turns back into these forward weights."""
        self._check_engine_state()
        eng, master = self.eng, self.master.cpu()
        state = dict(eng.state)
        for name, lo in eng.layout.items():
            wm = master[lo["woff"]:lo["woff"] + lo["rows"] * lo["K"]].view(lo["rows"], lo["K"])
            state[name + "/kernel"] = Wt.unpack_conv(name, lo, wm).contiguous().numpy()
            if lo["has_bias"]:
                bo = self.NW + lo["boff"]
                state[name + "/bias"] = master[bo:bo + lo["cout"]].clone().numpy()
        return state

    def grad_views(self, name):
        """(dW [rows][K] f32, db [rows] f32) views of the flat gradient buffer for one layer."""
        lo = self.eng.layout[name]
        return (self.grad[lo["woff"]:lo["woff"] + lo["rows"] * lo["K"]].view(lo["rows"], lo["K"]),
                self.grad[self.NW + lo["boff"]:self.NW + lo["boff"] + lo["rows"]])

    # ------------------------------------------------------------------ backward plan
    def _bplan(self, B, H, W):
        """The backward plan of a canvas, cached: the op list (bplan.Emit), the gradient buffers and the loss-side tensors."""
        key = (B, H, W)
        if key in self.bplans:
            self.eng._plan(B, H, W)                        # marks the canvas as recently used in the engine's cache
            return self.bplans[key]
        plan = self.eng._plan(B, H, W)                     # may evict the least recently used canvas: _drop_bplan() follows
        bp = self.bplans[key] = BP.Emit(self, plan, B).build()
        return bp

    # ------------------------------------------------------------------ backward lanes
    @staticmethod
    def _bop_io(b):
        """(pointers read, pointers written) of a backward op (accumulating outputs are both)."""
        return b.io()

    def _bschedule(self, bops, nwg, dyp_cls):
        """Lane of every backward op and the cross-lane events it must wait for.  Lane 0: the data-gradient chain; lanes
        1..nwg: weight / bias gradients (independent of each other: round-robin); lane nwg+1: the data gradients of the
        classification tower, which only meet the rest of the graph where the pyramid gradients are summed; lane nwg+2
        (RTN_BWD_EXTRA_LANE): the data gradients beside the forward graph's forks.  Events come from schedule_lanes;
        write-after-read hazards arise here (gradient buffers are accumulated in place by several ops)."""
        fixed = {O.MAIN: 0, O.CLS: nwg + 1, O.EXTRA: nwg + 2 if os.environ.get("RTN_BWD_EXTRA_LANE", "0") != "0" else 0}
        weight = itertools.cycle(range(1, nwg + 1))
        lanes = [next(weight) if cls == O.WEIGHT else fixed[cls] for cls in (b.lane(dyp_cls) for b in bops)]
        return schedule_lanes(lanes, [b.io() for b in bops])

    def forward_backward(self, images, regression_batch, labels_batch):
        """Forward, loss and backward; leaves dL/dparams in self.grad (flat f32) and returns the device tensor
        loss_sums = [sum focal terms, sum smooth-L1 terms, #positives (labels), #positives (regression)] of THIS rank."""
        self._check_engine_state()
        eng, lib = self.eng, L.lib
        h = eng.h
        B, H, W, _ = images.shape
        eng.training = True
        try:
            bp = self._bplan(B, H, W)
            # the full backward reads every extra output of the training forward; a pruned one maybe none (Engine._fused)
            eng.train_keep = None if self.trainable is None else bp["keep_fwd"]
            self.fwd_key = eng._fused()              # the fusion key this forward runs: the pool backward follows its stem
            reg, cls = eng.forward(images)
        finally:
            eng.training = False
            eng.train_keep = None
        N, K = bp["plan"]["N"], eng.K
        rows = B * N
        eng._bind_stream()
        h.check(lib.rtn_retina_loss_fwd(h.raw, rows, K, labels_batch.data_ptr(), regression_batch.data_ptr(), cls.data_ptr(),
                                        reg.data_ptr(), self.alpha, self.gamma, self.sigma, self.loss_sums.data_ptr(),
                                        bp["loss_ws"].data_ptr(), bp["loss_ws"].numel()))
        norm = self.loss_sums
        if self.pg is not None:                      # merged-batch normaliser (multi_gpu_model semantics)
            norm = Par.allreduce_loss_sums(self.loss_sums, self.pg)
        self.norm_sums = norm
        if not bp["bops"]:                           # every layer frozen: the loss alone, no backward kernel
            return self.loss_sums
        h.check(lib.rtn_retina_loss_bwd_dev(h.raw, rows, K, labels_batch.data_ptr(), regression_batch.data_ptr(), cls.data_ptr(),
                                            reg.data_ptr(), self.alpha, self.gamma, self.sigma, norm.data_ptr(), 1,
                                            bp["d_cls"].data_ptr(), bp["d_reg"].data_ptr()))
        self.grad.zero_()
        # Lanes (see _bschedule): data-gradient chain on the launch stream; weight / bias gradients round-robin over side streams;
        # the classification tower's data gradients on one more.  Events follow the per-buffer hazards.
        bops = bp["bops"]
        if not self.wgrad_lane:
            for bi, b in enumerate(bops):
                b.launch(self, bp, bi)
            return self.loss_sums
        main = torch.cuda.current_stream(eng.device)
        nwg = self.wgrad_lanes        # also under DP: the bucketer records one event per (bucket, lane) and waits for all of them
        sch = bp.get(("bsched", nwg))
        if sch is None:
            sch = bp[("bsched", nwg)] = self._bschedule(bops, nwg, bp["dyp_cls"])
            sch["ev"] = {i: torch.cuda.Event() for i in sch["events"]}
        if self._wg_stream is None:
            # lanes on hardware queues of their own as far as the runtime has them (Engine._concurrent_streams)
            self._wg_stream = eng._concurrent_streams(self.WG_LANES + 2, beside=(main,))
            self._wg_ev = torch.cuda.Event()
        # the fork (_wg_ev): side lanes start behind the loss backward and the gradient reset
        run_lanes(h, [main] + self._wg_stream, sch, sch["ev"], self._wg_ev, lambda bi, st: bops[bi].launch(self, bp, bi, st))
        return self.loss_sums

    def optimizer_step(self, lr=None):
        """Clipnorm + Adam over the trainable tensors' element ranges of the flat parameter vector (every layer's when trainable is
        None), re-emission of their forward and dgrad weights.  Slots outside the ranges (frozen layers, bias slots of layers without a
        Keras bias) are never read or written.  global_clip: the global sum lands in self.sumsq and one norm clips everything;
        otherwise one sum per range (a Keras weight tensor each) clips that range and the global sum is not computed."""
        if self._epoch != self.eng.load_epoch:
            raise RuntimeError("Engine.load_state() ran between forward_backward() and optimizer_step(): the gradient belongs to "
                               "the previous weights")
        eng, lib, h = self.eng, L.lib, self.eng.h
        eng.join()                                   # inference batches still in flight (Engine.in_flight > 1) read the weights rewritten below
        eng._bind_stream()
        if self.bucketer is not None:                # sum of per-rank gradients == gradient of the merged batch
            self.bucketer.finish()
        self.step_count += 1
        lr = self.lr if lr is None else lr
        rt = self._range_tables()
        tab, nr, span = rt["all"]
        if nr == 0:                                     # nothing trains: no kernel, the weights and their copies stay
            return
        n = self.NW + self.NB
        each = rt["each"]
        h.check(lib.rtn_sumsq_ranges(h.raw, self.grad.data_ptr(), self.gscale.data_ptr(), n, tab.data_ptr(), nr, span,
                                     self.sumsq.data_ptr() if self.global_clip else None, None if self.global_clip else each.data_ptr(),
                                     self.ss_ws.data_ptr(), self.ss_ws.numel()))
        nrw = rt["w"][1]
        for part, lo_, cnt, wf, code, sums in (("w", 0, self.NW, eng.wflat, eng.rdt, 0), ("b", self.NW, self.NB, eng.bflat, L.RTN_F32, nrw)):
            t, nrp, sp = rt[part]
            if nrp == 0:
                continue
            off4 = lo_ * 4
            args = (h.raw, self.master.data_ptr() + off4, self.m.data_ptr() + off4, self.v.data_ptr() + off4, self.grad.data_ptr() + off4,
                    self.gscale.data_ptr() + off4, self.fold.data_ptr() + off4, wf.data_ptr(), code, cnt, t.data_ptr(), nrp, sp,
                    self.step_count, lr, self.b1, self.b2, self.eps)
            if self.global_clip:
                h.check(lib.rtn_adam_clipnorm_step_ranges(*args, self.sumsq.data_ptr(), self.clipnorm, 1.0))
            else:
                h.check(lib.rtn_adam_clipnorm_step_ranges_pertensor(*args, each.data_ptr() + sums * 8, self.clipnorm, 1.0))
        self._repack_dgrad()
        eng.weights_version += 1                        # fused inference copies of the filters are stale now

    def _range_tables(self):
        """Element ranges of the trainable tensors (one per weight tensor, one per bias vector of a layer that owns a Keras bias):
        device tables for the whole flat vector (the norms), the weights and the biases (relative to NW), built once per trainable
        set and clipping mode.  Under global clipping no kernel asks which tensor an element belongs to, so adjacent tensors share
        a row (the full step: one row for all weights): the same elements in the same order, and next to no table search."""
        if self._ranges is None or self._ranges["global_clip"] != self.global_clip:
            dev = self.eng.device
            wr = [(lo["woff"], lo["woff"] + lo["rows"] * lo["K"]) for name, lo in self.eng.layout.items() if self._is_trainable(name)]
            br = [(lo["boff"], lo["boff"] + lo["rows"]) for name, lo in self.eng.layout.items()
                  if lo["has_bias"] and self._is_trainable(name)]
            allr = wr + [(self.NW + a, self.NW + b) for a, b in br]
            if self.global_clip:
                wr, br, allr = merge_adjacent(wr), merge_adjacent(br), merge_adjacent(allr)
            self._ranges = {"all": L.ranges_table(allr, dev), "w": L.ranges_table(wr, dev), "b": L.ranges_table(br, dev),
                            "each": torch.zeros(max(1, len(allr)), dtype=torch.float64, device=dev), "global_clip": self.global_clip}
        return self._ranges

    def train_on_batch(self, images, regression_batch, labels_batch, lr=None):
        """Keras-style step. Returns (total, regression_loss, classification_loss) as Python floats (one host sync)."""
        self.forward_backward(images, regression_batch, labels_batch)
        self.optimizer_step(lr)
        s = self.norm_sums.cpu().numpy()
        reg_loss = float(s[1] / max(1.0, s[3]))
        cls_loss = float(s[0] / max(1.0, s[2]))
        return reg_loss + cls_loss, reg_loss, cls_loss
