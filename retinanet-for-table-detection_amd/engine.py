"""Executor of the RetinaNet graph on librtn.so: one ctypes call per fused layer.

Graph (what a forward pass IS in the reference):
  resnet_retinanet (model/defineModel.py:357-389) -> keras_resnet backbone C3..C5
  __create_pyramid_features (:170-205) -> P3..P7
  regression / classification submodels on every level, concatenated (:208-228, :255-265)
  retinanet_bbox (:296-353): Anchors -> RegressBoxes -> ClipBoxes -> FilterDetections.
PyTorch is used for device memory and the stream only; all arithmetic is in the HIP library.
Frozen BN, bias, ReLU, the residual add, UpsampleLike+Add and the sigmoid are fused into the
convolution epilogues; the five pyramid levels of a head layer run as ONE grouped launch.
"""
import ctypes as C

import numpy as np
import os
import torch

from typing import Any, NamedTuple, Optional

from . import _lib as L
from . import ops as O
from . import weights as Wt
from .ops import SRC_DT as _SRC_DT

_TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32}
_RTN_DT = {"bf16": L.RTN_BF16, "f32": L.RTN_F32}


class Block(NamedTuple):
    """One bottleneck block of a plan: what _variant() needs to substitute its fused forms.  x: the block's input, sc: its shortcut
    (x itself in an identity block, branch1's output in a stage's first block), a / b2: the outputs of branch2a / branch2b, y: the
    block's output; i_*: indices of the block's convs in plan["ops"] (i_2a / i_2b None where the fp8 pairing owns them, i_b1 None in
    an identity block); step: the stride of branch2a and branch1."""
    stage: int; block: int; f: int; step: int; key: str; n2a: str; n2b: str; n2c: str; n1: Optional[str]
    x: Any; a: Any; b2: Any; sc: Any; y: Any; i_2a: Optional[int]; i_2b: Optional[int]; i_b1: Optional[int]; i_2c: int; Ho: int; Wo: int


def same_pad_before(n, k, s):
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2


class AnchorParams:
    """model/anchors.py:7-33 values (sizes/strides per level, float32 ratios/scales)."""

    def __init__(self, sizes=(32, 64, 128, 256, 512), strides=(8, 16, 32, 64, 128),
                 ratios=None, scales=None):
        self.sizes = list(sizes)
        self.strides = list(strides)
        self.ratios = np.array([0.5, 1, 2], np.float32) if ratios is None else np.asarray(ratios)
        self.scales = (np.array([2 ** 0, 2 ** (1.0 / 3.0), 2 ** (2.0 / 3.0)], np.float32)
                       if scales is None else np.asarray(scales))

    def num_anchors(self):
        return len(self.ratios) * len(self.scales)


def detect_flags(nms=True, class_specific_filter=True):
    """FilterDetections' switches (model/layers.py:200-264) -> the flags of rtn_decode_filter_nms_ex (0: the reference's pair)."""
    return (0 if nms else L.RTN_DET_NO_NMS) | (0 if class_specific_filter else L.RTN_DET_CLASS_AGNOSTIC)


class BoxLoss:
    """What Engine.detect(loss=...) needs to run the focal + smooth-L1 sums of one batch from its ground-truth boxes:
    device tensors in rtn_anchor_targets' layout - gt_boxes f64 (B, RTN_MAX_GT, 4) at network scale, gt_labels i32 (B, RTN_MAX_GT),
    gt_count i32 (B,), img_hw i32 (B, 2): each page's own resized (h, w) - uploaded in the caller's stream order before the call;
    `out`: the caller's f64 (num_images, 4) device array and `row`: the first of the B rows this batch writes."""

    def __init__(self, gt_boxes, gt_labels, gt_count, img_hw, out, row, alpha=0.25, gamma=2.0, sigma=3.0,
                 negative_overlap=0.4, positive_overlap=0.5):
        for t, dt, shape in ((gt_boxes, torch.float64, (L.RTN_MAX_GT, 4)), (gt_labels, torch.int32, (L.RTN_MAX_GT,)),
                             (gt_count, torch.int32, ()), (img_hw, torch.int32, (2,))):
            if t.device.type != "cuda" or t.dtype != dt or tuple(t.shape[1:]) != shape or t.shape[0] != gt_boxes.shape[0] \
                    or not t.is_contiguous():
                raise ValueError("BoxLoss: contiguous device tensors f64 (B,%d,4), i32 (B,%d), i32 (B,), i32 (B,2) expected"
                                 % (L.RTN_MAX_GT, L.RTN_MAX_GT))
        if out.device.type != "cuda" or out.dtype != torch.float64 or out.dim() != 2 or out.shape[1] != 4 or not out.is_contiguous():
            raise ValueError("BoxLoss: out must be a contiguous f64 (num_images, 4) device tensor")
        self.gt_boxes, self.gt_labels, self.gt_count, self.img_hw, self.out, self.row = gt_boxes, gt_labels, gt_count, img_hw, out, int(row)
        self.alpha, self.gamma, self.sigma = float(alpha), float(gamma), float(sigma)
        self.negative_overlap, self.positive_overlap = float(negative_overlap), float(positive_overlap)

    def tensors(self):
        return (self.gt_boxes, self.gt_labels, self.gt_count, self.img_hw, self.out)


def make_anchor_cfg(image_hw, params=None, levels=(3, 4, 5, 6, 7)):
    """rtn_anchor_cfg_t for a canvas: guess_shapes (model/anchors.py:155-165) + base anchors."""
    params = params or AnchorParams()
    cfg = L.AnchorCfg()
    cfg.nlevels = len(levels)
    cfg.A = params.num_anchors()
    off = 0
    for i, lv in enumerate(levels):
        h = (int(image_hw[0]) + 2 ** lv - 1) // 2 ** lv
        w = (int(image_hw[1]) + 2 ** lv - 1) // 2 ** lv
        cfg.H[i], cfg.W[i], cfg.stride[i] = h, w, params.strides[i]
        cfg.anchor_off[i] = off
        off += h * w * cfg.A
        base = L.generate_anchors_f64(params.sizes[i], params.ratios, params.scales)
        for a in range(cfg.A):
            for j in range(4):
                cfg.base[i][a][j] = float(base[a, j])
    for i in range(len(levels), L.RTN_MAX_GROUPS + 1):
        cfg.anchor_off[i] = off
    return cfg, off


def schedule_lanes(lanes, io):
    """Cross-lane events of an op list whose ops already have their HIP stream lanes.  io: per op, (pointers read, pointers
    written); null pointers are skipped.  An op waits for the ops on OTHER lanes it has a read-after-write, write-after-write or
    write-after-read hazard with - per lane only the latest, streams are in order.  The last op of every side lane is joined into
    lane 0.  Returns {lanes, waits: per op the indices it waits for, events: the ops that record one, joins, nlanes}."""
    writer, readers, waits = {}, {}, []
    for i, (reads, writes) in enumerate(io):
        reads = [p_ for p_ in reads if p_]
        writes = [p_ for p_ in writes if p_]
        deps = set()
        for ptr in reads + writes:
            j = writer.get(ptr)
            if j is not None and lanes[j] != lanes[i]:
                deps.add(j)
        for ptr in writes:
            deps.update(j for j in readers.get(ptr, ()) if lanes[j] != lanes[i])
        latest = {}
        for j in deps:
            latest[lanes[j]] = max(latest.get(lanes[j], -1), j)
        waits.append(sorted(latest.values()))
        for ptr in reads:
            readers.setdefault(ptr, []).append(i)
        for ptr in writes:
            writer[ptr] = i
            readers[ptr] = []
    last = {ln: i for i, ln in enumerate(lanes)}
    joins = sorted(i for ln, i in last.items() if ln != 0)
    events = set(j for w in waits for j in w) | set(joins)
    return {"lanes": lanes, "waits": waits, "events": events, "joins": joins, "nlanes": max(lanes) + 1}


def run_lanes(handle, streams, sched, events, fork, launch):
    """Run an op list on its lanes.  streams: one per lane, [0] the launch stream; sched: schedule_lanes' result; events: {op index:
    event} for sched["events"].  The side lanes start behind `fork`, recorded on the launch stream now; every op waits for its
    cross-lane events, runs as launch(index, stream) with the handle bound to its lane's stream (re-bound only when the stream
    changes) and records its event if another lane or the join waits for it; the last op of every side lane is joined into the
    launch stream, to which the handle is bound again."""
    main = streams[0]
    fork.record(main)
    for st in streams[1:sched["nlanes"]]:
        st.wait_event(fork)
    bound = None
    for i, (ln, waits) in enumerate(zip(sched["lanes"], sched["waits"])):
        st = streams[ln]
        for j in waits:
            st.wait_event(events[j])
        if bound is not st:
            handle.set_stream(st.cuda_stream)
            bound = st
        launch(i, st)
        if i in events:
            events[i].record(st)
    for j in sched["joins"]:
        main.wait_event(events[j])
    handle.set_stream(main.cuda_stream)


class Engine:
    def __init__(self, backbone="resnet50", num_classes=1, num_anchors=9, dtype="bf16", device=0, anchor_params=None):
        if not torch.cuda.is_available():
            raise RuntimeError("the RetinaNet engine needs a ROCm GPU: no CPU fallback exists")
        if backbone.split("_")[0] not in Wt.STAGE_BLOCKS:
            raise ValueError("Backbone ('{}') not in allowed backbones ({}).".format(backbone, list(Wt.STAGE_BLOCKS)))
        self.backbone = backbone.split("_")[0]
        self.K, self.A = int(num_classes), int(num_anchors)
        self.dtype = dtype
        self.tdt, self.rdt = _TORCH_DT[dtype], _RTN_DT[dtype]
        self.device = torch.device("cuda", device)
        self.h = L.Handle(device)
        self.anchor_params = anchor_params or AnchorParams()
        self.w = {}
        self.plans = {}
        # A plan owns every activation buffer, descriptor and workspace of one (batch, canvas): several GB at the benchmark sizes.
        # csv_generator.compute_inputs pads each batch to ITS largest page, so a data set with varied page shapes shows a new canvas
        # nearly every step: the cache keeps the `max_plans` most recently used canvases and frees the rest (RTN_MAX_PLANS).
        self.max_plans = max(1, int(os.environ.get("RTN_MAX_PLANS", "4")))
        # detect() with `in_flight` > 1: consecutive batches run on `in_flight` buffer sets, each on ONE HIP stream of its own, so the
        # next batch's backbone fills the CUs the current batch's small-M layers and kernel tails leave idle (see detect()).
        self.in_flight = 1
        self.last_slot = 0
        self.trace_in_flight = None
        self._slots, self._next_slot = [], 0
        self.on_plan_evict = []        # weakref.WeakMethod callbacks key -> None (a Trainer drops its backward plan of the same canvas)
        self.state = None
        self.training = False          # set by trainer.Trainer: the pool then records its argmax taps
        # set by trainer.Trainer around a training forward whose backward is pruned to the trainable layers: (keep branch2b of the
        # fused 64-channel blocks, record the pool's taps) - what that backward reads; None = both (the full backward)
        self.train_keep = None
        self.two_streams = os.environ.get("RTN_TWO_STREAMS", "1") != "0"    # graph forks on side HIP streams (_schedule)
        self.fuse_stem = os.environ.get("RTN_FUSE_STEM", "1") != "0"        # inference/bf16: conv1+ReLU+pool1 in one kernel
        self.fuse_stem_2a = os.environ.get("RTN_FUSE_STEM_2A", "1") != "0"  # ... which also applies res2a_branch2a to the pooled pixels
        # training/bf16: the same kernel also records the pool's winning taps; conv1's output is never written and the pool's
        # backward takes its ReLU mask from pool1 (trainer.py)
        self.fuse_stem_train = os.environ.get("RTN_FUSE_STEM_TRAIN", "1") != "0"
        self.fuse_shortcut = os.environ.get("RTN_FUSE_SHORTCUT", "1") != "0"  # inference: branch1 folded into branch2c (dual-source GEMM)
        # inference/bf16: the identity blocks of the 64-channel stage as one kernel each (rtn_bottleneck64_fwd: branch2b -> branch2c
        # + shortcut -> the next block's branch2a)
        self.fuse_bottleneck = os.environ.get("RTN_FUSE_BOTTLENECK", "1") != "0"
        # ... and res2b_branch2a appended to res2a's fused block (its projection form with the three per-chunk filter sets streamed)
        self.fuse_proj_tail = os.environ.get("RTN_FUSE_PROJ_TAIL", "1") != "0"
        # bf16: an identity block's branch2c + Add + ReLU and the next block's branch2a as one launch in the 128-channel stage
        # (rtn_chain1x1_fwd; the 256-channel instance measured no faster and left the library: profiles/r4_seam_kernel.txt)
        self.fuse_chain = os.environ.get("RTN_FUSE_CHAIN", "1") != "0"
        # detect(): nobody outside the network sees the backbone features, and stage 3 reads C2 only at its even pixels (both readers
        # are 1x1 / stride 2): res2b stores and res2c computes that quarter only (_fused(private=True); forward() keeps C2 whole)
        self.skip_unread_c2 = os.environ.get("RTN_SKIP_UNREAD_C2", "1") != "0"
        self.weights_version = 0
        self.load_epoch = 0            # bumped by load_state(): a live Trainer re-derives its master copy / plans from it
        self._dual, self._dual_version = {}, -1
        self._side = None
        self.fp8_scales = None         # set by calibrate_fp8(): the head towers then run in fp8 (inference, bf16 engine)
        self._w8, self._w8_version = {}, -1
        self.fp8_backbone = False      # calibrate_fp8(..., backbone=True): the 3x3 branch2b layers with >= 128 channels too

    # ------------------------------------------------------------------ weights
    def load_state(self, state):
        """state: Keras-named dict (see weights.py). Packs every conv (BN folded) into ONE flat device buffer of
        forward weights (dtype of the path) and one flat f32 bias buffer; per-layer tensors are views into them, so an
        optimizer can rewrite all weights with a single kernel (trainer.py)."""
        if any(s["done"] is not None for s in self._slots):
            torch.cuda.synchronize(self.device)          # batches in flight read the buffers released below
        self._slots, self._next_slot = [], 0
        self.state = state
        self.w = {}
        self.layout = {}
        packed, woff, boff = [], 0, 0
        for (name, kh, kw, cin, cout, has_bias, bn) in Wt.conv_layers(self.backbone, self.K, self.A):
            bnp = None if bn is None else [state[bn + s] for s in ("/gamma", "/beta", "/moving_mean", "/moving_variance")]
            bias = state.get(name + "/bias") if has_bias else None
            pack = Wt.pack_stem if name == "conv1" else Wt.pack_conv
            wk, bk = pack(state[name + "/kernel"], bias, bnp, self.tdt, "cpu")
            packed.append((name, wk, bk, kh, kw, cin, cout))
            self.layout[name] = {"woff": woff, "rows": wk.shape[0], "K": wk.shape[1], "boff": boff, "has_bias": has_bias,
                                 "bn": bn, "kh": kh, "kw": kw, "cin": cin, "cout": cout}
            woff += wk.numel()
            boff += bk.numel()
        self.wflat = torch.empty(woff, dtype=self.tdt, device=self.device)
        self.bflat = torch.empty(boff, dtype=torch.float32, device=self.device)
        for (name, wk, bk, kh, kw, cin, cout) in packed:
            lo = self.layout[name]
            wv = self.wflat[lo["woff"]:lo["woff"] + wk.numel()].view(wk.shape)
            bv = self.bflat[lo["boff"]:lo["boff"] + bk.numel()]
            wv.copy_(wk)
            bv.copy_(bk)
            self.w[name] = (wv, bv, kh, kw, cin, cout)
        self.plans = {}
        self.weights_version += 1
        self.load_epoch += 1

    def _dual_weights(self):
        """K-concatenated filters of every stage's first block: [branch2c | branch1] along K, biases summed
        (rtn_conv1x1_dual_fwd).  Copies of the flat forward weights: refreshed whenever those change (load_state, an
        optimizer step)."""
        if self._dual_version != self.weights_version:
            for stage in range(4):
                s = str(stage + 2)
                bname = Wt.block_name(self.backbone, stage, 0)
                wc, bc = self.w["res%s%s_branch2c" % (s, bname)][:2]
                w1, b1 = self.w["res%s%s_branch1" % (s, bname)][:2]
                key = "res%s%s" % (s, bname)
                if key not in self._dual:
                    self._dual[key] = (torch.empty(wc.shape[0], wc.shape[1] + w1.shape[1], dtype=wc.dtype, device=wc.device),
                                       torch.empty_like(bc))
                wd, bd = self._dual[key]
                wd[:, :wc.shape[1]].copy_(wc)
                wd[:, wc.shape[1]:].copy_(w1)
                torch.add(bc, b1, out=bd)
            self._dual_version = self.weights_version
        return self._dual

    # ------------------------------------------------------------------ fp8 head towers (BASELINE.json configs[4])
    TOWERS = ("pyramid_regression", "pyramid_classification")

    def _fp8_on(self):
        return self.fp8_scales is not None and self.dtype == "bf16" and not self.training

    def _fp8_layers(self):
        names = ["%s_%d" % (prefix, i) for prefix in self.TOWERS for i in range(4)]
        if self.fp8_backbone:
            for stage, nblocks in enumerate(Wt.STAGE_BLOCKS[self.backbone]):
                if 64 * 2 ** stage >= 128:                    # the halo kernel needs whole 128-byte channel chunks
                    names += ["res%d%s_branch2b" % (stage + 2, Wt.block_name(self.backbone, stage, b)) for b in range(nblocks)]
            names.append("P3")
        return names

    def _fp8_weights(self):
        """e4m3 copies of the fp8 layers' (BN-folded) filters, one scale per tensor (448 / max |w|); rebuilt when the weights change."""
        if self._w8_version != self.weights_version or any(n not in self._w8 for n in self._fp8_layers()):
            for name in self._fp8_layers():
                wk = self.w[name][0].float()
                sw = 448.0 / max(float(wk.abs().max()), 1e-30)
                wq = torch.clamp(wk * sw, -448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
                if name in self._w8 and self._w8[name][0].shape == wq.shape:
                    self._w8[name][0].copy_(wq)                        # descriptors of existing plans keep pointing at it
                    self._w8[name] = (self._w8[name][0], sw)
                else:
                    self._w8[name] = (wq, sw)
            self._w8_version = self.weights_version
        return self._w8

    def calibrate_fp8(self, images, margin=1.25, backbone=False):
        """Switch the two head towers (4 x [3x3 conv 256 + ReLU] each, model/defineModel.py:78-167 - 38 % of the network's FLOPs
        at 1024x1024 with ResNet-101) to fp8 e4m3: activations get ONE static scale per tensor, 448 / (margin x max |x|) over the
        five pyramid levels of a bf16 forward pass of `images`; weights one scale per layer.  The towers' first input is the
        quantised pyramid, their last layer writes bf16 for the (bf16) output convs.  backbone=True also runs every 3x3 branch2b
        layer with >= 128 channels in fp8: its producer branch2a writes e4m3 straight from its epilogue (rtn_conv2d_fwd_fp8out),
        branch2b writes bf16 for the 1x1 branch2c.  `images` may be a list of batches (scales from the maximum over all of
        them); calibrate_fp8(None) switches back."""
        self.fp8_scales = None
        self.fp8_backbone = bool(backbone) and images is not None
        self.plans = {k: v for k, v in self.plans.items() if not k[3]}     # bf16 plans (and a trainer's view of them) stay valid
        if images is None:
            return None
        if self.dtype != "bf16":
            raise ValueError("fp8 towers extend the bf16 engine")
        batches = list(images) if isinstance(images, (list, tuple)) else [images]     # several batches: the maximum over all
        amax = {}

        def see(key, tensors):
            amax[key] = max([amax.get(key, 0.0)] + [float(t.float().abs().max()) for t in tensors])

        for x in batches:
            B, H, W, _ = x.shape
            self.forward(x)
            torch.cuda.synchronize(self.device)
            plan = self._plan(B, H, W)
            see("in", plan["pyr"])
            for prefix, acts in plan["tower_acts"].items():
                for i, levels in enumerate(acts):
                    see((prefix, i), levels)
            if self.fp8_backbone:
                for name, a in plan["a_acts"].items():
                    see(("a", name), [a])
        scales = {k: 448.0 / (margin * max(v, 1e-20)) for k, v in amax.items()}
        self.fp8_scales = scales
        return scales

    def _conv8(self, name, groups, B, s_in, s_out, out_fp8, relu=True):
        """One fp8 layer (rtn_conv2d_fp8_fwd): bias (+ ReLU), fp8 or bf16 output."""
        wq, sw = self._fp8_weights()[name]
        _, bk, kh, kw, cin, cout = self.w[name]
        d = self._desc(groups, B, L.RTN_FP8, wq, bk, cout, kh, kw, cin, pad=((kh - 1) // 2, (kw - 1) // 2), flags=L.CONV_RELU if relu else 0)
        q = L.ConvFp8(acc_scale=1.0 / (s_in * sw), out_scale=s_out, out_dtype=L.RTN_FP8 if out_fp8 else L.RTN_BF16)
        meta = {"name": name, "xs": [g._x for g in groups], "ys": [g._out for g in groups], "res": [None] * len(groups),
                "kh": kh, "kw": kw, "cin": cin, "cout": cout, "B": B, "fp8": True, "s_in": s_in, "sw": sw}
        return O.Conv8("conv8", d, name, meta, q)

    # ------------------------------------------------------------------ descriptors
    def _group(self, x, out, Hout, Wout, res=None, out_off=0, out_img_stride=None, res_hw=None):
        g = L.ConvGroup()
        B, Hin, Win, Cin = x.shape
        g.in_ = x.data_ptr(); g.in_elems = x.numel()
        g.out = out.data_ptr(); g.out_elems = out.numel()
        g.in_img_stride = Hin * Win * Cin
        g.in_row_stride = Win * Cin
        g.Hin, g.Win, g.Hout, g.Wout = Hin, Win, Hout, Wout
        g.out_img_stride = out.numel() // B if out_img_stride is None else out_img_stride
        g.out_off = out_off
        if res is not None:
            g.res = res.data_ptr(); g.res_elems = res.numel()
            g.res_img_stride = res.numel() // B
            g.res_ld = res.shape[3]
            g.Hres, g.Wres = (res.shape[1], res.shape[2]) if res_hw is None else res_hw
        g._x, g._out, g._res, g._off = x, out, res, out_off       # python-side refs for the backward graph
        return g

    def _desc(self, groups, B, dtype, w, bias, N, kh, kw, cin, stride=1, pad=(0, 0), flags=0, out_ld=None):
        """A conv descriptor over `groups`: filters w [rows][kh * kw * cin], N output channels, `cin`-element pixels."""
        d = L.ConvDesc()
        for i, g in enumerate(groups):
            d.g[i] = g
        d.ngroups, d.batch, d.dtype = len(groups), B, dtype
        d.w, d.bias = w.data_ptr(), bias.data_ptr()
        d.w_rows, d.N, d.KH, d.KW = w.shape[0], N, kh, kw
        d.Crun = d.pix_stride = cin
        d.sy = d.sx = stride
        d.pad_t, d.pad_l = pad
        d.out_ld, d.flags = N if out_ld is None else out_ld, flags
        return d

    def _conv(self, name, groups, B, stride=1, pad=(0, 0), flags=0, out_ld=None):
        """One fused conv launch; the torch tensors behind the groups are kept in the op's meta for the backward graph."""
        wk, bk, kh, kw, cin, cout = self.w[name]
        d = self._desc(groups, B, self.rdt, wk, bk, cout, kh, kw, cin, stride, pad, flags, out_ld)
        L.attach_conv_workspace(self.h, d)                 # split-K / tail-split slabs (P6, P7, res4-sized grids): caller-owned
        meta = {"name": name, "xs": [g._x for g in groups], "ys": [g._out for g in groups], "res": [g._res for g in groups],
                "offs": [g._off for g in groups], "stride": stride, "pad": pad, "flags": flags,
                "relu": bool(flags & L.CONV_RELU), "kh": kh, "kw": kw, "cin": cin, "cout": cout, "B": B,
                "out_ld": d.out_ld}
        return O.Conv("conv", d, name, meta)

    def _dual_op(self, fb, B):
        """First block of a stage with the projection shortcut folded into branch2c: y = relu([W2c | W1] . [b2 ; x(step)] + b)."""
        wd, bd = self._dual_weights()[fb.key]
        d = self._desc([self._group(fb.b2, fb.y, fb.Ho, fb.Wo)], B, self.rdt, wd, bd, 4 * fb.f, 1, 1, fb.f, flags=L.CONV_RELU)
        x = fb.x
        s2 = L.ConvSrc2()
        s2.in_, s2.in_elems = x.data_ptr(), x.numel()
        s2.in_img_stride, s2.in_row_stride, s2.pix_stride = x.shape[1] * x.shape[2] * x.shape[3], x.shape[2] * x.shape[3], x.shape[3]
        s2.Hin, s2.Win, s2.C, s2.step = x.shape[1], x.shape[2], x.shape[3], fb.step
        L.attach_conv_workspace(self.h, d, s2)             # stream-K slabs of the small-M stages (res5a): caller-owned
        return O.Dual("dual", d, fb.key + "_branch2c+1", s2, {"xs": [fb.b2, x], "ys": [fb.y]})

    def _bneck_op(self, blk, nxt, B, keep_h1=False, xq=None, yq=None):
        """A block of the 64-channel stage as one launch (rtn_bottleneck64_fwd): branch2b + branch2c + Add + ReLU of `blk`, and
        branch2a of the following identity block `nxt` when there is one.  The stage's FIRST block takes branch2c and its projection
        shortcut as one product over the K-concatenated filters of _dual_weights() (p_in / wproj).  xq / yq (identity blocks): compact
        quarter tensors (the even pixels) that stand in for the shortcut / the block output (the library's x_in_step / x_out_step = 2)."""
        proj = blk.block == 0
        w2b, b2b = self.w[blk.n2b][:2]
        w2c, b2c = self._dual_weights()[blk.key] if proj else self.w[blk.n2c][:2]
        a, x, y = blk.a, blk.x if xq is None else xq, blk.y if yq is None else yq
        d = L.BottleneckDesc()
        d.a_in, d.a_in_elems = a.data_ptr(), a.numel()
        d.x_out, d.x_out_elems = y.data_ptr(), y.numel()
        d.w2b, d.b2b, d.w2c, d.b2c = w2b.data_ptr(), b2b.data_ptr(), w2c.data_ptr(), b2c.data_ptr()
        d.batch, d.H, d.W, d.mid, d.dtype = B, blk.Ho, blk.Wo, 64, self.rdt
        meta = {"xs": [a, x], "ys": [y], "B": B, "H": blk.Ho, "W": blk.Wo, "tail": nxt is not None, "h1": keep_h1}
        if proj:
            d.p_in, d.p_in_elems = x.data_ptr(), x.numel()
            d.wproj, d.w2c_ld = w2c.data_ptr() + 64 * w2c.element_size(), w2c.shape[1]
            meta["proj"] = True
        else:
            d.x_in, d.x_in_elems = x.data_ptr(), x.numel()
            d.x_in_step, d.x_out_step = meta["x_in_step"], meta["x_out_step"] = 1 if xq is None else 2, 1 if yq is None else 2
        if nxt is not None:
            w2a, b2a = self.w[nxt.n2a][:2]
            d.a_out, d.a_out_elems = nxt.a.data_ptr(), nxt.a.numel()
            d.w2a, d.b2a = w2a.data_ptr(), b2a.data_ptr()
            meta["ys"].append(nxt.a)
        if keep_h1:                                      # training: branch2b's activation is an input of the backward pass
            d.h1_out, d.h1_out_elems = blk.b2.data_ptr(), blk.b2.numel()
            meta["ys"].append(blk.b2)
        return O.Bneck("bneck", d, blk.n2b + ("+2c+1" if proj else "+2c") + ("+next2a" if nxt is not None else ""), meta)

    def _chain_op(self, blk, nxt):
        """The seam between two identity blocks of the 128- / 256-channel stages as one launch (rtn_chain1x1_fwd): branch2c + Add +
        ReLU of `blk`, branch2a + ReLU of `nxt`."""
        w2c, b2c = self.w[blk.n2c][:2]
        w2a, b2a = self.w[nxt.n2a][:2]
        h, x, y, a, f = blk.b2, blk.sc, blk.y, nxt.a, blk.f
        d = L.ChainDesc()
        d.h_in, d.h_in_elems, d.x_in, d.x_in_elems = h.data_ptr(), h.numel(), x.data_ptr(), x.numel()
        d.x_out, d.x_out_elems, d.a_out, d.a_out_elems = y.data_ptr(), y.numel(), a.data_ptr(), a.numel()
        d.w2c, d.b2c, d.w2a, d.b2a = w2c.data_ptr(), b2c.data_ptr(), w2a.data_ptr(), b2a.data_ptr()
        d.pixels, d.mid, d.out, d.next, d.dtype = y.numel() // y.shape[3], f, 4 * f, f, self.rdt
        return O.Chain("chain", d, blk.n2c + "+next2a", {"xs": [h, x], "ys": [y, a], "pixels": int(d.pixels), "mid": f})

    # ------------------------------------------------------------------ plan
    def _plan(self, B, H, W, slot=0):
        fp8_on = self._fp8_on()
        key = (B, H, W, fp8_on) if slot == 0 else (B, H, W, fp8_on, slot)      # slot: buffer set of a batch in flight (detect())
        if key in self.plans:
            self.plans[key] = self.plans.pop(key)          # most recently used last
            return self.plans[key]
        if self.state is None:
            raise RuntimeError("load_state() first")
        if len(self.plans) >= self.max_plans:
            # least recently used canvases go.  Their buffers may still be read by launches in flight on the side streams, and the
            # caching allocator would hand the memory to this plan's tensors on the current stream: drain the device first (a new
            # canvas costs a plan build anyway).
            torch.cuda.synchronize(self.device)
            while len(self.plans) >= self.max_plans:
                old = next(iter(self.plans))
                self.on_plan_evict = [r for r in self.on_plan_evict if r() is not None]     # weak references to bound methods
                for r in self.on_plan_evict:
                    r()(old)
                del self.plans[old]
        dev, tdt = self.device, self.tdt
        ops, keep = [], []

        def buf(*shape, dtype=None):
            t = torch.empty(*shape, dtype=dtype or tdt, device=dev)
            keep.append(t)
            return t

        # ---- stem: pack to [B][Hp][Wp][4], then 7x7/2 as an 8x1 implicit GEMM over 32-element runs
        H1, W1 = (H + 1) // 2, (W + 1) // 2
        Hp = max(H + 6, 2 * (H1 - 1) + 8)
        Wp = max(W + 6, 2 * (W1 - 1) + 8)
        Wp += Wp & 1
        xin = {"B": B, "H": H, "W": W, "Hp": Hp, "Wp": Wp}
        xp = torch.zeros(B * Hp * Wp * 4 + 64, dtype=tdt, device=dev)     # +64: the last pixel's 32-run stays in bounds
        keep.append(xp)
        c1 = buf(B, H1, W1, 64)
        wk, bk, *_ = self.w["conv1"]
        g = L.ConvGroup()
        g.in_ = xp.data_ptr(); g.in_elems = xp.numel()
        g.out = c1.data_ptr(); g.out_elems = c1.numel()
        g.in_img_stride, g.in_row_stride = Hp * Wp * 4, Wp * 4
        g.Hin, g.Win, g.Hout, g.Wout = Hp, Wp, H1, W1
        g.out_img_stride = H1 * W1 * 64
        d = self._desc([g], B, self.rdt, wk, bk, 64, 8, 1, 32, stride=2, flags=L.CONV_RELU)
        d.pix_stride = 4                                   # a 32-element run spans eight packed pixels
        ops.append(O.Pack("pack", xp, xin))
        ops.append(O.Conv("conv", d, "conv1", {"name": "conv1", "xs": [xp], "ys": [c1], "res": [None], "offs": [0], "stride": 2,
                                               "pad": (0, 0), "flags": L.CONV_RELU, "relu": True, "kh": 8, "kw": 1, "cin": 32,
                                               "cout": 64, "B": B, "out_ld": 64, "stem": True}))
        # ---- pool1
        H2, W2 = (H1 + 1) // 2, (W1 + 1) // 2
        x = buf(B, H2, W2, 64)
        pool_idx = torch.empty(B * H2 * W2 * 64, dtype=torch.uint8, device=dev)     # winning taps (training mode only)
        keep.append(pool_idx)
        ops.append(O.Pool("pool", c1, x, (B, H1, W1, 64), pool_idx))
        # inference, bf16: the three stem ops above collapse into one kernel (rtn_stem_conv_pool); tail: set with fuse_stem == 2
        stem_fused = O.Stem("stem", x, (B, H, W), wk, bk, xp, (Hp, Wp), None, pool_idx)
        n_stem_ops = len(ops)
        # ---- bottleneck stages
        feats = []
        blocks = []                      # one Block per bottleneck block: what _variant() fuses
        a_acts = {}
        for stage, nblocks in enumerate(Wt.STAGE_BLOCKS[self.backbone]):
            f = 64 * 2 ** stage
            for block in range(nblocks):
                res = "res%d%s" % (stage + 2, Wt.block_name(self.backbone, stage, block))
                st = 2 if (block == 0 and stage > 0) else 1
                Hi, Wi = x.shape[1], x.shape[2]
                Ho, Wo = (Hi - 1) // st + 1, (Wi - 1) // st + 1
                n2a, n2b, n2c, n1 = res + "_branch2a", res + "_branch2b", res + "_branch2c", res + "_branch1" if block == 0 else None
                fp8_pair = fp8_on and ("a", n2a) in self.fp8_scales
                a = buf(B, Ho, Wo, f, dtype=torch.uint8 if fp8_pair else None)
                c2a = self._conv(n2a, [self._group(x, a, Ho, Wo)], B, stride=st, flags=L.CONV_RELU)
                b2 = buf(B, Ho, Wo, f)
                if fp8_pair:                                      # branch2a -> e4m3 -> fp8 branch2b -> bf16
                    sa = self.fp8_scales[("a", n2a)]
                    ops += [O.ConvQ("convq", *c2a[1:], sa), self._conv8(n2b, [self._group(a, b2, Ho, Wo)], B, sa, 1.0, out_fp8=False)]
                else:
                    ops += [c2a, self._conv(n2b, [self._group(a, b2, Ho, Wo)], B, pad=(1, 1), flags=L.CONV_RELU)]
                    if f >= 128:
                        a_acts[n2a] = a
                i_2b = len(ops) - 1
                sc = x
                if block == 0:
                    sc = buf(B, Ho, Wo, 4 * f)
                    ops.append(self._conv(n1, [self._group(x, sc, Ho, Wo)], B, stride=st))
                y = buf(B, Ho, Wo, 4 * f)
                ops.append(self._conv(n2c, [self._group(b2, y, Ho, Wo, res=sc)], B, flags=L.CONV_RELU | L.CONV_RES_SAME))
                blocks.append(Block(stage, block, f, st, res, n2a, n2b, n2c, n1, x, a, b2, sc, y, None if fp8_pair else i_2b - 1,
                                    None if fp8_pair else i_2b, i_2b + 1 if block == 0 else None, len(ops) - 1, Ho, Wo))
                x = y
            feats.append(x)
        C3, C4, C5 = feats[1], feats[2], feats[3]
        # ---- FPN (model/defineModel.py:183-203)
        def hw(t):
            return t.shape[1], t.shape[2]
        P5r = buf(B, *hw(C5), 256)
        ops.append(self._conv("C5_reduced", [self._group(C5, P5r, *hw(C5))], B))
        P5 = buf(B, *hw(C5), 256)
        ops.append(self._conv("P5", [self._group(P5r, P5, *hw(C5))], B, pad=(1, 1)))
        P4m = buf(B, *hw(C4), 256)
        ops.append(self._conv("C4_reduced", [self._group(C4, P4m, *hw(C4), res=P5r)], B, flags=L.CONV_RES_UPSAMPLE))
        P4 = buf(B, *hw(C4), 256)
        ops.append(self._conv("P4", [self._group(P4m, P4, *hw(C4))], B, pad=(1, 1)))
        p3_fp8 = fp8_on and ("a", "C3_reduced") in self.fp8_scales
        P3m = buf(B, *hw(C3), 256, dtype=torch.uint8 if p3_fp8 else None)
        c3r = self._conv("C3_reduced", [self._group(C3, P3m, *hw(C3), res=P4m)], B, flags=L.CONV_RES_UPSAMPLE)
        P3 = buf(B, *hw(C3), 256, dtype=torch.uint8 if p3_fp8 else None)
        if p3_fp8:        # P3's input has no other reader and P3 itself only feeds the towers: C3_reduced -> e4m3 -> fp8 P3 -> e4m3
            s3 = self.fp8_scales[("a", "C3_reduced")]
            ops += [O.ConvQ("convq", *c3r[1:], s3),
                    self._conv8("P3", [self._group(P3m, P3, *hw(C3))], B, s3, self.fp8_scales["in"], out_fp8=True, relu=False)]
        else:
            ops += [c3r, self._conv("P3", [self._group(P3m, P3, *hw(C3))], B, pad=(1, 1))]
            a_acts["C3_reduced"] = P3m
        H6, W6 = (C5.shape[1] + 1) // 2, (C5.shape[2] + 1) // 2
        P6 = buf(B, H6, W6, 256)
        ops.append(self._conv("P6", [self._group(C5, P6, H6, W6)], B, stride=2,
                              pad=(same_pad_before(C5.shape[1], 3, 2), same_pad_before(C5.shape[2], 3, 2))))
        P6r = buf(B, H6, W6, 256)
        ops.append(O.Relu("relu", P6, P6r))
        H7, W7 = (H6 + 1) // 2, (W6 + 1) // 2
        P7 = buf(B, H7, W7, 256)
        ops.append(self._conv("P7", [self._group(P6r, P7, H7, W7)], B, stride=2,
                              pad=(same_pad_before(H6, 3, 2), same_pad_before(W6, 3, 2))))
        pyr = [P3, P4, P5, P6, P7]
        # ---- anchors / outputs
        cfg, N = make_anchor_cfg((H, W), self.anchor_params)
        for i, p in enumerate(pyr):
            if (p.shape[1], p.shape[2]) != (cfg.H[i], cfg.W[i]):
                raise RuntimeError("pyramid level %d is %s, anchors expect %s" % (i + 3, hw(p), (cfg.H[i], cfg.W[i])))
        regression = buf(B, N, 4, dtype=torch.float32)
        classification = buf(B, N, self.K, dtype=torch.float32)
        # ---- heads: every layer is ONE grouped launch over the five levels (weights shared, :217)
        tower_ranges = []
        tower_acts = {}
        if fp8_on:                                       # the pyramid, quantised once for both towers
            pyr8 = [p if p.dtype == torch.uint8 else buf(B, *hw(p), 256, dtype=torch.uint8) for p in pyr]
            for p, p8 in zip(pyr, pyr8):
                if p8 is not p:
                    ops.append(O.Quant("quant", p, p8, self.fp8_scales["in"]))
        for prefix, out_t, per_anchor, last_flags in (("pyramid_regression", regression, 4, L.CONV_OUT_F32),
                                                      ("pyramid_classification", classification, self.K,
                                                       L.CONV_OUT_F32 | L.CONV_SIGMOID)):
            tower_start = len(ops)
            cur = pyr8 if fp8_on else pyr
            tower_acts[prefix] = []
            for i in range(4):
                if fp8_on:
                    nxt = [buf(B, *hw(p), 256, dtype=torch.uint8 if i < 3 else tdt) for p in pyr]
                    groups = [self._group(ci, ni, *hw(ci)) for ci, ni in zip(cur, nxt)]
                    s_in = self.fp8_scales["in"] if i == 0 else self.fp8_scales[(prefix, i - 1)]
                    ops.append(self._conv8("%s_%d" % (prefix, i), groups, B, s_in, self.fp8_scales[(prefix, i)], out_fp8=i < 3))
                else:
                    nxt = [buf(B, *hw(p), 256) for p in pyr]
                    groups = [self._group(ci, ni, *hw(ci)) for ci, ni in zip(cur, nxt)]
                    ops.append(self._conv("%s_%d" % (prefix, i), groups, B, pad=(1, 1), flags=L.CONV_RELU))
                tower_acts[prefix].append(nxt)
                cur = nxt
            groups = [self._group(ci, out_t, *hw(ci), out_off=cfg.anchor_off[l] * per_anchor, out_img_stride=N * per_anchor)
                      for l, ci in enumerate(cur)]
            ops.append(self._conv(prefix, groups, B, pad=(1, 1), flags=last_flags, out_ld=self.A * per_anchor))
            tower_ranges.append((tower_start, len(ops)))
        ws_bytes = L.lib.rtn_detect_workspace_bytes(B, N, self.K)
        # what _variant() substitutes: the fused ops of a fusion key are built on its first use
        fusion = {"stem": stem_fused, "n_stem_ops": n_stem_ops, "blocks": blocks}
        plan = {"ops": ops, "towers": tower_ranges, "tower_acts": tower_acts, "a_acts": a_acts, "fp8": fp8_on, "sched": self._schedule(ops),
                "keep": keep, "fusion": fusion, "variants": {}, "xin": xin, "cfg": cfg, "N": N, "regression": regression,
                "classification": classification, "pyr": pyr, "feats": feats,
                "det_ws": torch.empty(ws_bytes, dtype=torch.uint8, device=dev), "det_ws_bytes": ws_bytes,
                "boxes": torch.empty(B, L.RTN_MAX_DET, 4, dtype=torch.float32, device=dev),
                "scores": torch.empty(B, L.RTN_MAX_DET, dtype=torch.float32, device=dev),
                "labels": torch.empty(B, L.RTN_MAX_DET, dtype=torch.int32, device=dev)}
        self.plans[key] = plan
        return plan

    def _variant(self, plan, key):
        """{ops, sched, events} that forward() runs under the fusion key (fs, fd, fk, fc, fp, ft, fq) of _fused(): built on first use
        and kept in the plan.  The all-zero key is the plan's own op list and schedule."""
        rec = plan["variants"].get(key)
        if rec is not None:
            return rec
        if not any(key):
            ops, sched = plan["ops"], plan["sched"]
        else:
            fs, fd, fk, fc, fp, ft, fq = key
            fu, B = plan["fusion"], plan["xin"]["B"]
            blocks = fu["blocks"]
            first_blocks = [b for b in blocks if b.block == 0]
            blocks64 = [b for b in blocks if b.f == 64 and b.block > 0 and b.i_2b is not None]      # identity blocks of the 64-channel stage
            v = list(plan["ops"])
            if fc:                                   # consecutive identity blocks of a stage: branch2c + the next branch2a as one launch
                for blk, nxt in zip(blocks, blocks[1:]):
                    if blk.stage == nxt.stage and blk.block >= 1 and blk.i_2a is not None and nxt.i_2a is not None \
                            and L.lib.rtn_chain1x1_supported(blk.f, 4 * blk.f, blk.f):
                        v[blk.i_2c] = self._chain_op(blk, nxt)
                        v[nxt.i_2a] = None
            if fd:
                # one set per plan, shared by its variants: dual ops run on lane 0, a plan's variants run in stream order, and every
                # in-flight slot has a plan of its own
                if "dual_ops" not in plan:
                    plan["dual_ops"] = [self._dual_op(fb, B) for fb in first_blocks]
                for fb, op in zip(first_blocks, plan["dual_ops"]):
                    v[fb.i_2c] = op
                    v[fb.i_b1] = None
            if fk:                                   # with fd, res2a too: branch2b + [branch2c | branch1] + ReLU as one launch
                fused = [fb for fb in first_blocks if fd and fb.f == 64 and fb.step == 1 and fb.i_2b is not None] + blocks64
                for blk in fused:
                    # the next block's branch2a rides along (blocks64[k] is block k + 1; res2a takes res2b's only under fp)
                    nxt = blocks64[blk.block] if blk.block < len(blocks64) and (blk.block or fp) else None
                    v[blk.i_2b] = self._bneck_op(blk, nxt, B, keep_h1=fk == 2)
                    v[blk.i_2c] = None
                    if nxt is not None:
                        v[nxt.i_2a] = None
            if fq:
                # C2 is read at its even pixels only (res3a's branch2a and branch1: 1x1, stride 2).  The stage's last block computes
                # and writes that quarter, the block before it stores the matching quarter of its output (whose only reader in
                # memory is the last block's shortcut), and res3a reads the compact C2 with stride 1.
                prev, last = blocks64[-2], blocks64[-1]
                fb3 = [fb for fb in first_blocks if fb.x is last.y][0]
                if "c2_quarter" not in plan:                  # two tensors a quarter of C2 each, shared by the variants like dual_ops
                    hq, wq = (last.Ho + 1) // 2, (last.Wo + 1) // 2
                    plan["c2_quarter"] = [torch.empty(B, hq, wq, 256, dtype=self.tdt, device=self.device) for _ in range(2)]
                    plan["keep"] += plan["c2_quarter"]
                    xq, c2q = plan["c2_quarter"]
                    plan["c2_quarter_ops"] = (self._bneck_op(prev, last, B, yq=xq), self._bneck_op(last, None, B, xq=xq, yq=c2q),
                                              self._conv(fb3.n2a, [self._group(c2q, fb3.a, fb3.Ho, fb3.Wo)], B, flags=L.CONV_RELU),
                                              self._dual_op(fb3._replace(x=c2q, step=1), B))
                v[prev.i_2b], v[last.i_2b], v[fb3.i_2a], v[fb3.i_2c] = plan["c2_quarter_ops"]
            if fs:
                sf = fu["stem"]
                fb0 = first_blocks[0]
                if fs == 2 and fb0.f == 64 and fb0.step == 1 and fb0.i_2a is not None and v[fb0.i_2a] is not None:
                    # the pooled pixels go through res2a_branch2a before they leave the registers
                    sf = sf._replace(tail=(fb0.a,) + tuple(self.w[fb0.n2a][:2]))
                    v[fb0.i_2a] = None
                v = [v[0], sf] + v[fu["n_stem_ops"]:]              # pack, then conv1 + ReLU + pool1 as one launch
            ops = [op for op in v if op is not None]
            sched = self._schedule(ops)
        rec = {"ops": ops, "sched": sched, "events": {i: torch.cuda.Event() for i in sched["events"]}}
        plan["variants"][key] = rec
        return rec

    # ------------------------------------------------------------------ lanes: the records of ops.py say what an op reads, where it runs, how
    @staticmethod
    def _op_io(op):
        """(tensors read, tensors written) of a plan op, as data pointers."""
        return op.io()

    @staticmethod
    def _lane_of(op):
        """HIP stream lane of an op: 0 except at the graph's forks (ops._conv_lane)."""
        return op.lane()

    @staticmethod
    def _schedule(ops):
        """Lanes of a forward op list and their events (schedule_lanes).  Every tensor of a plan is written by exactly one op of a
        forward pass, so only read-after-write hazards arise inside a pass; passes are joined on lane 0."""
        return schedule_lanes([op.lane() for op in ops], [op.io() for op in ops])

    # ------------------------------------------------------------------ run
    def _bind_stream(self):
        self.h.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def forward(self, images, private=False):
        """images: device tensor (B,H,W,3), float32 / bfloat16 (already normalised) or uint8 (raw 3-channel
        distance-transform page: the x/127.5-1 of model/utils.py:43-46 is fused into the stem packer).
        Returns device tensors regression (B,N,4) f32, classification (B,N,K) f32 — the training
        model's outputs in the reference's order (model/defineModel.py:244-249).
        The returned tensors are the plan's OWN output buffers for this (B,H,W): the next forward()/detect() call with the
        same shape overwrites them (no allocation per step).  Clone what must outlive the next call
        (Model.predict_on_batch copies to the host).
        private: the caller reads nothing but the two outputs (detect()), so launches may leave out what only plan["feats"] shows."""
        if images.device.type != "cuda" or images.dim() != 4 or images.shape[3] != 3:
            raise ValueError("images must be a (B,H,W,3) tensor on the GPU")
        if images.dtype not in _SRC_DT:
            raise ValueError("unsupported image dtype %s" % images.dtype)
        images = images.contiguous()
        B, H, W, _ = images.shape
        if self._fp8_on() and self._w8_version != self.weights_version:
            self.plans = {k: v for k, v in self.plans.items() if not k[3]}      # new filters: new weight scales in the fp8 ops
        plan = self._plan(B, H, W)
        self._bind_stream()
        key = self._fused(private)
        if key[1]:
            self._dual_weights()                         # refresh the concatenated filters if the weights changed
        var = self._variant(plan, key)
        ops = var["ops"]
        if not self.two_streams:
            for op in ops:
                self._run_op(op, images)
            return plan["regression"], plan["classification"]
        main = torch.cuda.current_stream(self.device)
        if self._side is None:                               # three lanes that do not share a hardware queue with each other or with `main`
            self._side = self._concurrent_streams(3, beside=(main,))
        # the fork: side lanes start after everything queued before this pass
        run_lanes(self.h, [main] + self._side, var["sched"], var["events"], plan.setdefault("fork", torch.cuda.Event()),
                  lambda i, st: self._run_op(ops[i], images))
        return plan["regression"], plan["classification"]

    def _fused(self, private=False):
        """Fusion key (fs, fd, fk, fc, fp, ft, fq) of the engine's state, the variant of a plan that forward() runs (_variant): stem fused
        (0 / 1 / 2 = with res2a_branch2a), shortcut folded, 64-channel bottleneck blocks fused (1 / 2 = keeping branch2b's output),
        stage-3 seams chained, res2b_branch2a appended to res2a's block, the pool's winning taps recorded.  A training forward whose
        backward never reaches the stem or the 64-channel stage (frozen layers, train_keep) runs those launches in their inference
        form: fk = 1, ft = 0 - the same bits, fewer stores.  Training keeps
        every bottleneck tensor (the backward reads them) and, in fp32, conv1 / pool1 separate; the folded
        shortcut is used there too - no gradient needs the shortcut TENSOR, only its input and filters.  The fused stem and the fused
        bottleneck exist for bf16 only; the fp8 plan keeps its own branch2a / branch2b pairing.
        fq (only with `private`, i.e. from detect(): the backbone features stay inside the network): with the fused blocks in their
        inference form and the shortcut folded, C2 and res2b's output exist only at the even pixels that stage 3 reads."""
        stem16 = self.dtype == "bf16" and (not self.training or self.fuse_stem_train)
        keep_h1, ft = (self.train_keep or (True, True)) if self.training else (False, False)
        fk = 0
        if self.fuse_bottleneck and self.dtype == "bf16" and not self._fp8_on():
            fk = 2 if keep_h1 else 1                     # training: the fused blocks also store branch2b's output for the backward pass
        fs = (2 if self.fuse_stem_2a else 1) if (self.fuse_stem and stem16) else 0
        # (training too: both tensors of a seam are written, which is all the backward pass reads)
        fc = 1 if (self.fuse_chain and self.dtype == "bf16" and not self._fp8_on()) else 0
        fp = 1 if (self.fuse_proj_tail and fk and self.fuse_shortcut) else 0
        fq = 1 if (private and self.skip_unread_c2 and fk == 1 and self.fuse_shortcut and not self.training) else 0
        return (fs, self.fuse_shortcut, fk, fc, fp, int(ft), fq)

    def _taps(self):
        """The pool (or the fused stem) records its winning taps: a training forward whose backward runs the pool's backward."""
        return self.training and (self.train_keep is None or bool(self.train_keep[1]))

    def active_ops(self, plan, private=False):
        """The op list forward() executes; private: the one detect() executes (the same launches, one for one)."""
        return self._variant(plan, self._fused(private))["ops"]

    def _run_op(self, op, images):
        op.launch(self, images)

    def profile_ops(self, images, reps=1):
        """Per-op device time: events recorded on the launch stream around every op of `reps` forward passes.
        Returns [(kind, total_ms_over_reps)] in execution order, plus ("detect", ms) for the post-processing."""
        images = images.contiguous()
        B, H, W, _ = images.shape
        plan = self._plan(B, H, W)
        self._bind_stream()
        ops = self.active_ops(plan, private=True)            # what detect() runs
        totals = [0.0] * (len(ops) + 1)
        for _ in range(reps):
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(ops) + 2)]
            evs[0].record()
            for i, op in enumerate(ops):
                self._run_op(op, images)
                evs[i + 1].record()
            self.postprocess(plan["cfg"], plan["regression"], plan["classification"], H, W, plan["boxes"], plan["scores"],
                             plan["labels"], plan["det_ws"])
            evs[-1].record()
            torch.cuda.synchronize()
            for i in range(len(ops) + 1):
                totals[i] += evs[i].elapsed_time(evs[i + 1])
        return [(op.kind, totals[i]) for i, op in enumerate(ops)] + [("detect", totals[-1])]

    def detect(self, images, score_threshold=0.05, nms_threshold=0.5, max_detections=300, nms=True, class_specific_filter=True,
               loss=None):
        """Inference model outputs [boxes (B,300,4), scores (B,300), labels (B,300)] (model/defineModel.py:310-315).
        Views of the plan's output buffers: overwritten by the next call with the same (B,H,W) - clone to keep them.
        nms / class_specific_filter: FilterDetections' two switches (model/layers.py:200-264); the defaults are the reference's.

        in_flight > 1 (throughput mode; default 1): the call enqueues this batch on the next of `in_flight` buffer sets and returns at
        once; batches of consecutive calls then overlap on the device (separate HIP streams, one per buffer set: stage-4/5 layers
        use 44-175 of 256 CUs and every kernel has a tail - the neighbouring batch's kernels run there; measured 4.07 -> 3.57 ms per
        batch of 8 at 800x1333, profiles/r4_in_flight.txt).  The page tensor is consumed in the caller's stream order (the stem packer
        runs on the caller's stream), so it may be overwritten as soon as the call returns.  The returned views belong to the buffer
        set: valid after join() (or any device synchronisation) and until the in_flight-th call after this one.

        loss (a BoxLoss): the same forward also feeds the validation loss - rtn_retina_loss_boxes_fwd runs on this batch's
        regression / classification outputs, on the stream that ran the forward, beside postprocess, and writes its (B,4) rows at
        loss.row of loss.out.  Nothing is read back."""
        md = int(max_detections)
        if not 1 <= md <= L.RTN_MAX_DET:
            raise ValueError("max_detections must be in [1, %d]" % L.RTN_MAX_DET)
        flags = detect_flags(nms, class_specific_filter)
        if self.in_flight > 1 and not self.training:
            return self._detect_in_flight(images, score_threshold, nms_threshold, md, flags, loss)
        reg, cls = self.forward(images, private=True)
        B, H, W, _ = images.shape
        plan = self._plan(B, H, W)
        # the library writes (B, max_detections, .) densely: hand it views of that shape over the plan's buffers
        boxes = plan["boxes"].view(-1)[:B * md * 4].view(B, md, 4)
        scores = plan["scores"].view(-1)[:B * md].view(B, md)
        labels = plan["labels"].view(-1)[:B * md].view(B, md)
        self.postprocess(plan["cfg"], reg, cls, H, W, boxes, scores, labels, plan["det_ws"], score_threshold, nms_threshold, md, flags)
        if loss is not None:
            self.loss_from_boxes(plan, loss)
        return boxes, scores, labels

    def loss_from_boxes(self, plan, loss):
        """rtn_retina_loss_boxes_fwd on the outputs `plan` holds, on the current stream: per image {focal sum, smooth-L1 sum,
        positives, positives} into rows loss.row .. loss.row + B of loss.out (csrc/rtn_loss.hip).  The workspace belongs to the
        plan (one per buffer set), so batches in flight on different sets do not share it."""
        self._bind_stream()
        reg, cls = plan["regression"], plan["classification"]
        B, N, K = cls.shape
        if loss.gt_boxes.shape[0] != B or loss.row < 0 or loss.row + B > loss.out.shape[0]:
            raise ValueError("BoxLoss: %d images of ground truth at row %d of %d for a batch of %d"
                             % (loss.gt_boxes.shape[0], loss.row, loss.out.shape[0], B))
        need = int(L.lib.rtn_retina_loss_boxes_workspace_bytes(B, N))
        ws = plan.get("loss_ws")
        if ws is None or ws.numel() < need:
            ws = plan["loss_ws"] = torch.empty(need, dtype=torch.uint8, device=self.device)
        cur = torch.cuda.current_stream(self.device)
        for t in loss.tensors():
            t.record_stream(cur)
        self.h.check(L.lib.rtn_retina_loss_boxes_fwd(self.h.raw, C.byref(plan["cfg"]), B, K, loss.gt_boxes.data_ptr(),
                                                     loss.gt_labels.data_ptr(), loss.gt_count.data_ptr(), loss.img_hw.data_ptr(),
                                                     loss.negative_overlap, loss.positive_overlap, cls.data_ptr(), reg.data_ptr(),
                                                     loss.alpha, loss.gamma, loss.sigma, loss.out[loss.row:].data_ptr(),
                                                     ws.data_ptr(), ws.numel()))

    def _detect_in_flight(self, images, score_threshold, nms_threshold, md, flags=0, loss=None):
        if images.device.type != "cuda" or images.dim() != 4 or images.shape[3] != 3:
            raise ValueError("images must be a (B,H,W,3) tensor on the GPU")
        if images.dtype not in _SRC_DT:
            raise ValueError("unsupported image dtype %s" % images.dtype)
        images = images.contiguous()
        B, H, W, _ = images.shape
        if len(self._slots) != self.in_flight:
            self.join()
            self._slots = [{"stream": st_, "done": None, "fed": torch.cuda.Event()} for st_ in self._concurrent_streams(self.in_flight)]
            self._next_slot = 0
        si = self._next_slot
        self._next_slot = (si + 1) % self.in_flight
        self.last_slot = si                                  # wait_slot(last_slot): the host waits for THIS batch only
        slot = self._slots[si]
        if self._fp8_on() and self._w8_version != self.weights_version:
            self.join()
            self.plans = {k: v for k, v in self.plans.items() if not k[3]}
        plan = self._plan(B, H, W, slot=si + 1)             # slot 0 is forward()'s / the one-batch path's own buffer set
        key = self._fused(private=True)
        caller = torch.cuda.current_stream(self.device)
        if key[1] and self._dual_version != self.weights_version:
            self.join()                                       # new weights: the concatenated filters are rewritten on the caller's
            self._dual_weights()                              # stream - nothing may be in flight on the old ones, and the batches
            caller.synchronize()                              # that follow on other streams must see the new ones
        ops = self._variant(plan, key)["ops"]
        if slot.get("consumed") is not None:
            # the packer below rewrites this buffer set's packed image: its previous batch must have read it (the stem, that batch's
            # first kernel on the slot's stream).  NOT the whole previous batch: that would chain the slots through the caller's
            # stream and keep the batches in lockstep (measured: no overlap at all with two in flight, profiles/r4_in_flight.txt)
            caller.wait_event(slot["consumed"])
        self.h.set_stream(caller.cuda_stream)
        first = 0
        if ops and ops[0].kind == "pack":                      # the only reader of `images`: in the caller's stream order
            self._run_op(ops[0], images)
            first = 1
        else:
            images = images.clone()                          # (paths without the packer: a private copy, made in the caller's order)
        slot["fed"].record(caller)
        st = slot["stream"]
        st.wait_event(slot["fed"])
        # (Staggering the batches by stage - a batch's backbone behind the previous batch's backbone, its towers behind the previous
        # towers - was measured too and is WORSE than letting the slots' streams drift: 4.27 against 3.55 ms with three in flight.)
        with torch.cuda.stream(st):
            self.h.set_stream(st.cuda_stream)
            if self.trace_in_flight is not None:             # tools/exp_in_flight_engine.py: (slot, start, end) timing events per batch
                t_ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                t_ev[0].record(st)
            for i in range(first, len(ops)):
                self._run_op(ops[i], images)
                if i == first:
                    slot["consumed"] = torch.cuda.Event()
                    slot["consumed"].record(st)
            if first == 0:
                images.record_stream(st)                     # the private copy is read on the slot's stream
            boxes = plan["boxes"].view(-1)[:B * md * 4].view(B, md, 4)
            scores = plan["scores"].view(-1)[:B * md].view(B, md)
            labels = plan["labels"].view(-1)[:B * md].view(B, md)
            self.postprocess(plan["cfg"], plan["regression"], plan["classification"], H, W, boxes, scores, labels, plan["det_ws"],
                             score_threshold, nms_threshold, md, flags)
            if loss is not None:
                self.loss_from_boxes(plan, loss)             # its inputs were uploaded in the caller's order, before `fed`
            slot["done"] = torch.cuda.Event()
            slot["done"].record(st)
            if self.trace_in_flight is not None:
                t_ev[1].record(st)
                self.trace_in_flight.append((si, t_ev[0], t_ev[1]))
        self.h.set_stream(caller.cuda_stream)
        return boxes, scores, labels

    def _concurrent_streams(self, n, beside=()):
        """n HIP streams whose kernels really run beside each other (and beside the streams in `beside`).  The runtime multiplexes HIP streams onto a few hardware queues
        (GPU_MAX_HW_QUEUES, 4 by default) and two streams that share one are served strictly in turn: batches "in flight" on such a
        pair do not overlap at all (measured: 4.28 against 3.60 ms per batch, and WHICH streams of torch's pool collide changes with
        the streams created before; profiles/r4_in_flight.txt).  So candidates are tested, once: a one-workgroup spin kernel
        (torch.cuda._sleep) on the candidate and on every stream already chosen must take the time of one, not of two."""
        sleep = getattr(torch.cuda, "_sleep", None)
        chosen = []
        if sleep is None or os.environ.get("RTN_STREAM_SELECT", "1") == "0":
            return [torch.cuda.Stream(device=self.device) for _ in range(n)]
        import time
        cycles = 400000

        def spin(streams):
            torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            for st_ in streams:
                with torch.cuda.stream(st_):
                    sleep(cycles)
            for st_ in streams:
                st_.synchronize()
            return time.perf_counter() - t0
        for _ in range(8 * n):
            if len(chosen) == n:
                break
            cand = torch.cuda.Stream(device=self.device)
            spin([cand])                                             # first use of a stream: not timed
            one = min(spin([cand]) for _ in range(2))
            if all(min(spin([cand, c]) for _ in range(2)) < 1.5 * one for c in list(beside) + chosen):
                chosen.append(cand)
        while len(chosen) < n:                                       # (no overlapping set found: the batches still run, one queue at a time)
            chosen.append(torch.cuda.Stream(device=self.device))
        return chosen

    def wait_slot(self, si):
        """The HOST waits until the batch most recently given to buffer set `si` is done (its outputs may then be copied out)."""
        if 0 <= si < len(self._slots) and self._slots[si]["done"] is not None:
            self._slots[si]["done"].synchronize()

    def slot_stream(self, si):
        """The HIP stream buffer set `si` runs its batches on (in_flight > 1): work enqueued there after detect() sees that batch's
        outputs, and the set's next batch is ordered after it (model/eval.py DeviceEvaluator.add)."""
        return self._slots[si]["stream"]

    def join(self):
        """The caller's current stream waits for every batch detect() has in flight (in_flight > 1)."""
        cur = torch.cuda.current_stream(self.device)
        for slot in self._slots:
            if slot["done"] is not None:
                cur.wait_event(slot["done"])

    def postprocess(self, cfg, regression, classification, H, W, boxes, scores, labels, ws, score_threshold=0.05,
                    nms_threshold=0.5, max_detections=300, flags=0):
        """flags: detect_flags(nms, class_specific_filter); every mode fits the plan's workspace (rtn_detect_workspace_bytes)."""
        self._bind_stream()
        B = regression.shape[0]
        args = (self.h.raw, C.byref(cfg), B, classification.shape[2], regression.data_ptr(), classification.data_ptr(), H, W, score_threshold,
                nms_threshold, max_detections, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), ws.data_ptr(), ws.numel())
        self.h.check(L.lib.rtn_decode_filter_nms(*args) if flags == 0 else L.lib.rtn_decode_filter_nms_ex(*args, flags, None))
