"""Plan ops as named records: one typing.NamedTuple per op kind of the forward list (engine.Engine._plan / _variant) and of the
backward list (trainer.Trainer._bplan).  Field 0 is the kind string and the field order IS the tuple layout that bench.py, tools/
and the tests read by position.  Next to its fields every record says what it reads and writes (io(): data pointers, null ones are
skipped by engine.schedule_lanes, which derives the cross-lane events from them), which lane it runs on (lane()) and how it is
launched (launch()).  A new op kind is one class here; nothing else lists the kinds."""
import ctypes as C
from typing import Any, NamedTuple, Optional

import torch

from . import _lib as L

SRC_DT = {torch.bfloat16: 0, torch.float32: 1, torch.uint8: 2}
MAIN, WEIGHT, CLS, EXTRA = "main", "weight", "cls", "extra"        # lane classes of the backward ops (Trainer._bschedule)


def _call(h, fn, *args):
    h.check(fn(h.raw, *args))


def _tensor_io(reads, writes):
    """io() of an op whose operands are tensor fields: the names of the fields it reads and of those it writes."""
    def io(op):
        return [getattr(op, f).data_ptr() for f in reads], [getattr(op, f).data_ptr() for f in writes]
    return io


def _meta_io(op):
    """Descriptor ops keep the tensors behind their descriptor in meta: xs and the epilogue's residual inputs are read, ys written."""
    m = op.meta
    return [t.data_ptr() for t in m["xs"]] + [t.data_ptr() for t in m.get("res", ()) if t is not None], [t.data_ptr() for t in m["ys"]]


def _launch_desc(fn):
    def launch(op, eng, images):
        _call(eng.h, fn, C.byref(op.desc))
    return launch


def _lane(v):
    """lane() of an op that always runs on lane (forward) / lane class (backward) v."""
    return lambda op, *_: v


def _conv_lane(op):
    """The graph is a chain except where the reference's model forks (model/defineModel.py:183-249): the projection shortcut of a
    stage's first block (branch1, beside branch2a/2b), the P6 -> P7 and P5 / P4 branches of the pyramid (beside the top-down C4/C3
    path) and the two head towers.  Those run on side lanes so that their launch latency and partly filled last rounds of
    workgroups overlap other work."""
    name = op.name
    if name.endswith("_branch1") or name in ("P6", "P7") or name.startswith("pyramid_classification"):
        return 1
    return 2 if name in ("P5", "P4") else 0


# ---------------------------------------------------------------------- forward: lane() -> lane, launch(engine, images)
class Pack(NamedTuple):
    kind: str; xp: Any; xin: dict
    io, lane = _tensor_io((), ("xp",)), _lane(0)
    def launch(self, eng, images):
        xi = self.xin
        _call(eng.h, L.lib.rtn_stem_pack, images.data_ptr(), SRC_DT[images.dtype], self.xp.data_ptr(), eng.rdt,
              xi["B"], xi["H"], xi["W"], xi["Hp"], xi["Wp"])


class Conv(NamedTuple):
    kind: str; desc: Any; name: str; meta: dict
    io, lane, launch = _meta_io, _conv_lane, _launch_desc(L.lib.rtn_conv2d_fwd)


class Bneck(NamedTuple):
    kind: str; desc: Any; name: str; meta: dict
    io, lane, launch = _meta_io, _lane(0), _launch_desc(L.lib.rtn_bottleneck64_fwd)


class Chain(NamedTuple):
    kind: str; desc: Any; name: str; meta: dict
    io, lane, launch = _meta_io, _lane(0), _launch_desc(L.lib.rtn_chain1x1_fwd)


class ConvQ(NamedTuple):
    """A conv whose epilogue writes e4m3 with the static scale `scale`."""
    kind: str; desc: Any; name: str; meta: dict; scale: float
    io, lane = _meta_io, _conv_lane
    def launch(self, eng, images):
        _call(eng.h, L.lib.rtn_conv2d_fwd_fp8out, C.byref(self.desc), self.scale)


class Conv8(NamedTuple):
    """An fp8 conv; q: its ConvFp8 scales."""
    kind: str; desc: Any; name: str; meta: dict; q: Any
    io, lane = _meta_io, _conv_lane
    def launch(self, eng, images):
        _call(eng.h, L.lib.rtn_conv2d_fp8_fwd, C.byref(self.desc), C.byref(self.q))


class Dual(NamedTuple):
    """branch2c with the projection shortcut folded in; src2: the ConvSrc2 of the shortcut's input."""
    kind: str; desc: Any; name: str; src2: Any; meta: dict
    io, lane = _meta_io, _lane(0)
    def launch(self, eng, images):
        _call(eng.h, L.lib.rtn_conv1x1_dual_fwd, C.byref(self.desc), C.byref(self.src2))


class Quant(NamedTuple):
    kind: str; src: Any; dst: Any; scale: float
    io, lane = _tensor_io(("src",), ("dst",)), _lane(0)
    def launch(self, eng, images):
        _call(eng.h, L.lib.rtn_quantize_fp8, self.src.data_ptr(), eng.rdt, self.dst.data_ptr(), self.src.numel(), self.scale)


class Stem(NamedTuple):
    """conv1 + ReLU + pool1 as one kernel.  tail: None or (a_out, w2a, b2a) - res2a_branch2a applied to the pooled pixels before
    they leave the registers; pool_idx: the pool's winning taps, written by a training forward whose backward reads them."""
    kind: str; out: Any; bhw: tuple; w: Any; b: Any; xp: Any; padded_hw: tuple; tail: Optional[tuple]; pool_idx: Any
    lane = _lane(0)
    def io(self):
        return [self.xp.data_ptr()], [self.out.data_ptr(), self.pool_idx.data_ptr()] + ([self.tail[0].data_ptr()] if self.tail is not None else [])

    def launch(self, eng, images):
        taps = eng._taps()
        args = (self.xp.data_ptr(), *self.padded_hw, self.w.data_ptr(), self.w.shape[0], self.b.data_ptr(), self.out.data_ptr(), *self.bhw)
        if self.tail is None and not taps:
            return _call(eng.h, L.lib.rtn_stem_conv_pool, *args)
        a_out, w2a, b2a = [t.data_ptr() for t in self.tail] if self.tail is not None else (None, None, None)
        _call(eng.h, L.lib.rtn_stem_conv_pool_branch2a, *args, w2a, b2a, a_out, self.pool_idx.data_ptr() if taps else None)


class Pool(NamedTuple):
    kind: str; src: Any; dst: Any; bhwc: tuple; idx: Any
    io, lane = _tensor_io(("src",), ("dst", "idx")), _lane(0)
    def launch(self, eng, images):
        if eng._taps():
            _call(eng.h, L.lib.rtn_maxpool3x3s2_tfsame_fwd_idx, self.src.data_ptr(), self.dst.data_ptr(), self.idx.data_ptr(), eng.rdt, *self.bhwc)
        else:
            _call(eng.h, L.lib.rtn_maxpool3x3s2_tfsame_fwd, self.src.data_ptr(), self.dst.data_ptr(), eng.rdt, *self.bhwc)


class Relu(NamedTuple):
    kind: str; src: Any; dst: Any
    io, lane = _tensor_io(("src",), ("dst",)), _lane(1)          # lane 1: between P6 and P7
    def launch(self, eng, images):
        _call(eng.h, L.lib.rtn_relu, self.src.data_ptr(), self.dst.data_ptr(), eng.rdt, self.src.numel())


# ---------------------------------------------------------------------- backward: lane(dyp_cls) -> lane class, launch(trainer, bp, index, side)
class PadCast(NamedTuple):
    kind: str; src: Any; dst: Any; rows: int; cin: int; cout: int
    io = _tensor_io(("src",), ("dst",))
    def lane(self, dyp_cls):
        return CLS if self.dst is dyp_cls else MAIN

    def launch(self, tr, bp, i, side=None):
        _call(tr.eng.h, L.lib.rtn_pad_cast_rows, self.src.data_ptr(), self.dst.data_ptr(), tr.eng.rdt, self.rows, self.cin, self.cout)


class Wgrad(NamedTuple):
    """Weight gradient dW (and, fused, the bias gradient db over `cout` channels when the layer owns a bias) of layer `name`."""
    kind: str; desc: Any; dW: Any; name: str; db: Any; cout: int
    lane = _lane(WEIGHT)
    def io(self):
        d = self.desc
        reads = [p_ for i in range(d.ngroups) for p_ in (d.g[i].in_, d.g[i].out)]
        return reads, [self.dW.data_ptr()] + ([self.db.data_ptr()] if self.db is not None else [])

    def launch(self, tr, bp, i, side=None):
        """side: the side stream the op runs on; None: the launch stream (no lanes)."""
        h, lib, d = tr.eng.h, L.lib, C.byref(self.desc)
        tab = bp["rowinfo"].get(i)
        # every weight-gradient op owns its workspace (row-info table + the slabs of its ordered split reduction: 130 MB for a head
        # layer at batch 16 x 800 x 1333, 3.4 GB over the 107 layers), allocated at its first launch: ops on different lanes never
        # share scratch
        if tab is None:                               # the row-info table depends on the descriptor only: built once per layer
            tab = torch.empty(lib.rtn_conv2d_wgrad_workspace_bytes(d), dtype=torch.uint8, device=tr.eng.device)
            _call(h, lib.rtn_conv2d_wgrad_rowinfo, d, tab.data_ptr(), tab.numel())
            bp["rowinfo"][i] = tab
        bias = (self.db.data_ptr(), self.cout) if self.db is not None else (None, 0)
        _call(h, lib.rtn_conv2d_wgrad_prepared, d, self.dW.data_ptr(), *bias, tab.data_ptr(), tab.numel())
        if tr.record_impls:
            tr.impls[("wgrad", self.name)] = lib.rtn_debug_last_wgrad_impl(h.raw)
        if tr.bucketer is not None:                   # this layer's weight gradient is enqueued: its bucket may go out
            last_bias = i == bp["last_bias_bop"]      # the last fused bias gradient: the bias segments are complete too
            if last_bias and side is not None:        # they came from every weight-gradient lane: mark them on all
                for st in tr._wg_stream[:tr.wgrad_lanes]:
                    with torch.cuda.stream(st):
                        for bn_ in tr.bias_names:
                            tr.bucketer.mark(bn_)
            with torch.cuda.stream(side):             # the bucket's event must follow the kernels on THEIR stream (None: the current one)
                for dn in [self.name] + (tr.bias_names if last_bias else []):
                    tr.bucketer.layer_done(dn)


class Dgrad(NamedTuple):
    kind: str; desc: Any; name: str

    def io(self):
        d = self.desc
        gs = [d.g[i] for i in range(d.ngroups)]
        mask, res = d.flags & L.CONV_RELU_MASK, d.flags & (L.CONV_RES_SAME | L.CONV_RES_UPSAMPLE)      # what the epilogue reads
        return [p_ for g in gs for p_ in [g.in_] + ([g.mask] if mask else []) + ([g.res] if res else [])], [g.out for g in gs]

    def lane(self, dyp_cls):
        if self.name.startswith("pyramid_classification"):
            return CLS
        return EXTRA if self.name.endswith("_branch1") or self.name in ("P6", "P7", "P5", "P4") else MAIN

    def launch(self, tr, bp, i, side=None):
        _call(tr.eng.h, L.lib.rtn_conv2d_dgrad, C.byref(self.desc))
        if tr.record_impls:
            tr.impls[("dgrad", self.name)] = L.lib.rtn_debug_last_conv_impl(tr.eng.h.raw)


class Zins(NamedTuple):
    """Zero insertion of a stride-2 3x3 conv's dY; dims: (B, Ho, Wo, C, Hs, Ws)."""
    kind: str; src: Any; dst: Any; dims: tuple
    io, lane = _tensor_io(("src",), ("dst",)), _lane(MAIN)
    def launch(self, tr, bp, i, side=None):
        _call(tr.eng.h, L.lib.rtn_zero_insert2, self.src.data_ptr(), self.dst.data_ptr(), tr.eng.rdt, *self.dims)


class UpBwd(NamedTuple):
    """Backward of UpsampleLike + Add into dst; dims: (B, Hd, Wd, Hs, Ws, C); acc: dst already holds a contribution."""
    kind: str; dy: Any; dst: Any; dims: tuple; acc: int
    lane = _lane(MAIN)
    def io(self):
        return [self.dy.data_ptr()] + ([self.dst.data_ptr()] if self.acc else []), [self.dst.data_ptr()]      # accumulating: both

    def launch(self, tr, bp, i, side=None):
        _call(tr.eng.h, L.lib.rtn_upsample_add_bwd, self.dy.data_ptr(), self.dst.data_ptr(), tr.eng.rdt, *self.dims, self.acc)


class PoolBwd(NamedTuple):
    """Backward of pool1; dims: (B, Hi, Wi, C); y: the pooled tensor, the ReLU mask when the fused stem never wrote conv1's output x."""
    kind: str; x: Any; dy: Any; dx: Any; dims: tuple; idx: Any; y: Any
    io, lane = _tensor_io(("x", "dy", "idx", "y"), ("dx",)), _lane(MAIN)
    def launch(self, tr, bp, i, side=None):
        fused = tr.fwd_key[0] != 0
        _call(tr.eng.h, L.lib.rtn_maxpool3x3s2_tfsame_bwd_idx, self.dy.data_ptr(), self.idx.data_ptr(), (self.y if fused else self.x).data_ptr(),
              self.dx.data_ptr(), tr.eng.rdt, *self.dims, 2 if fused else 1)
