"""The backward plan of a training step, derived from the forward op list of engine.Engine._plan (trainer.Trainer._bplan is the cached
entry point): the graph pass (analyse), the gradient slots (GradSlots), the layout of a layer's groups in its dY (dy_layout), the
descriptor builders (wgrad_desc, dgrad_group, dgrad_epilogue) and the loop that appends the backward ops of ops.py (Emit).  All but
Emit are pure host code over tensor identities, shapes and ctypes fields: tests/test_backward_plan.py runs them on CPU tensors."""
import ctypes as C
from typing import NamedTuple

import torch

from . import _lib as L
from . import ops as O
from .engine import Engine

ALIAS, BUF = "alias", "buf"           # GradSlots.state(): the tensor's gradient is another tensor's / is in its own buffer


class Graph(NamedTuple):
    relu_src: dict        # id(relu output) -> its source tensor (P6r -> P6)
    relu_out: set         # ids of the tensors whose producing conv applies a ReLU (the pool does not)
    need: set             # ids of the tensors that need a gradient
    tensors: dict         # id -> tensor, every tensor the ops read or write: keeps the ids above valid


def analyse(ops, is_trainable):
    """Graph pass over the forward op list.  The pruning rule: a tensor needs a gradient iff its producer is a trainable layer or any
    input of its producer needs one.  Every consumer of a tensor is pruned alike, so the first-writer / accumulate order of the
    backward ops that survive is the full backward's, minus whole tensors."""
    g = Graph({}, set(), set(), {})
    for op in ops:
        if op.kind == "conv":
            me = op.meta
            ins = list(me["xs"]) + [r for r in me["res"] if r is not None]
            g.tensors.update((id(t), t) for t in ins + list(me["ys"]))
            if me.get("relu"):
                g.relu_out.update(id(y) for y in me["ys"])
            if is_trainable(op.name) or any(id(t) in g.need for t in ins):
                g.need.update(id(y) for y in me["ys"])
        elif op.kind in ("pool", "relu"):
            g.tensors.update(((id(op.src), op.src), (id(op.dst), op.dst)))
            if op.kind == "relu":
                g.relu_src[id(op.dst)] = op.src
            if id(op.src) in g.need:
                g.need.add(id(op.dst))
    return g


class GradSlots:
    """The gradient of every forward tensor while the backward list is built.  A tensor starts unwritten (state None).  The identity
    shortcut of a residual add aliases it to the sum's gradient (ALIAS: no launch, and it must come first); every other contribution
    goes to the tensor's own zeroed buffer (BUF), the first one taking an alias along as its residual input."""

    def __init__(self, keep):
        self.keep, self.bufs, self.aliases, self.states = keep, {}, {}, {}

    def adopt(self, t, buf):
        """`buf` is t's gradient buffer, written from outside the op list (the loss backward): t itself stays unwritten."""
        self.bufs[id(t)] = buf
        self.keep.append(buf)

    def of(self, t):
        """The tensor that holds t's gradient: its own buffer, the aliased sum, or None."""
        return self.bufs.get(id(t), self.aliases.get(id(t)))

    def state(self, t):
        return self.states.get(id(t))

    def alias(self, t, dy, who):
        if self.state(t) is not None:
            raise RuntimeError("identity gradient must be the first contribution (%s)" % who)
        self.aliases[id(t)], self.states[id(t)] = dy, ALIAS

    def contribute(self, t):
        """(out, res) for one more contribution to t's gradient: out is t's buffer (zeros when new: scatter targets and never-touched
        pixels stay 0), res what the contribution adds to - None for the first writer, the alias, or out itself."""
        state = self.state(t)
        res = self.aliases.pop(id(t)) if state == ALIAS else self.bufs[id(t)] if state == BUF else None
        if id(t) not in self.bufs:
            self.adopt(t, torch.zeros_like(t))
        self.states[id(t)] = BUF
        return self.bufs[id(t)], res

    def grad_of(self):
        """id(forward tensor) -> the tensor that holds its gradient after the backward pass: its own buffer, or the aliased sum's for a
        tensor whose only consumer is a residual add."""
        return {**self.bufs, **self.aliases}


def dy_layout(d_f, crun, cells_total=None):
    """[(image stride, element offset)] of every group of forward descriptor d_f in the layer's dY of `crun` channels.  cells_total
    (head outputs): the groups are the pyramid levels, one behind the other in a dY of that many cells per image; otherwise every group
    has a dY of its own."""
    out, cell_off = [], 0
    for gi in range(d_f.ngroups):
        cells = d_f.g[gi].Hout * d_f.g[gi].Wout
        out.append((cells * crun, 0) if cells_total is None else (cells_total * crun, cell_off * crun))
        cell_off += cells
    return out


def wgrad_desc(d_f, dys, crun, layout, rows=None):
    """Weight-gradient descriptor: the forward geometry with `out` re-pointed at dY.  rows: the rows of the layer's dW."""
    dw = L.ConvDesc()
    C.memmove(C.byref(dw), C.byref(d_f), C.sizeof(L.ConvDesc))
    dw.flags, dw.w, dw.bias = 0, None, None
    # dY is `crun` columns wide; the head outputs pad it to a power of two that can exceed dW's ceil128(cout) rows (270 -> 512 of 384):
    # the columns behind the last row of dW are padding, so the launch leaves them out
    dw.out_ld = crun
    dw.N = crun if rows is None else min(crun, rows)
    for gi, (dy, (img_stride, off)) in enumerate(zip(dys, layout)):
        g = dw.g[gi]
        g.out, g.out_elems = dy.data_ptr(), dy.numel()
        g.res, g.res_elems = None, 0
        g.out_img_stride, g.out_off = img_stride, off
    return dw


def dgrad_group(x, dy, Ho, Wo, kh, kw, stride, pad, crun, layout):
    """Input side of one data-gradient group, for forward input x and a forward output of Ho x Wo whose gradient is dy at `layout`
    (one entry of dy_layout): (group, (pad_t, pad_l), zins).  zins: None, or the op that fills the zero-inserted dY the group reads."""
    B, Hx, Wx = x.shape[:3]
    g, zins = L.ConvGroup(), None
    img_stride, off = layout
    if stride == 1:
        src, Hs, Ws, pads = dy, Ho, Wo, (kh - 1 - pad[0], kw - 1 - pad[1])
        g.Hout, g.Wout = Hx, Wx
    elif kh == 1:                                        # stride-2 1x1 'valid': scatter onto the stride grid
        src, Hs, Ws, pads = dy, Ho, Wo, (0, 0)
        g.Hout, g.Wout = Ho, Wo
        g.out_step, g.out_pix_w = stride, Wx
    else:                                                # stride-2 3x3: stride-1 conv over the zero-inserted dY
        Hs, Ws, pads = 2 * Ho - 1, 2 * Wo - 1, (kh - 1 - pad[0], kw - 1 - pad[1])
        src = torch.zeros(B, Hs, Ws, crun, dtype=dy.dtype, device=dy.device)
        zins = O.Zins("zins", dy, src, (B, Ho, Wo, crun, Hs, Ws))
        img_stride = Hs * Ws * crun
        g.Hout, g.Wout = Hx, Wx
    g.in_, g.in_elems = src.data_ptr() + off * src.element_size(), src.numel() - off
    g.in_img_stride, g.in_row_stride = img_stride, Ws * crun
    g.Hin, g.Win = Hs, Ws
    return g, pads, zins


def dgrad_epilogue(g, target, state, res, pre_mask, prod_relu):
    """Epilogue flags of a data-gradient group into `target`, with the group's res / mask fields.  state, res: GradSlots.state() before
    and the residual input from GradSlots.contribute().  pre_mask: the forward op read relu(target); prod_relu: target's producer
    applies a ReLU."""
    flags = 0
    if res is not None:
        flags |= L.CONV_RES_SAME
        g.res, g.res_elems, g.res_img_stride, g.res_ld = res.data_ptr(), res.numel(), res.numel() // res.shape[0], res.shape[-1]
    if pre_mask or prod_relu:
        flags |= L.CONV_RELU_MASK
        # an aliased identity gradient is not yet masked by this tensor's ReLU: mask the sum; otherwise mask this contribution alone
        # (the accumulated part was masked when it was written)
        if state != ALIAS:
            flags |= L.CONV_MASK_PRE
        g.mask, g.mask_elems, g.mask_img_stride, g.mask_ld = target.data_ptr(), target.numel(), target.numel() // target.shape[0], target.shape[-1]
    return flags


class Emit:
    """The backward op list of one forward plan under construction.  The order of the appends is the launch order: pad-casts; per conv
    (last to first) its wgrad, the residual ops, zins, dgrad; the pool backward."""

    def __init__(self, tr, plan, B):
        self.tr, self.eng, self.plan, self.B = tr, tr.eng, plan, B
        self.graph = analyse(plan["ops"], tr._is_trainable)
        self.keep, self.bops = [], []
        self.slots = GradSlots(self.keep)
        cfg = plan["cfg"]
        self.cells_total = sum(cfg.H[i] * cfg.W[i] for i in range(cfg.nlevels))

    def build(self):
        eng, plan, B, bops = self.eng, self.plan, self.B, self.bops
        d_reg, _ = self.loss_side(plan["regression"], Engine.TOWERS[0], 4)
        d_cls, dyp_cls = self.loss_side(plan["classification"], Engine.TOWERS[1], eng.K)
        for op in reversed(plan["ops"]):
            if op.kind == "conv":
                self.conv(op)
            elif op.kind == "pool" and id(op.src) in self.graph.need:
                dx, _ = self.slots.contribute(op.src)
                # op.dst: the pooled tensor (the fused stem's ReLU mask)
                bops.append(O.PoolBwd("poolbwd", op.src, self.slots.of(op.dst), dx, op.bhwc, op.idx, op.dst))
        loss_ws = torch.empty(L.lib.rtn_retina_loss_workspace_bytes(B * plan["N"]), dtype=torch.uint8, device=eng.device)
        bias_bops = [i for i, b in enumerate(bops) if b.kind == "wgrad" and b.db is not None]
        # what the pruned backward reads of the training forward's extra outputs: branch2b of the fused 64-channel blocks, the pool taps
        reads = set(p_ for b in bops for p_ in b.io()[0])
        keep_fwd = (any(blk.b2.data_ptr() in reads for blk in plan["fusion"]["blocks"] if blk.f == 64), any(b.kind == "poolbwd" for b in bops))
        grad_of = self.slots.grad_of()
        # grad_src keeps the forward tensors of grad_of alive, so its ids stay valid
        return {"bops": bops, "keep": self.keep, "last_bias_bop": bias_bops[-1] if bias_bops else -1, "keep_fwd": keep_fwd,
                "grad_of": grad_of, "grad_src": [self.graph.tensors[i] for i in grad_of], "d_reg": d_reg, "d_cls": d_cls,
                "dyp_cls": dyp_cls, "loss_ws": loss_ws, "plan": plan, "rowinfo": {}}

    def loss_side(self, out, name, width):
        """(d, dyp) of head output `out` with `width` values per anchor: the f32 gradient the loss backward writes and its cast, padded
        to the channel count the output conv's backward runs on, which is out's gradient slot."""
        eng, B, cells = self.eng, self.B, self.cells_total
        cp = self.tr._dy_channels(name)
        d = torch.zeros(B, self.plan["N"], width, dtype=torch.float32, device=eng.device)
        dyp = torch.zeros(B, cells, cp, dtype=eng.tdt, device=eng.device)
        self.keep.append(d)
        self.slots.adopt(out, dyp)
        if id(out) in self.graph.need:
            self.bops.append(O.PadCast("padcast", d, dyp, B * cells, eng.A * width, cp))
        return d, dyp

    def conv(self, op):
        tr, slots, need, bops = self.tr, self.slots, self.graph.need, self.bops
        d_f, name, me = op.desc, op.name, op.meta
        if id(me["ys"][0]) not in need:                  # frozen, and nothing below it trains
            return
        lo = self.eng.layout[name]
        crun = tr._dy_channels(name)
        dys = [slots.of(y) for y in me["ys"]]
        if any(dy is None for dy in dys):
            raise RuntimeError("no gradient reached the output of %s" % name)
        layout = dy_layout(d_f, crun, self.cells_total if name in Engine.TOWERS else None)
        if tr._is_trainable(name):
            dW, db = tr.grad_views(name)
            bops.append(O.Wgrad("wgrad", wgrad_desc(d_f, dys, crun, layout, dW.shape[0]), dW, name, db if lo["has_bias"] else None, lo["cout"]))     # bias gradient fused
        for r, dy in zip(me["res"], dys):                # residual inputs of the forward epilogue
            if r is None or id(r) not in need:
                continue
            if me["flags"] & L.CONV_RES_SAME:
                slots.alias(r, dy, name)
            else:                                        # UpsampleLike + Add
                dst, res = slots.contribute(r)
                bops.append(O.UpBwd("upbwd", dy, dst, (self.B, dy.shape[1], dy.shape[2], r.shape[1], r.shape[2], r.shape[3]), 1 if res is dst else 0))
        if not me.get("stem"):
            self.dgrad(op, dys, crun, layout)

    def dgrad(self, op, dys, crun, layout):
        """One grouped data-gradient launch into the inputs of `op` that need a gradient."""
        graph, slots, B = self.graph, self.slots, self.B
        d_f, name, me = op.desc, op.name, op.meta
        lo, wd = self.eng.layout[name], self.tr.wd[name]
        dd = L.ConvDesc()
        dd.batch, dd.dtype = B, self.eng.rdt
        dd.w, dd.bias, dd.w_rows, dd.N = wd.data_ptr(), None, wd.shape[0], lo["cin"]
        dd.KH, dd.KW, dd.Crun, dd.pix_stride = lo["kh"], lo["kw"], crun, crun
        dd.sy = dd.sx = 1
        dd.out_ld = lo["cin"]
        flags_all, ngd = None, 0
        for gi, x in enumerate(me["xs"]):
            pre_mask = id(x) in graph.relu_src           # x = relu(S): differentiate straight into S
            target = graph.relu_src.get(id(x), x)
            if id(target) not in graph.need:
                continue
            g, (dd.pad_t, dd.pad_l), zins = dgrad_group(x, dys[gi], d_f.g[gi].Hout, d_f.g[gi].Wout, lo["kh"], lo["kw"], me["stride"],
                                                        me["pad"], crun, layout[gi])
            if zins is not None:
                self.keep.append(zins.dst)
                self.bops.append(zins)
            state = slots.state(target)
            out, res = slots.contribute(target)
            g.out, g.out_elems, g.out_img_stride = out.data_ptr(), out.numel(), out.numel() // B
            flags = dgrad_epilogue(g, target, state, res, pre_mask, id(target) in graph.relu_out)
            if flags_all not in (None, flags):
                raise RuntimeError("grouped dgrad of %s needs uniform epilogue flags" % name)
            flags_all = flags
            dd.g[ngd] = g
            ngd += 1
        if ngd == 0:
            return
        dd.ngroups, dd.flags = ngd, flags_all
        L.attach_conv_workspace(self.eng.h, dd)          # caller-owned K-split slabs, one buffer per launch
        self.bops.append(O.Dgrad("dgrad", dd, name))
