"""Host tests of the plan-op records (ops.py): every kind keeps the tuple layout that bench.py, the tools and the audit tests read by
position, and io() names the pointers each kind reads and writes - the input of the lane scheduler, where a miss is a silent
cross-stream race.  CPU tensors and empty descriptors stand in for device buffers, as in test_backward_schedule.py."""
import importlib

import pytest
import torch

O = importlib.import_module("retinanet-for-table-detection_amd.ops")
L = importlib.import_module("retinanet-for-table-detection_amd._lib")
E = importlib.import_module("retinanet-for-table-detection_amd.engine")
T = importlib.import_module("retinanet-for-table-detection_amd.trainer")


def tensors(n):
    return [torch.zeros(8) for _ in range(n)]


def ptrs(*ts):
    return [t.data_ptr() for t in ts]


def desc(ins, outs, flags=0, res=None, mask=None):
    d = L.ConvDesc()
    d.ngroups, d.flags = len(ins), flags
    for i, (a, o) in enumerate(zip(ins, outs)):
        g = L.ConvGroup()
        g.in_, g.out = a.data_ptr(), o.data_ptr()
        if res is not None:
            g.res = res[i].data_ptr()
        if mask is not None:
            g.mask = mask[i].data_ptr()
        d.g[i] = g
    return d


# ------------------------------------------------------------------ positions: (record class, kind, field names after `kind`)
LAYOUT = [
    (O.Pack, "pack", ("xp", "xin")),
    (O.Conv, "conv", ("desc", "name", "meta")),
    (O.Bneck, "bneck", ("desc", "name", "meta")),
    (O.Chain, "chain", ("desc", "name", "meta")),
    (O.ConvQ, "convq", ("desc", "name", "meta", "scale")),
    (O.Conv8, "conv8", ("desc", "name", "meta", "q")),
    (O.Dual, "dual", ("desc", "name", "src2", "meta")),
    (O.Quant, "quant", ("src", "dst", "scale")),
    (O.Stem, "stem", ("out", "bhw", "w", "b", "xp", "padded_hw", "tail", "pool_idx")),
    (O.Pool, "pool", ("src", "dst", "bhwc", "idx")),
    (O.Relu, "relu", ("src", "dst")),
    (O.PadCast, "padcast", ("src", "dst", "rows", "cin", "cout")),
    (O.Wgrad, "wgrad", ("desc", "dW", "name", "db", "cout")),
    (O.Dgrad, "dgrad", ("desc", "name")),
    (O.Zins, "zins", ("src", "dst", "dims")),
    (O.UpBwd, "upbwd", ("dy", "dst", "dims", "acc")),
    (O.PoolBwd, "poolbwd", ("x", "dy", "dx", "dims", "idx", "y")),
]


@pytest.mark.parametrize("cls,kind,fields", LAYOUT, ids=[k for _, k, _ in LAYOUT])
def test_record_keeps_the_tuple_layout(cls, kind, fields):
    values = [object() for _ in fields]
    op = cls(kind, *values)
    assert isinstance(op, tuple) and len(op) == 1 + len(fields)
    assert op[0] == kind and op.kind == kind
    assert cls._fields == ("kind",) + fields
    for i, (f, v) in enumerate(zip(fields, values)):
        assert op[1 + i] is v and getattr(op, f) is v, (kind, f)
    assert op._replace(**{fields[-1]: None})[len(fields)] is None


def test_every_record_class_is_in_the_layout_table():
    classes = {c for c in vars(O).values() if isinstance(c, type) and issubclass(c, tuple) and hasattr(c, "_fields")}
    assert classes == {cls for cls, _, _ in LAYOUT}
    for cls in classes:
        assert callable(cls.io) and callable(cls.lane) and callable(cls.launch), cls


# ------------------------------------------------------------------ io(): (pointers read, pointers written)
def test_forward_io():
    x, y, r, a, b, c, idx, w, bias = tensors(9)
    meta = {"xs": [x, a], "ys": [y, b], "res": [r, None]}
    for op in (O.Conv("conv", None, "P4", meta), O.ConvQ("convq", None, "C3_reduced", meta, 1.0), O.Conv8("conv8", None, "P3", meta, None)):
        assert op.io() == (ptrs(x, a, r), ptrs(y, b)), op.kind                 # + the residual inputs of the epilogue
    plain = {"xs": [x, a], "ys": [y, b]}
    for op in (O.Bneck("bneck", None, "n", plain), O.Chain("chain", None, "n", plain), O.Dual("dual", None, "n", None, plain)):
        assert op.io() == (ptrs(x, a), ptrs(y, b)), op.kind
    assert O.Pack("pack", x, {}).io() == ([], ptrs(x))
    assert O.Quant("quant", x, y, 1.0).io() == (ptrs(x), ptrs(y))
    assert O.Pool("pool", x, y, (1, 2, 2, 64), idx).io() == (ptrs(x), ptrs(y, idx))
    assert O.Relu("relu", x, y).io() == (ptrs(x), ptrs(y))
    stem = O.Stem("stem", y, (1, 4, 4), w, bias, x, (10, 10), None, idx)
    assert stem.io() == (ptrs(x), ptrs(y, idx))
    assert stem._replace(tail=(a, b, c)).io() == (ptrs(x), ptrs(y, idx, a))      # + res2a_branch2a's output
    for op in (stem, O.Relu("relu", x, y), O.Conv("conv", None, "P4", meta)):
        assert E.Engine._op_io(op) == op.io() and E.Engine._lane_of(op) == op.lane()


def test_backward_io():
    x, dy, dx, dw, db, r, m, idx, y = tensors(9)
    assert O.PadCast("padcast", x, dy, 1, 1, 1).io() == (ptrs(x), ptrs(dy))
    assert O.Zins("zins", dy, dx, (1, 1, 1, 1, 1, 1)).io() == (ptrs(dy), ptrs(dx))
    assert O.UpBwd("upbwd", dy, dx, (1,) * 6, 0).io() == (ptrs(dy), ptrs(dx))
    assert O.UpBwd("upbwd", dy, dx, (1,) * 6, 1).io() == (ptrs(dy, dx), ptrs(dx))      # an accumulating output is both
    assert O.PoolBwd("poolbwd", x, dy, dx, (1, 2, 2, 64), idx, y).io() == (ptrs(x, dy, idx, y), ptrs(dx))
    wd = desc([x, r], [dy, m])
    assert O.Wgrad("wgrad", wd, dw, "P3", None, 4).io() == (ptrs(x, dy, r, m), ptrs(dw))
    assert O.Wgrad("wgrad", wd, dw, "P3", db, 4).io() == (ptrs(x, dy, r, m), ptrs(dw, db))
    both = desc([dy], [dx], res=[r], mask=[m])                              # the flags decide what the epilogue reads
    assert O.Dgrad("dgrad", both, "P3").io() == (ptrs(dy), ptrs(dx))
    both.flags = L.CONV_RELU_MASK
    assert O.Dgrad("dgrad", both, "P3").io() == (ptrs(dy, m), ptrs(dx))
    both.flags = L.CONV_RES_SAME
    assert O.Dgrad("dgrad", both, "P3").io() == (ptrs(dy, r), ptrs(dx))
    both.flags = L.CONV_RELU_MASK | L.CONV_RES_SAME | L.CONV_MASK_PRE
    assert O.Dgrad("dgrad", both, "P3").io() == (ptrs(dy, m, r), ptrs(dx))
    two = desc([dy, x], [dx, y], flags=L.CONV_RES_UPSAMPLE, res=[r, m])
    op = O.Dgrad("dgrad", two, "P3")
    assert op.io() == (ptrs(dy, r, x, m), ptrs(dx, y))
    assert T.Trainer._bop_io(op) == op.io()


def test_lanes():
    x, y = tensors(2)
    lanes = {"res3a_branch1": 1, "P6": 1, "P7": 1, "P5": 2, "P4": 2, "pyramid_classification_2": 1, "pyramid_classification": 1,
             "pyramid_regression_2": 0, "res3a_branch2a": 0, "C4_reduced": 0, "P3": 0}
    for name, lane in lanes.items():
        for op in (O.Conv("conv", None, name, {}), O.ConvQ("convq", None, name, {}, 1.0), O.Conv8("conv8", None, name, {}, None)):
            assert op.lane() == lane, (op.kind, name)
    assert O.Relu("relu", x, y).lane() == 1
    for op in (O.Pack("pack", x, {}), O.Quant("quant", x, y, 1.0), O.Pool("pool", x, y, (), x), O.Bneck("bneck", None, "res2b_branch1", {}),
               O.Chain("chain", None, "P6", {}), O.Dual("dual", None, "P5", None, {}), O.Stem("stem", *[None] * 8)):
        assert op.lane() == 0, op.kind
    # backward: lane classes, which Trainer._bschedule turns into lanes
    assert O.Wgrad("wgrad", None, x, "P5", None, 4).lane(y) == O.WEIGHT
    assert O.PadCast("padcast", x, y, 1, 1, 1).lane(y) == O.CLS and O.PadCast("padcast", y, x, 1, 1, 1).lane(y) == O.MAIN
    classes = {"pyramid_classification_1": O.CLS, "pyramid_classification": O.CLS, "res4a_branch1": O.EXTRA, "P6": O.EXTRA, "P4": O.EXTRA,
               "pyramid_regression_1": O.MAIN, "res4a_branch2a": O.MAIN}
    for name, cls in classes.items():
        assert O.Dgrad("dgrad", None, name).lane(y) == cls, name
    for op in (O.Zins("zins", x, y, ()), O.UpBwd("upbwd", x, y, (), 0), O.PoolBwd("poolbwd", x, x, y, (), x, x)):
        assert op.lane(y) == O.MAIN, op.kind
