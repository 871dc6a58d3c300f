"""GPU: the conv launcher's dispatch, layer by layer, against a census recorded with the library of the commit BEFORE the launcher
was split into check / choose / fill / launch steps (csrc/rtn_conv.hip).  Which kernel a layer gets, on which tile, in which
work decomposition and with how much scratch is behaviour: a refactor of the launcher must not move any of it.

The census takes every conv descriptor (with its second source / fp8 scale block / fp8 output scale) the Engine builds - the plan's
per-layer ops and the ops of the fused variant forward() runs - and every data-gradient descriptor of the Trainer's backward plan, at
the benchmark's batch and canvas (8 x 800 x 1333 inference, 16 x 800 x 1333 training) and at 2 x 320 x 448, for bf16 inference, bf16
training, f32 inference, fp8 towers and fp8 towers + backbone.  Each descriptor is launched under the default environment and under
every knob setting of ENVS; the record of one launch is [return code, rtn_debug_last_conv_impl, rtn_debug_last_conv_tile,
rtn_debug_last_conv_streamk, the *_workspace_bytes answer].  The descriptors keep the workspace attach_conv_workspace gave them under
the default environment: where a knob asks for more, the launcher's own fallback is what gets recorded.  The three debug values are
read only after RTN_OK (a failed launch leaves its predecessor's in the handle) and recorded as -1 otherwise.

The fixture (tests/golden/conv_dispatch_census.json) depends on the CU count (tile choice, tail split, stream-K): it carries num_cus
and the test skips on a device that reports another.  `python tests/test_gpu_conv_dispatch.py` rewrites it from whatever library
RTN_LIB_PATH names; it is committed as the parent's library wrote it.  It holds every entry, packed without loss (pack / unpack): per
configuration the distinct records (`rows`), the distinct columns of row indices over ENVS (`patterns`) and each layer's column."""
import ctypes as C
import gc
import importlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_dispatch_census.json")
PKG = "retinanet-for-table-detection_amd"
pytestmark = pytest.mark.gpu

BENCH_CANVAS, BENCH_BATCH, BENCH_TRAIN_BATCH = (800, 1333), 8, 16          # bench.py: CANVAS, BATCH, TRAIN_BATCH
SMALL = (2, 320, 448)
MODES = ("bf16_inference", "bf16_training", "f32_inference", "fp8_towers", "fp8_towers_backbone")
ENVS = ([{}] + [{"RTN_CONV_IMPL": str(i)} for i in range(1, 7)] +
        [{"RTN_CONV_TAIL": "0"}, {"RTN_CONV_SPLITK": "0"}, {"RTN_CONV_G8_SK": "0"}, {"RTN_CONV_G8_SK": "1"}, {"RTN_CONV_H8": "0"},
         {"RTN_CONV_G8": "0"}, {"RTN_CONV_HN": "0"}])
KNOBS = sorted({k for e in ENVS for k in e})


def env_tag(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


def conv_ops(mode, B, H, W):
    """[(name, kind, descriptor, extra)] of one mode at one shape, and the objects that keep their buffers alive."""
    E, Wt, T = [importlib.import_module(PKG + "." + m) for m in ("engine", "weights", "trainer")]
    state = Wt.init_state("resnet50", 1, 9, seed=0, randomize_bn=True, cls_bias=-2.0, tame=True)
    eng = E.Engine("resnet50", 1, 9, dtype="f32" if mode == "f32_inference" else "bf16")
    eng.load_state(state)
    tr = None
    if mode.startswith("fp8"):
        g = torch.Generator().manual_seed(4)
        x = (torch.rand(B, H, W, 3, generator=g) * 2 - 1).to(torch.bfloat16).cuda()
        eng.calibrate_fp8(x, backbone=mode == "fp8_towers_backbone")
        del x
    if mode == "bf16_training":
        tr = T.Trainer(eng)
    plan = eng._plan(B, H, W)
    seen, out = set(), []
    for op in list(plan["ops"]) + list(eng.active_ops(plan)):
        if op[0] not in ("conv", "dual", "conv8", "convq") or id(op) in seen:
            continue
        seen.add(id(op))
        extra = op[3] if op[0] == "dual" else (op[4] if op[0] in ("conv8", "convq") else None)
        out.append((str(op[2]), op[0], op[1], extra))
    bp = None
    if tr is not None:
        bp = tr._bplan(B, H, W)
        out += [("dgrad:" + str(b[2]), "dgrad", b[1], None) for b in bp["bops"] if b[0] == "dgrad"]
    return out, (eng, tr, plan, bp)


def run_one(L, h, kind, d, extra):
    lib = L.lib
    if kind == "dual":
        ws = int(lib.rtn_conv1x1_dual_workspace_bytes(h.raw, C.byref(d), C.byref(extra)))
        rc = lib.rtn_conv1x1_dual_fwd(h.raw, C.byref(d), C.byref(extra))
    else:
        ws = int(lib.rtn_conv2d_workspace_bytes(h.raw, C.byref(d)))       # (an fp8 descriptor has no scratch: 0)
        if kind == "conv":
            rc = lib.rtn_conv2d_fwd(h.raw, C.byref(d))
        elif kind == "conv8":
            rc = lib.rtn_conv2d_fp8_fwd(h.raw, C.byref(d), C.byref(extra))
        elif kind == "convq":
            rc = lib.rtn_conv2d_fwd_fp8out(h.raw, C.byref(d), extra)
        else:
            rc = lib.rtn_conv2d_dgrad(h.raw, C.byref(d))
    if rc != 0:
        return [int(rc), -1, -1, -1, ws]
    return [0, int(lib.rtn_debug_last_conv_impl(h.raw)), int(lib.rtn_debug_last_conv_tile(h.raw)),
            int(lib.rtn_debug_last_conv_streamk(h.raw)), ws]


def census():
    L = importlib.import_module(PKG + "._lib")
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    configs = {}
    try:
        for mode in MODES:
            for B, H, W in ((BENCH_TRAIN_BATCH if mode == "bf16_training" else BENCH_BATCH,) + BENCH_CANVAS, SMALL):
                ops, alive = conv_ops(mode, B, H, W)
                eng = alive[0]
                eng._bind_stream()
                runs = {}
                for env in ENVS:
                    os.environ.update(env)
                    try:
                        runs[env_tag(env)] = [run_one(L, eng.h, kind, d, extra) for _, kind, d, extra in ops]
                    finally:
                        for k in env:
                            del os.environ[k]
                    torch.cuda.synchronize()
                configs["%s/%dx%dx%d" % (mode, B, H, W)] = {"layers": [n for n, _, _, _ in ops], "runs": runs}
                del ops, alive, eng
                gc.collect()
                torch.cuda.empty_cache()
    finally:
        os.environ.update(saved)
    return {"num_cus": torch.cuda.get_device_properties(0).multi_processor_count, "configs": configs}


def entries(c):
    return sum(len(rows) for cfg in c["configs"].values() for rows in cfg["runs"].values())


def pack(c):
    tags = [env_tag(e) for e in ENVS]
    out = {"num_cus": c["num_cus"], "entries": entries(c), "envs": tags, "layer_lists": [], "configs": {}}
    for key, cfg in c["configs"].items():
        if cfg["layers"] not in out["layer_lists"]:
            out["layer_lists"].append(cfg["layers"])
        rows = sorted({tuple(r) for t in tags for r in cfg["runs"][t]})
        cols = [tuple(rows.index(tuple(cfg["runs"][t][i])) for t in tags) for i in range(len(cfg["layers"]))]
        pats = sorted(set(cols))
        out["configs"][key] = {"layers": out["layer_lists"].index(cfg["layers"]), "rows": rows, "patterns": pats,
                               "layer_pattern": [pats.index(col) for col in cols]}
    return out


def unpack(f):
    configs = {}
    for key, cfg in f["configs"].items():
        cols = [cfg["patterns"][p] for p in cfg["layer_pattern"]]
        configs[key] = {"layers": f["layer_lists"][cfg["layers"]],
                        "runs": {t: [list(cfg["rows"][col[k]]) for col in cols] for k, t in enumerate(f["envs"])}}
    return {"num_cus": f["num_cus"], "configs": configs}


def test_conv_dispatch_matches_the_recorded_census(pkg):
    with open(FIXTURE) as f:
        packed = json.load(f)
    want = unpack(packed)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != want["num_cus"]:
        pytest.skip("the census was recorded on %d CUs, this device has %d" % (want["num_cus"], cus))
    got = census()
    assert sorted(got["configs"]) == sorted(want["configs"]) and len(want["configs"]) == 2 * len(MODES)
    bad, n = [], 0
    for key, w in want["configs"].items():
        g = got["configs"][key]
        assert g["layers"] == w["layers"], key
        assert sorted(g["runs"]) == sorted(w["runs"]) == sorted(env_tag(e) for e in ENVS), key
        for tag, rows in w["runs"].items():
            assert len(g["runs"][tag]) == len(rows) == len(w["layers"])
            for name, a, b in zip(w["layers"], g["runs"][tag], rows):
                n += 1
                if a != b:
                    bad.append("%s %s [%s]: got %s, recorded %s" % (key, name, tag, a, b))
    print("conv dispatch census: %d entries compared, %d differ" % (n, len(bad)))
    assert n == entries(want) == entries(got) == packed["entries"]
    assert not bad, "[rc, impl, tile, stream-K, workspace bytes] moved:\n" + "\n".join(bad[:40])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    c = census()
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    assert unpack(pack(c)) == c
    with open(path, "w") as f:                             # one line per top-level key and per configuration
        p = pack(c)
        f.write("{" + ",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in p.items() if k != "configs"))
        f.write(',\n"configs": {\n' + ",\n".join(' "%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in p["configs"].items()) + "\n}}\n")
    print("wrote %s: %d entries, num_cus %d, library %s" % (path, entries(c), c["num_cus"], importlib.import_module(PKG).LIB_PATH))
