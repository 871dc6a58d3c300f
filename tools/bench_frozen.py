"""Frozen-layer training against the full step: ResNet-50 RetinaNet, 800x1333, batch 16, bf16, one GPU.

Three configurations on ONE engine and trainer (same weights, same batch, same device-side anchor targets), each timed after its
own warm-up with the same step counts:  full (every layer trains), backbone frozen (conv1 .. res5c: the FPN and the heads train,
resnet_retinanet(modifier=freeze)), stem + res2 frozen.  A step is targets + forward + loss + backward + clipnorm Adam, as in
bench.py's training line.  Prints ms/step, img/s, the ratio to the full step and the library launches per step (forward ops,
loss, backward ops, optimizer; one launch may run more than one kernel - `rocprofv3 --kernel-trace --stats` counts those).

  python tools/bench_frozen.py [--steps 20] [--warmup 5] [--only full|backbone|stem_res2] [--json OUT]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

PKG = bench.PKG
E = importlib.import_module(PKG + ".engine")
Wt = importlib.import_module(PKG + ".weights")
T = importlib.import_module(PKG + ".trainer")
L = importlib.import_module(PKG + "._lib")

CONFIGS = {
    "full": lambda n: True,
    "backbone": lambda n: not (n == "conv1" or n.startswith("res")),
    "stem_res2": lambda n: not (n == "conv1" or n.startswith("res2")),
}


def optimizer_launches(tr):
    """Library calls of Trainer.optimizer_step: the norm, one Adam per part (weights / biases), the dgrad repack."""
    rt = tr._range_tables()
    if rt["all"][1] == 0:
        return 0
    return 1 + (rt["w"][1] > 0) + (rt["b"][1] > 0) + (1 if tr._pack_table is not None and tr._pack_table[1] else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=bench.TRAIN_BATCH)
    ap.add_argument("--only", choices=sorted(CONFIGS), action="append")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    B, (H, W) = args.batch, bench.CANVAS
    state = Wt.init_state("resnet50", 1, 9, seed=0, randomize_bn=True, cls_bias=-2.0, tame=True)
    eng = E.Engine("resnet50", 1, 9, dtype="bf16")
    eng.load_state(state)
    tr = T.Trainer(eng, lr=1e-4, clipnorm=0.001)
    x = bench.synth_images(torch, B, 2000, "cuda")
    cfg, N = E.make_anchor_cfg((H, W))
    rng = np.random.RandomState(100)
    gb, gc = np.zeros((B, 64, 4)), np.zeros(B, np.int32)
    for b in range(B):                                  # bench.py's boxes: 1-6 per page, w,h in [80,900]x[60,600]
        g = rng.randint(1, 7)
        w, h = rng.uniform(80, 900, g), rng.uniform(60, 600, g)
        x1, y1 = rng.uniform(0, W - w), rng.uniform(0, H - h)
        gb[b, :g] = np.stack([x1, y1, x1 + w, y1 + h], 1)
        gc[b] = g
    gbd, gld, gcd = torch.as_tensor(gb).cuda(), torch.zeros(B, 64, dtype=torch.int32, device="cuda"), torch.as_tensor(gc).cuda()
    hw = torch.as_tensor(np.tile(np.array((H, W), np.int32), (B, 1))).cuda()
    reg_t = torch.empty(B, N, 5, device="cuda")
    lab_t = torch.empty(B, N, 2, device="cuda")

    def step():
        eng._bind_stream()
        eng.h.check(L.lib.rtn_anchor_targets(eng.h.raw, C.byref(cfg), B, 1, gbd.data_ptr(), gld.data_ptr(), gcd.data_ptr(), hw.data_ptr(),
                                             0.4, 0.5, reg_t.data_ptr(), lab_t.data_ptr()))
        tr.forward_backward(x, reg_t, lab_t)
        tr.optimizer_step()

    rows = []
    for name in (args.only or ["full", "backbone", "stem_res2"]):
        live = CONFIGS[name]
        names = [n for n in eng.layout if live(n)]
        tr.set_trainable(None if len(names) == len(eng.layout) else names)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        bp = tr.bplans[(B, H, W)]
        kinds = {}
        for b in bp["bops"]:
            kinds[b[0]] = kinds.get(b[0], 0) + 1
        n_fwd = len(eng._variant(eng._plan(B, H, W), tr.fwd_key)["ops"])
        row = {"config": name, "trainable_layers": len(names), "ms_per_step": 1e3 * dt, "img_per_s": B / dt,
               "forward_key": list(tr.fwd_key), "launches": {"targets": 1, "forward": n_fwd, "loss": 2 if bp["bops"] else 1,
                                                             "gradient_reset": 1 if bp["bops"] else 0, "backward": len(bp["bops"]),
                                                             "optimizer": optimizer_launches(tr)},
               "backward_ops": kinds}
        row["launches_per_step"] = sum(row["launches"].values())
        rows.append(row)
        tr.set_trainable(None)                          # drops this configuration's backward plans before the next one
    full = next((r for r in rows if r["config"] == "full"), None)
    print("ResNet-50 RetinaNet training step, %dx%d, batch %d, bf16, %d warm-up + %d timed steps per configuration" %
          (H, W, B, args.warmup, args.steps))
    print("%-10s %8s %10s %9s %8s %9s  %s" % ("config", "layers", "ms/step", "img/s", "ratio", "launches", "backward ops"))
    for r in rows:
        ratio = r["ms_per_step"] / full["ms_per_step"] if full else float("nan")
        r["ratio_to_full"] = ratio
        print("%-10s %8d %10.2f %9.1f %8.3f %9d  %s" % (r["config"], r["trainable_layers"], r["ms_per_step"], r["img_per_s"], ratio,
                                                       r["launches_per_step"], r["backward_ops"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
