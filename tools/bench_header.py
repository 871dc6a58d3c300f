"""Measure header detection on 16 synthetic table crops of 300 x 500 (the recipe of tests/header_cases.py table():
a header band, shaded rows, 12 % dark and 2 % red pixels, Gaussian noise of sigma 2 / 6 / 15, one seed per crop).

  python tools/bench_header.py [--batch 16] [--iters 9] [--twin-crops 4] [--sklearn-crops 1]

Reports, medians over --iters after a warm-up iteration:
  (1) each device stage between stream events, buffers allocated beforehand (every entry is a copy of its tables, the wait for
      it and one launch): rtn_header_sample, rtn_header_cluster, rtn_header_stats, rtn_header_patches;
  (2) model.header.detect_headers for the batch, wall time from device crops to the dicts and device patches;
  (3) the CPU twins of the four stages on one thread over the first --twin-crops crops, per crop;
  (4) where sklearn is importable, the reference's ten KMeans fits (k = 1 .. 9, then the chosen k; its defaults, random_state=0)
      over the first --sklearn-crops crops' H,S,V points, per crop, with the threads sklearn finds.
For the kernels by themselves: rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -o header --
  python tools/bench_header.py --iters 3 --twin-crops 0 --sklearn-crops 0
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "retinanet-for-table-detection_amd"
HDR = importlib.import_module(PKG + ".model.header")
L = HDR.L
ROWS = 300


def table(seed, sigma, rows=ROWS):
    rng = np.random.default_rng(seed)
    img = np.full((rows, 500, 3), 255.0)
    img[0:24] = (200, 120, 40)
    for r0 in range(24, rows, 32):
        img[r0:r0 + 16] = (235, 235, 245)
    u = rng.random((rows, 500))
    img[u < 0.12] = (20, 20, 20)
    img[(u >= 0.12) & (u < 0.14)] = (30, 30, 200)
    img = img + rng.normal(0.0, sigma, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def wall_ms(fn, sync=True):
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stage_calls(be, plan, crops, bufs):
    """The four entries as closures over preallocated buffers (ks and the patch table from a first run)."""
    n, total = plan["n"], plan["total"]
    layout = [n, plan["dst"].ctypes.data, plan["offsets"].ctypes.data]
    ptrs = HDR._pointers(be, [crops[i] for i in plan["idx"]])
    p = lambda key: be.ptr(bufs[key])                                         # noqa: E731
    keep = bufs["tables"]
    return {
        "sample": lambda: be.call("rtn_header_sample", [n, ptrs, plan["heights"].ctypes.data, plan["widths"].ctypes.data, *layout[1:],
                                                        p("hsv"), 3 * total], HDR._workspace(n)),
        "cluster": lambda: be.call("rtn_header_cluster", [*layout, p("hsv"), 3 * total, 300, p("centres"), p("counts"), p("passes"),
                                                          p("fx"), p("labels"), 9 * total], HDR._workspace(n)),
        "stats": lambda: be.call("rtn_header_stats", [*layout, keep["ks"].ctypes.data, p("hsv"), 3 * total, p("labels"), 9 * total,
                                                      p("hist")], HDR._workspace(n)),
        "patches": lambda: be.call("rtn_header_patches", [*layout, p("hsv"), 3 * total, len(keep["pc"]), keep["pc"].ctypes.data,
                                                          keep["lo"].ctypes.data, keep["hi"].ctypes.data, keep["offs"].ctypes.data,
                                                          p("out"), int(keep["bytes"])], HDR._workspace(n, len(keep["pc"]))),
    }


def buffers(be, plan, results):
    n, total = plan["n"], plan["total"]
    pc, lo, hi = [], [], []
    for i, r in enumerate(results):
        for c in r["clusters"]:
            pc.append(i)
            lo.append(np.array(np.clip(c["Q1"], 0, 255), dtype=np.uint8))
            hi.append(np.array(np.clip(c["Q3"], 0, 255), dtype=np.uint8))
    pc = np.asarray(pc, np.int32)
    sizes = plan["points"][pc] * 3
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    tables = {"ks": np.asarray([r["k"] for r in results], np.int32), "pc": pc, "lo": np.ascontiguousarray(lo, np.uint8),
              "hi": np.ascontiguousarray(hi, np.uint8), "offs": offs[:-1].copy(), "bytes": offs[-1]}
    return {"hsv": be.empty(3 * total), "centres": be.empty(n * 243, np.float32), "counts": be.empty(n * 81, np.uint32),
            "passes": be.empty(n * 9, np.int32), "fx": be.empty(n * 9, np.uint64), "labels": be.empty(9 * total),
            "hist": be.empty(n * 6912, np.uint32), "out": be.empty(int(offs[-1])), "tables": tables}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--twin-crops", type=int, default=4)
    ap.add_argument("--sklearn-crops", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_header.py measures on the GPU: none found")
    n = a.batch
    host = [table(i, (2, 6, 15)[i % 3]) for i in range(n)]
    dev = [torch.from_numpy(c).cuda() for c in host]
    plan = HDR._plan([c.shape[:2] for c in host])
    results = HDR.detect_headers(dev)                                         # also the warm-up of every kernel
    torch.cuda.synchronize()
    be = HDR._pages.Device(dev[0].device)
    calls = stage_calls(be, plan, dev, buffers(be, plan, results))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    stage_ms = {k: [] for k in calls}
    whole_ms = []
    for it in range(a.iters + 1):
        for name, fn in calls.items():
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if it:
                stage_ms[name].append(ev[0].elapsed_time(ev[1]))
        ms, _ = wall_ms(lambda: HDR.detect_headers(dev))
        if it:
            whole_ms.append(ms)
    med = lambda v: float(np.median(v))                                       # noqa: E731
    total_pts = plan["total"]
    passes = sum(sum(r["passes"]) for r in results)
    print("batch: %d crops of %dx500x3: %d points, %d assignment passes over the nine fits of all crops (%.1f per crop), k picked: %s" %
          (n, ROWS, total_pts, passes, passes / n, sorted(r["k"] for r in results)))
    out = {"batch": n, "iters": a.iters}
    for name in calls:
        v = stage_ms[name]
        print("(1) rtn_header_%-8s %8.3f ms per batch (%.3f .. %.3f)" % (name, med(v), min(v), max(v)))
        out[name + "_ms"] = round(med(v), 3)
    slow = max(sum(r["passes"]) for r in results)
    print("    cluster: one workgroup per crop; the longest chain has %d passes, the batch %d: %.1f us per pass of %d points in that chain" %
          (slow, passes, med(stage_ms["cluster"]) * 1e3 / slow, ROWS * 500))
    print("(2) detect_headers: %.2f ms per batch (%.2f .. %.2f), %.0f crops/s" % (med(whole_ms), min(whole_ms), max(whole_ms),
                                                                               n / med(whole_ms) * 1e3))
    out["detect_headers_ms"] = round(med(whole_ms), 2)

    m = min(a.twin_crops, n)
    if m:
        torch.set_num_threads(1)
        sub = HDR._plan([c.shape[:2] for c in host[:m]])
        tw = HDR._pages.Twins()
        tcalls = stage_calls(tw, sub, host, buffers(tw, sub, results[:m]))
        twin_total = 0.0
        for name, fn in tcalls.items():
            ms = min(wall_ms(fn, sync=False)[0] for _ in range(2))
            twin_total += ms
            print("(3) rtn_header_%s_host, one thread: %.1f ms per crop" % (name, ms / m))
            out["twin_%s_ms_per_crop" % name] = round(ms / m, 2)
        dev_per_crop = sum(med(stage_ms[k]) for k in calls) / n
        print("    twins %.1f ms per crop against %.3f ms per crop on the device, in batches of %d (%.0fx)" %
              (twin_total / m, dev_per_crop, n, twin_total / m / dev_per_crop))
        out["twin_ms_per_crop"] = round(twin_total / m, 1)
    try:
        from sklearn.cluster import KMeans
    except ImportError:
        KMeans = None
    s = min(a.sklearn_crops, n)
    if KMeans is not None and s:
        hsv = HDR._sample(be, plan, dev).cpu().numpy()
        t = []
        for i in range(s):
            pts = hsv[3 * int(plan["offsets"][i]):3 * int(plan["offsets"][i] + plan["points"][i])].reshape(-1, 3)
            t0 = time.perf_counter()
            for k in list(range(1, 10)) + [results[i]["k"]]:
                KMeans(n_clusters=k, random_state=0, verbose=0).fit(pts)
            t.append((time.perf_counter() - t0) * 1e3)
        print("(4) the reference's ten KMeans fits (sklearn, %s threads): %.0f ms per crop" % (os.environ.get("OMP_NUM_THREADS", "all"), med(t)))
        out["sklearn_ms_per_crop"] = round(med(t), 0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
