"""Measure the skew estimator and the deskewing rotation on 16 pages of 2552 x 3303 x 3 (a 72-dpi scan enlarged by 4.17)
and 16 gray pages of 1712 x 2200 (the sample page's size), each page skewed by its own angle.

  python tools/bench_skew.py [--batch 16] [--iters 20] [--cpu-pages 1] > profiles/skew_bench.txt

The parent process never opens the GPU: it starts every step as a child under `timeout -k` and stops at the first one that fails.
  (1) device   rtn_skew_estimate for the batch between stream events (pages resident, 3 warm-up calls): with Otsu and with a fixed
               threshold at the default sweep (101 angles, band 32), and both with a single angle.  Otsu less fixed is the histogram
               pass with the threshold kernel; fixed / 1 angle is the count pass with one sweep workgroup per page, whose latency does
               not shrink with the angles.  Each gives a lower bound of its pixel pass's GB/s against the algorithmic bytes (each pass
               reads every page once), as a share of 6.3 TB/s; the exact split is a rocprofv3 --kernel-trace --stats run of
               `--step device` (profiles/skew_kernel_stats.csv).  The events enclose the call's upload of its page table and the host's
               wait for it.  Then estimate_skew (with its read-back) and deskew_images, wall clock, and page 0 against the CPU twin.
  (2) cpu      on one thread, per page: the CPU twin (rtn_skew_estimate_host), Otsu and fixed.
The last line is one JSON object with the same figures.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "retinanet-for-table-detection_amd"
HBM_BYTES_PER_S = 6.3e12
DETECT_BATCH_MS = (3.3, 3.5)                                                    # one detection batch, README
WORKLOADS = (("enlarged 72 dpi", 2552, 3303, 3), ("sample size", 1712, 2200, 1))   # name, width, height, channels
FIXED = 128


def make_page(np, w, h, c, seed):
    """A scan-like page whose lines run at an angle of its own (-2 .. 2 degrees): paper with noise, lines of dark word-sized blobs."""
    rng = np.random.RandomState(seed)
    page = np.clip(235 + rng.normal(0, 4, (h, w)), 0, 255).astype(np.uint8)
    slope = np.tan(np.radians(rng.uniform(-2.0, 2.0)))
    cols = np.arange(w)
    for y in range(h // 12, h - h // 12, max(h // 60, 6)):
        x = w // 10
        while x < w - w // 10:
            n = rng.randint(w // 60 + 1, w // 12 + 2)
            xs = cols[x:min(x + n, w - w // 10)]
            ys = y + np.rint((xs - w // 2) * slope).astype(np.int64)
            for k in range(max(h // 160, 2)):
                page[np.clip(ys + k, 0, h - 1), xs] = rng.randint(20, 90)
            x += n + rng.randint(3, w // 40 + 4)
    return np.ascontiguousarray(np.repeat(page[..., None], 3, axis=2)) if c == 3 else page


def stats(np, v):
    return [round(float(np.median(v)), 3), round(float(min(v)), 3), round(float(max(v)), 3)]


def host_arrays(np, pages):
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    return i32([p.shape[0] for p in pages]), i32([p.shape[1] for p in pages]), i32([3 if p.ndim == 3 else 1 for p in pages])


# ---- the children -----------------------------------------------------------------------------------------------------------------------
def step_device(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    P = importlib.import_module(PKG + ".model.preprocess")
    rt = importlib.import_module(PKG + ".model._rt")
    L = rt.L
    if not torch.cuda.is_available():
        raise SystemExit("bench_skew.py measures on the GPU: none found")
    out = {}
    for name, w, h, c in WORKLOADS:
        pages = [make_page(np, w, h, c, 10 + i) for i in range(a.batch)]
        dev = [torch.as_tensor(p).cuda() for p in pages]
        hs, ws, ch = host_arrays(np, pages)
        hd = rt.handle()
        sp = (C.c_void_p * a.batch)(*[d.data_ptr() for d in dev])
        full, _n = P.skew_shears(5.0, 0.1)
        one = np.zeros(1, np.int32)
        res = torch.zeros(a.batch * (len(full) + 2), dtype=torch.int64, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = {}
        for label, shear, thr in (("otsu_101", full, 0), ("fixed_101", full, FIXED), ("otsu_1", one, 0), ("fixed_1", one, FIXED)):
            K = len(shear)
            wsb = int(L.lib.rtn_skew_workspace_bytes(a.batch, hs.ctypes.data, ws.ctypes.data, 32, K))
            work = torch.empty(wsb, dtype=torch.uint8, device="cuda")
            base = res.data_ptr()
            ptrs = (base + 8 * a.batch * K + 8 * a.batch, base + 8 * a.batch * K, base + 8 * a.batch * K + 12 * a.batch, base)
            ms = []
            for i in range(a.iters + 3):
                ev[0].record()
                hd.check(L.lib.rtn_skew_estimate(hd.raw, a.batch, sp, hs.ctypes.data, ws.ctypes.data, ch.ctypes.data, thr, 32, K, shear.ctypes.data,
                                                 *ptrs, work.data_ptr(), wsb))
                ev[1].record()
                torch.cuda.synchronize()
                if i >= 3:
                    ms.append(ev[0].elapsed_time(ev[1]))
            times[label] = stats(np, ms)
        angles, details = P.estimate_skew(dev[:1], return_scores=True)
        K = len(full)
        t_thr, t_ink, t_best, t_sc = np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(K, np.uint64)
        assert L.lib.rtn_skew_estimate_host(1, (C.c_void_p * 1)(pages[0].ctypes.data), hs.ctypes.data, ws.ctypes.data, ch.ctypes.data, 0, 32, K,
                                            full.ctypes.data, t_thr.ctypes.data, t_ink.ctypes.data, t_best.ctypes.data, t_sc.ctypes.data) == 0
        d0 = details[0]
        equal = bool((d0["threshold"], d0["ink"], d0["best"]) == (int(t_thr[0]), int(t_ink[0]), int(t_best[0])) and np.array_equal(d0["scores"], t_sc))
        wall = {"estimate_skew": [], "deskew_images": []}
        for i in range(4):
            for key, fn in (("estimate_skew", P.estimate_skew), ("deskew_images", P.deskew_images)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fn(dev)
                torch.cuda.synchronize()
                wall[key].append(round((time.perf_counter() - t0) * 1e3, 3))
        all_angles = got[1]
        out[name] = {"page": [h, w, c], "times_ms": times, "pixel_bytes": sum(p.size for p in pages), "equal_twin": equal,
                     "wall_ms": wall, "angles": [round(v, 1) for v in all_angles], "rotated": sum(abs(v) >= 0.1 for v in all_angles)}
    print("DEVICE " + json.dumps(out))


def step_cpu(a):
    import numpy as np
    sys.path.insert(0, ROOT)
    try:
        import torch
        torch.set_num_threads(1)
    except ImportError:
        pass
    L = importlib.import_module(PKG)._lib
    P = importlib.import_module(PKG + ".model.preprocess")
    full, _n = P.skew_shears(5.0, 0.1)
    K = len(full)
    out = {}
    for name, w, h, c in WORKLOADS:
        res = {"otsu": [], "fixed": []}
        for i in range(a.cpu_pages):
            page = make_page(np, w, h, c, 10 + i)
            hs, ws, ch = host_arrays(np, [page])
            thr, ink, best, sc = np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(K, np.uint64)
            for key, t in (("otsu", 0), ("fixed", FIXED)):
                t0 = time.perf_counter()
                assert L.lib.rtn_skew_estimate_host(1, (C.c_void_p * 1)(page.ctypes.data), hs.ctypes.data, ws.ctypes.data, ch.ctypes.data, t, 32, K,
                                                    full.ctypes.data, thr.ctypes.data, ink.ctypes.data, best.ctypes.data, sc.ctypes.data) == 0
                res[key].append((time.perf_counter() - t0) * 1e3)
        out[name] = {k: round(float(np.median(v)), 1) for k, v in res.items()}
    print("CPU " + json.dumps(out))


# ---- the parent ---------------------------------------------------------------------------------------------------------------------
def child(limit_s, argv, a):
    cmd = ["timeout", "-k", "10", str(limit_s)] + argv + ["--batch", str(a.batch), "--iters", str(a.iters), "--cpu-pages", str(a.cpu_pages)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit("bench_skew.py: step failed with exit status %d, nothing more is started: %s" % (r.returncode, " ".join(cmd)))
    return r.stdout or ""


def tagged(text, tag):
    for line in text.splitlines():
        if line.startswith(tag + " "):
            return json.loads(line[len(tag) + 1:])
    raise SystemExit("bench_skew.py: no %s line in the step's output" % tag)


def report(batch, iters, dev, cpu):
    print("rtn_skew_estimate, %d pages per call, band 32, %d calls after 3 warm-up calls (stream events around the call, which enclose the upload of"
          " the page table and the host's wait for it):" % (batch, iters))
    for name, _w, _h, _c in WORKLOADS:
        v = dev[name]
        t = v["times_ms"]
        mb = v["pixel_bytes"] / 1e6
        rest_ms, hist_ms, grow_ms = t["fixed_1"][0], t["otsu_101"][0] - t["fixed_101"][0], t["fixed_101"][0] - t["fixed_1"][0]
        rate = lambda ms: v["pixel_bytes"] / (max(ms, 1e-6) * 1e-3)
        print("  %s, %dx%dx%d, %.1f MB of pixels:" % (name, v["page"][1], v["page"][0], v["page"][2], mb))
        for label, text in (("otsu_101", "Otsu, 101 angles"), ("fixed_101", "fixed threshold, 101 angles"), ("otsu_1", "Otsu, 1 angle"),
                            ("fixed_1", "fixed threshold, 1 angle")):
            print("    %-30s %.3f ms (%.3f .. %.3f)" % (text, t[label][0], t[label][1], t[label][2]))
        print("    Otsu less fixed, %.3f ms, is the histogram pass and the threshold kernel: the pass reads at %.0f GB/s or more, %.1f %% of 6.3 TB/s" %
              (hist_ms, rate(hist_ms) / 1e9, 100 * rate(hist_ms) / HBM_BYTES_PER_S))
        print("    fixed / 1 angle, %.3f ms, is the count pass, one sweep workgroup per page and the pick: the pass reads at %.0f GB/s or more, %.1f %%;"
              " 100 more angles add %.3f ms (per-kernel times: rocprofv3 --kernel-trace --stats)" %
              (rest_ms, rate(rest_ms) / 1e9, 100 * rate(rest_ms) / HBM_BYTES_PER_S, grow_ms))
        print("    against one detection batch of %.1f .. %.1f ms: Otsu %.2fx, fixed %.2fx" %
              (DETECT_BATCH_MS[0], DETECT_BATCH_MS[1], t["otsu_101"][0] / DETECT_BATCH_MS[0], t["fixed_101"][0] / DETECT_BATCH_MS[0]))
        print("    estimate_skew with its read-back, wall clock: %s ms; deskew_images (%d of %d pages rotated): %s ms; page 0 equals the CPU twin: %s" %
              (" / ".join("%.2f" % x for x in v["wall_ms"]["estimate_skew"]), v["rotated"], batch,
               " / ".join("%.2f" % x for x in v["wall_ms"]["deskew_images"]), v["equal_twin"]))
        if cpu:
            c = cpu[name]
            print("    one CPU thread, per page: twin %.1f ms with Otsu, %.1f ms fixed; the call is %.0fx the twin" %
                  (c["otsu"], c["fixed"], c["otsu"] * batch / t["otsu_101"][0]))
    print(json.dumps({"batch": batch, "iters": iters, "device": dev, "cpu": cpu}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-pages", type=int, default=1)
    ap.add_argument("--step", choices=("device", "cpu"))
    a = ap.parse_args()
    if a.step:
        return {"device": step_device, "cpu": step_cpu}[a.step](a)
    me = [sys.executable, os.path.abspath(__file__)]
    dev = tagged(child(600, me + ["--step", "device"], a), "DEVICE")
    cpu = tagged(child(900, me + ["--step", "cpu"], a), "CPU") if a.cpu_pages > 0 else {}
    report(a.batch, a.iters, dev, cpu)


if __name__ == "__main__":
    main()
