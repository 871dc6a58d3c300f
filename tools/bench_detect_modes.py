"""Time the four FilterDetections modes of rtn_decode_filter_nms_ex (class-specific / class-agnostic x NMS / NMS-free) at batch 8,
800 x 1333 (200,700 anchors), K in {1, 3}, on two inputs:
  (a) sparse: ~2,000 candidates per image over all classes (the bench's regime: the trained table model at threshold 0.05);
  (b) all:    every anchor above the threshold in every class (an untrained head: the radix-select path).
Prints one line per (case, K, mode): us per call (CUDA events, mean of 20 after 3 warm-ups) and the detections kept in image 0.
Per-kernel times:  rocprofv3 --kernel-trace --stats -d rocprof_out -o detect_modes -- python3 tools/bench_detect_modes.py
               then python3 tools/bench_detect_modes.py --summarize rocprof_out/detect_modes_results.db
(the trace's dispatches, in launch order, are cut into the calls above: mean kernel time per call, last 20 calls of each line)."""
import ctypes as C
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

PKG = "retinanet-for-table-detection_amd"
L = importlib.import_module(PKG + "._lib")
E = importlib.import_module(PKG + ".engine")

MODES = [("class-specific nms", 0), ("class-agnostic nms", L.RTN_DET_CLASS_AGNOSTIC), ("class-specific no-nms", L.RTN_DET_NO_NMS),
         ("class-agnostic no-nms", L.RTN_DET_CLASS_AGNOSTIC | L.RTN_DET_NO_NMS)]


def inputs(case, B, N, K, rng):
    reg = (rng.standard_normal((B, N, 4), dtype=np.float32) * 0.5).astype(np.float32)
    if case == "all":
        cls = rng.uniform(0.06, 0.99, (B, N, K)).astype(np.float32)
    else:
        cls = rng.uniform(0.0, 0.05, (B, N, K)).astype(np.float32)
        hot = rng.uniform(size=(B, N, K)) < 2000.0 / (N * K)
        cls[hot] = rng.uniform(0.051, 0.99, int(hot.sum())).astype(np.float32)
    return reg, cls


CASES = [(case, K, name) for case in ("sparse", "all") for K in (1, 3) for name, _ in MODES]
WARM, REPS = 3, 20


def summarize(db):
    """Per (case, K, mode): mean us per call of every detect kernel (and of their sum) from a rocprofv3 kernel trace of main()."""
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    calls, cur = [], None
    for i, (name, t0, t1) in enumerate(rows):
        short = name.replace("(anonymous namespace)::", "").split("(")[0]
        if short.startswith("detect_candidates"):
            cur = {}
            if i > 0 and rows[i - 1][0].startswith("__amd_rocclr_fill"):       # the counts memset of this call
                cur["memset"] = (rows[i - 1][2] - rows[i - 1][1]) / 1e3
            calls.append(cur)
        if cur is not None and any(short.startswith(k) for k in ("detect_candidates", "nms_", "merge_topk")):
            cur[short] = cur.get(short, 0.0) + (t1 - t0) / 1e3
    per = WARM + REPS
    assert len(calls) == per * len(CASES), "%d calls in the trace, expected %d" % (len(calls), per * len(CASES))
    for j, (case, K, name) in enumerate(CASES):
        sel = calls[j * per + WARM:(j + 1) * per]
        names = list(sel[0])
        parts = ["%s %.1f" % (n, np.mean([c[n] for c in sel])) for n in names]
        total = np.mean([sum(c.values()) for c in sel])
        print("%-6s K %d  %-22s kernels %7.1f us  = %s" % (case, K, name, total, " + ".join(parts)))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--summarize":
        return summarize(sys.argv[2])
    dev = torch.device("cuda", 0)
    h = L.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    B, canvas = 8, (800, 1333)
    cfg, N = E.make_anchor_cfg(canvas)
    rng = np.random.default_rng(0)
    ob = torch.empty(B, 300, 4, device=dev)
    os_ = torch.empty(B, 300, device=dev)
    ol = torch.empty(B, 300, dtype=torch.int32, device=dev)
    print("B %d  canvas %dx%d  N %d" % (B, canvas[0], canvas[1], N))
    for case in ("sparse", "all"):
        for K in (1, 3):
            reg, cls = inputs(case, B, N, K, rng)
            tr, tc = torch.from_numpy(reg).to(dev), torch.from_numpy(cls).to(dev)
            ncand = int((cls[0] > np.float32(0.05)).sum())
            ws_bytes = L.lib.rtn_detect_workspace_bytes(B, N, K)            # what an engine plan holds: every mode fits it
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            for name, flags in MODES:
                def run():
                    h.check(L.lib.rtn_decode_filter_nms_ex(h.raw, C.byref(cfg), B, K, tr.data_ptr(), tc.data_ptr(), canvas[0], canvas[1],
                                                           C.c_float(0.05), C.c_float(0.5), 300, ob.data_ptr(), os_.data_ptr(),
                                                           ol.data_ptr(), ws.data_ptr(), ws_bytes, flags, None))
                for _ in range(WARM):
                    run()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                reps = REPS
                e0.record()
                for _ in range(reps):
                    run()
                e1.record()
                torch.cuda.synchronize()
                kept = int((ol[0] >= 0).sum())
                print("%-6s K %d  cand/img %6d  %-22s kept %3d  %8.1f us" % (case, K, ncand, name, kept, e0.elapsed_time(e1) / reps * 1e3),
                      flush=True)


if __name__ == "__main__":
    main()
