"""Measure scan analysis on 16 sample-sized pages: the 2200 x 1712 golden sample page repeated, resident on the device.

  python tools/bench_cca.py [--batch 16] [--iters 7] [--twin-pages 1] [--oracle-pages 1]

Reports, medians over --iters batches after a warm-up batch, between stream events around the whole call (launches, the waits
for the tables, the counts and boxes that come to the host between the stages, and the host arithmetic):
  (1) model.components.analyse_scan for the batch, and its two halves by themselves: remove_graphical_lines and
      component_heights on the cleaned pages;
  (2) the CPU twins (analyse_scan(device=False)) on one thread over the first --twin-pages pages, per page;
  (3) the NumPy / scipy oracle (tests/cca_ref.py analyse) on one thread over the first --oracle-pages pages, per page.
The last line is one JSON object with the same figures.
For the kernels by themselves: rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -o cca --
  python tools/bench_cca.py --iters 3 --twin-pages 0 --oracle-pages 0
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "retinanet-for-table-detection_amd"
CCA = importlib.import_module(PKG + ".model.components")


def sample_page():
    from PIL import Image
    with Image.open(os.path.join(ROOT, "tests", "golden", "sample_0717_023_orig.jpg")) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def event_ms(fn, iters):
    """fn() once to warm up, then `iters` times between two stream events each -> (the times in ms, the last result)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--twin-pages", type=int, default=1)
    ap.add_argument("--oracle-pages", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cca.py measures on the GPU: none found")
    page = sample_page()
    n = a.batch
    dev = [torch.from_numpy(page.copy()).cuda() for _ in range(n)]
    med = lambda v: float(np.median(v))                                       # noqa: E731
    out = {"batch": n, "iters": a.iters, "page": list(page.shape)}

    whole, res = event_ms(lambda: CCA.analyse_scan(dev), a.iters)
    lines, (cleaned, _boxes) = event_ms(lambda: CCA.remove_graphical_lines(dev), a.iters)
    text, _h = event_ms(lambda: CCA.component_heights(cleaned), a.iters)
    print("batch: %d pages of %dx%dx3; page 0: %d line boxes, %d kept text components, mode bin %d..%d" %
          (n, page.shape[0], page.shape[1], len(res[0]["line_boxes"]), len(res[0]["heights"]), *res[0]["mode_bin"]))
    for name, v in (("analyse_scan", whole), ("remove_graphical_lines", lines), ("component_heights", text)):
        print("(1) %-24s %8.2f ms per batch (%.2f .. %.2f), %.0f pages/s" % (name, med(v), min(v), max(v), n / med(v) * 1e3))
        out[name + "_ms"] = round(med(v), 2)
    out["device_pages_per_s"] = round(n / med(whole) * 1e3, 1)

    torch.set_num_threads(1)
    m = min(a.twin_pages, n)
    if m:
        t = []
        for _ in range(2):
            t0 = time.perf_counter()
            tw = CCA.analyse_scan([page] * m, device=False)
            t.append((time.perf_counter() - t0) / m)
        same = all(np.array_equal(tw[0][k], res[0][k].cpu().numpy() if hasattr(res[0][k], "cpu") else res[0][k])
                   for k in ("line_boxes", "cleaned", "heights", "histogram"))
        print("(2) the CPU twins, one thread: %.0f ms per page, %.2f pages/s (device: %.0fx); results equal the device's: %s" %
              (min(t) * 1e3, 1 / min(t), n / med(whole) * 1e3 * min(t), same))
        out["twin_ms_per_page"] = round(min(t) * 1e3, 1)
        out["equal"] = bool(same)
    m = min(a.oracle_pages, n)
    if m:
        import cca_ref as R
        t0 = time.perf_counter()
        for _ in range(m):
            R.analyse(page)
        t = (time.perf_counter() - t0) / m
        print("(3) the NumPy / scipy oracle, one thread: %.0f ms per page, %.2f pages/s (device: %.0fx)" %
              (t * 1e3, 1 / t, n / med(whole) * 1e3 * t))
        out["oracle_ms_per_page"] = round(t * 1e3, 0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
