"""Measure the output step of test(): 16 sample-sized pages (2200x1712x3, synthetic: a light page with dark runs
of "text"), 3 kept boxes each, written under .jpg names: 3 crops and the annotated page per page, 64 files a batch.

  python tools/bench_render.py [--batch 16] [--iters 7]

Reports, the two paths alternating inside every iteration, medians over --iters after a warm-up iteration:
  (1) rtn_render_pages alone between device events, buffers allocated beforehand: the copy of the tables, the wait for it and the
      one render_kernel launch; and the GB/s over the algorithmic bytes (every output byte read once and written once).
  (2) model.utils.render_detections_device for the batch: wall time from device pages and host detections to 64 files on disk
      (kept lists, captions rasterised by Pillow, tables, kernel, the device JPEG encoder at q95 4:2:0, file writes).
  (3) the host path on the same inputs: a loop of the unchanged model.utils.render_detections on one thread (NumPy pages, Pillow
      at its default q75), the pages already in host memory.
For the kernel by itself: rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -o render --
  python tools/bench_render.py --iters 3
"""
import argparse
import importlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "retinanet-for-table-detection_amd"
L = importlib.import_module(PKG + "._lib")
U = importlib.import_module(PKG + ".model.utils")
H, W = 2200, 1712
SCALE = 1333.0 / 2200.0
TABLES = ((150, 200, 1550, 800), (150, 900, 1550, 1500), (300, 1600, 1400, 2100))
SCORES = (0.98, 0.91, 0.77)


def make_page(seed):
    rng = np.random.default_rng(seed)
    page = np.full((H, W, 3), 245, np.uint8)
    for y in range(120, H - 120, 36):                       # lines of "words": dark runs of random length
        x = 140
        while x < W - 200:
            n = int(rng.integers(20, 140))
            page[y:y + 14, x:x + n] = rng.integers(0, 90, (14, n, 1), dtype=np.uint8)
            x += n + int(rng.integers(12, 40))
    return page


def detections(n):
    boxes = np.full((n, 300, 4), -1, np.float32)
    scores = np.full((n, 300), -1, np.float32)
    labels = np.full((n, 300), -1, np.int32)
    for k, (t, s) in enumerate(zip(TABLES, SCORES)):
        boxes[:, k] = np.asarray(t, np.float32) * np.float32(SCALE)
        scores[:, k], labels[:, k] = s, 0
    scores[:, 3] = 0.12
    return boxes, scores, labels


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=7)
    a = ap.parse_args()
    n = a.batch
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py measures on the GPU: none found")
    host_pages = [make_page(i) for i in range(n)]
    dev_pages = [torch.from_numpy(p).cuda() for p in host_pages]
    boxes, scores, labels = detections(n)
    names = ["page_%02d.jpg" % i for i in range(n)]
    tmp = tempfile.mkdtemp(prefix="bench_render_")
    dev_dir, host_dir = os.path.join(tmp, "device"), os.path.join(tmp, "host")

    # (1) the launch alone
    kept = [U._kept_detections(boxes[i:i + 1], scores[i:i + 1], labels[i:i + 1], SCALE, 0.6)[0] for i in range(n)]
    plan = U._render_plan([(H, W)] * n, kept)
    out = torch.empty(plan["out_bytes"], dtype=torch.uint8, device="cuda")
    masks = torch.from_numpy(plan["masks"].copy()).cuda()
    wsb = int(L.lib.rtn_render_workspace_bytes(n, len(plan["boxes"]), len(plan["images"])))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    args = U._render_args(plan, [p.data_ptr() for p in dev_pages], masks.data_ptr(), out.data_ptr())
    h = U._rt.handle()

    def launch():
        h.check(L.lib.rtn_render_pages(h.raw, *args, ws.data_ptr(), wsb))
    out_px = sum(hh * ww for _p, _k, hh, ww, _o in plan["images"])
    alg_bytes = 2 * 3 * out_px

    def device_path():
        U.render_detections_device(dev_pages, boxes, scores, labels, [SCALE] * n, dev_dir, names)

    def host_path(pages):
        for i in range(n):
            U.render_detections(None, pages[i], boxes[i:i + 1], scores[i:i + 1], labels[i:i + 1], SCALE, host_dir, names[i])

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    k_ms, d_ms, h_ms = [], [], []
    for it in range(a.iters + 1):                           # iteration 0 warms every path up
        ev[0].record()
        launch()
        ev[1].record()
        torch.cuda.synchronize()
        k = ev[0].elapsed_time(ev[1])
        d = wall_ms(device_path)
        fresh = [p.copy() for p in host_pages]              # render_detections draws in place
        hh = wall_ms(lambda: host_path(fresh))
        if it:
            k_ms.append(k); d_ms.append(d); h_ms.append(hh)

    # the two paths made the same pictures: the device's files are Pillow's q95 4:2:0 of the host path's arrays
    crops, annotated = [], host_pages[0].copy()
    for b, s, l in kept[0]:
        U.draw_box(annotated, b, color=None)
        crops.append(U.extract_box(annotated, b).copy())
        U.draw_caption(annotated, b, "table {:.3f}".format(s))
    for rel, img in [("detections_inImage/page_00.jpg", annotated)] + [("detections_cropped/page_00_%d.jpg" % k, c) for k, c in enumerate(crops)]:
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(b, "JPEG", quality=95, subsampling=2)
        assert open(os.path.join(dev_dir, rel), "rb").read() == b.getvalue(), rel
    files = sum(len(os.listdir(os.path.join(dev_dir, d))) for d in ("detections_cropped", "detections_inImage"))
    assert files == 4 * n == sum(len(os.listdir(os.path.join(host_dir, d))) for d in ("detections_cropped", "detections_inImage"))

    med = lambda v: float(np.median(v))                                   # noqa: E731
    spread = lambda v: "%.1f .. %.1f" % (min(v), max(v))                  # noqa: E731
    kern, dv, ho = med(k_ms), med(d_ms), med(h_ms)
    print("batch: %d pages of %dx%dx3, 3 kept boxes each: %d output images, %.1f MB of output, %d files" %
          (n, H, W, len(plan["images"]), 3 * out_px / 1e6, files))
    print("(1) rtn_render_pages (table copy + render_kernel): %.3f ms per batch, %.0f GB/s over %.1f MB read + written" %
          (kern, alg_bytes / kern / 1e6, alg_bytes / 1e6))
    print("(2) render_detections_device: %.1f ms per batch (%s), %.1f pages/s" % (dv, spread(d_ms), n / dv * 1e3))
    print("(3) render_detections loop, one thread: %.1f ms per batch (%s), %.1f pages/s" % (ho, spread(h_ms), n / ho * 1e3))
    print("    (2) is %.1fx (3)" % (ho / dv))
    print(json.dumps({"batch": n, "iters": a.iters, "render_pages_ms": round(kern, 3), "render_pages_gb_s": round(alg_bytes / kern / 1e6, 1),
                      "device_ms": round(dv, 1), "device_pages_s": round(n / dv * 1e3, 1), "host_ms": round(ho, 1),
                      "host_pages_s": round(n / ho * 1e3, 2), "speedup": round(ho / dv, 2)}))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
