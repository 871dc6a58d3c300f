"""Measure table structure on 16 sample-sized pages with three boxes each: the 2200 x 1712 golden sample page
repeated, resident on the device, and the three fixed boxes of tests/lattice_cases.py.

  python tools/bench_lattice.py [--batch 16] [--iters 7] [--twin-pages 1] [--limit 300]

Every step runs in a process of its own under a time limit (--limit seconds); the first step that fails or runs out of time ends
the run, and nothing more is started on the GPU.  Medians over --iters batches after a warm-up batch, between stream events
around the whole call (launches, the waits for the tables, the copies to the host and the host arithmetic):
  (1) model.structure.table_cells for the batch;
  (2) its stages by themselves: the masks (four launches), the profiles, the separator runs (host), the edges, the cells, the
      merged cells (host), each against the CPU twin's time for the same stage on one thread over the first --twin-pages pages;
  (3) detect_files with and without cells=True over 16 files of the sample page, with an engine that reports the three fixed
      boxes instead of running the network (so the difference is what cells=True adds to a batch; wall clock, files written).
Every step prints one JSON object as its last line; the parent prints them all as one.
For the kernels by themselves: rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -o lattice --
  python tools/bench_lattice.py --step cells --iters 3 --twin-pages 0
"""
import argparse
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "retinanet-for-table-detection_amd"
SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_0717_023_orig.jpg")
BOXES = np.array(((300, 600, 1300, 900), (150.5, 200, 1550, 1000.25), (100, 1200, 900, 2000)), np.float64)      # lattice_cases.GOLDEN_BOXES
KW = dict(flavor="auto", line_scale=15, line_tol=2, cover=50, col_gap=12, row_gap=4, margin=10)
med = lambda v: float(np.median(v))                                           # noqa: E731


def sample_page():
    from PIL import Image
    with Image.open(SAMPLE) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def event_ms(fn, iters):
    """fn() once to warm up, then `iters` times between two stream events each -> (the times in ms, the last result)."""
    import torch
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


def stage_functions(S, be, pages, shapes, boxes):
    """The stages of structure._grids one by one -> ordered name -> callable; each uses the results of those before it."""
    st = {}
    flat = [(i, S.crop_of(b, shapes[i][0], shapes[i][1], KW["margin"])) for i, bs in enumerate(boxes) for b in bs]
    box_page, crops = np.asarray([i for i, _c in flat], np.int32), np.asarray([c for _i, c in flat], np.int32).reshape(-1, 4)

    def masks():
        st["masks"] = S._masks(be, pages, shapes, box_page, crops, KW["line_scale"])

    def profiles():
        _bw, hm, vm, ink, offsets, total = st["masks"]
        profiles, st["prof_offsets"] = S._profiles(be, crops, offsets, total, hm, vm, ink)
        st["prof"] = be.host(profiles)

    def separators():
        rows, cols, flavors = [], [], []
        for j, (_x0, _y0, w, h) in enumerate(crops):
            p = st["prof"][int(st["prof_offsets"][j]):][:2 * (w + h)]
            r, c, f = S.separators(p[:h], 0, KW["line_tol"]), S.separators(p[2 * h:2 * h + w], 0, KW["line_tol"]), "lattice"
            if len(r) < 2 or len(c) < 2:
                r, c, f = S.separators(p[h:2 * h], 1, KW["row_gap"]), S.separators(p[2 * h + w:], 1, KW["col_gap"]), "stream"
            rows.append(r), cols.append(c), flavors.append(f)
        st["runs"], st["flavors"], st["rows"], st["cols"] = S._runs_table(rows, cols), flavors, rows, cols

    def edges():
        _bw, hm, vm, _ink, offsets, total = st["masks"]
        R, C, sep, runs = st["runs"]
        lat = np.array([f == "lattice" for f in st["flavors"]])
        e, st["edge_offsets"] = S._edges(be, crops, offsets, total, np.where(lat, R, 0).astype(np.int32), np.where(lat, C, 0).astype(np.int32),
                                         sep, runs, KW["line_tol"], KW["cover"], hm, vm)
        st["edges"] = be.host(e)

    def cells():
        _bw, _hm, _vm, ink, offsets, total = st["masks"]
        ci, cb, st["cell_offsets"] = S._cells(be, crops, offsets, total, *st["runs"], ink)
        st["cell_ink"], st["cell_box"] = be.host(ci), be.host(cb)

    def merged():
        n = 0
        for j in range(len(crops)):
            nr, nc = len(st["rows"][j]), len(st["cols"][j])
            o, m = int(st["cell_offsets"][j]), (nr - 1) * (nc - 1)
            e = st["edges"][int(st["edge_offsets"][j]):].astype(bool)
            lat = st["flavors"][j] == "lattice"
            h_e = e[:nr * (nc - 1)].reshape(nr, nc - 1) if lat else None
            v_e = e[nr * (nc - 1):nr * (nc - 1) + (nr - 1) * nc].reshape(nr - 1, nc) if lat else None
            n += len(S.merge_cells(st["rows"][j], st["cols"][j], h_e, v_e, st["cell_ink"][o:o + m].reshape(nr - 1, nc - 1),
                                   st["cell_box"][4 * o:4 * (o + m)].reshape(nr - 1, nc - 1, 4), stream=not lat))
        st["n_cells"] = n

    return st, [("masks", masks), ("profiles", profiles), ("separators", separators), ("edges", edges), ("cells", cells), ("merged", merged)]


def step_cells(a):
    import torch
    S = importlib.import_module(PKG + ".model.structure")
    page = sample_page()
    n = a.batch
    dev = [torch.from_numpy(page.copy()).cuda() for _ in range(n)]
    boxes = [BOXES] * n
    out = {"batch": n, "iters": a.iters, "page": list(page.shape), "boxes_per_page": len(BOXES)}
    whole, grids = event_ms(lambda: S.table_cells(dev, boxes), a.iters)
    g0 = grids[0]
    print("batch: %d pages of %dx%dx3, %d boxes each; page 0: %s" % (n, page.shape[0], page.shape[1], len(BOXES), ", ".join(
        "%s %dx%d separators, %d cells" % (g.flavor, len(g.rows), len(g.cols), len(g.cells)) for g in g0)))
    print("(1) %-12s %8.2f ms per batch (%.2f .. %.2f), %.0f pages/s" % ("table_cells", med(whole), min(whole), max(whole), n / med(whole) * 1e3))
    out["table_cells_ms"] = round(med(whole), 2)
    pages, shapes = S._pages.check_pages(dev, S.MIN_SIDE, S.MAX_SIDE)
    st, fns = stage_functions(S, S._pages.Device(pages[0].device), pages, shapes, boxes)
    for name, fn in fns:
        ms, _ = event_ms(fn, a.iters)
        out[name + "_ms"] = round(med(ms), 3)
    crop_px = int(sum(int(c[2]) * int(c[3]) for c in (S.crop_of(b, page.shape[0], page.shape[1], KW["margin"]) for b in BOXES)))
    out["crop_pixels_per_page"], out["page_pixels"] = crop_px, int(page.shape[0] * page.shape[1])
    torch.set_num_threads(1)
    m = min(a.twin_pages, n)
    twin = {}
    if m:
        tp, tshapes = S._pages.check_pages([page] * m, S.MIN_SIDE, S.MAX_SIDE, False)
        tst, tfns = stage_functions(S, S._pages.Twins(), tp, tshapes, boxes[:m])
        for name, fn in tfns:
            t0 = time.perf_counter()
            fn()
            twin[name] = (time.perf_counter() - t0) * 1e3 / m
        t0 = time.perf_counter()
        tw = S.table_cells([page] * m, boxes[:m], device=False)
        twin["table_cells"] = (time.perf_counter() - t0) * 1e3 / m
        same = all(a_.flavor == b_.flavor and np.array_equal(a_.cell_ink, b_.cell_ink) and np.array_equal(a_.rows, b_.rows) and
                   np.array_equal(a_.cols, b_.cols) and a_.cells == b_.cells for a_, b_ in zip(tw[0], g0))
        out["twin_ms_per_page"], out["equal"] = {k: round(v, 2) for k, v in twin.items()}, bool(same)
    for name, _fn in fns:
        line = "(2) %-12s %8.3f ms per batch" % (name, out[name + "_ms"])
        if name in twin:
            line += "; the CPU twin, one thread: %8.2f ms per page (device: %.0fx)" % (twin[name], twin[name] * n / max(out[name + "_ms"], 1e-6))
        print(line)
    if m:
        print("    table_cells through the twins, one thread: %.0f ms per page (device: %.0fx); results equal the device's: %s" %
              (twin["table_cells"], twin["table_cells"] * n / med(whole), out["equal"]))
    print(json.dumps(out))


class FixedBoxes:
    """The inference model detect_files asks for, whose engine reports BOXES for every page (score 0.9, label 0) without a network."""
    bbox, nms, class_specific_filter, dtype = True, True, True, "f32"

    def _root(self):
        return self

    def engine(self):
        return self

    def detect(self, canvas, nms=True, class_specific_filter=True):
        import torch
        n, k = canvas.shape[0], len(BOXES)
        boxes, scores = torch.zeros(n, 300, 4, device="cuda"), torch.full((n, 300), -1.0, device="cuda")
        labels = torch.full((n, 300), -1, dtype=torch.int32, device="cuda")
        boxes[:, :k] = torch.as_tensor(BOXES, dtype=torch.float32, device="cuda") * self.scale
        scores[:, :k], labels[:, :k] = 0.9, 0
        return boxes, scores, labels


def step_detect(a):
    import torch
    U = importlib.import_module(PKG + ".model.utils")
    tmp = tempfile.mkdtemp(prefix="bench_lattice_")
    try:
        paths = []
        for i in range(a.batch):
            paths.append(os.path.join(tmp, "page_%02d.jpg" % i))
            shutil.copyfile(SAMPLE, paths[-1])
        model = FixedBoxes()
        model.scale = U.compute_resize_scale((2200, 1712, 3))
        out = {"batch": a.batch, "iters": a.iters}
        for cells in (False, True):
            t = []
            for it in range(a.iters + 1):
                res = os.path.join(tmp, "out_%d_%d" % (cells, it))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                kept = U.detect_files(model, paths, paths, res, batch_size=a.batch, cells=cells)
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
                n_csv = len(os.listdir(os.path.join(res, "cellResults"))) if cells else 0
                shutil.rmtree(res)
            t = t[1:]
            name = "detect_files_cells_ms" if cells else "detect_files_ms"
            out[name] = round(med(t), 1)
            print("(3) detect_files(cells=%-5s) %8.1f ms per batch of %d files (%.1f .. %.1f), %d kept boxes, %d csv files" %
                  (cells, med(t), a.batch, min(t), max(t), sum(len(k) for k in kept), n_csv))
        out["cells_adds_ms"] = round(out["detect_files_cells_ms"] - out["detect_files_ms"], 1)
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


STEPS = {"cells": step_cells, "detect": step_detect}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--twin-pages", type=int, default=1)
    ap.add_argument("--limit", type=int, default=300, help="seconds every step may take")
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_lattice.py measures on the GPU: none found")
        return STEPS[a.step](a)
    merged = {}
    for step in ("cells", "detect"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(a.batch), "--iters", str(a.iters),
               "--twin-pages", str(a.twin_pages)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("step %s ran past %d s: nothing more is started" % (step, a.limit))
        lines = done.stdout.strip().splitlines()
        if done.returncode != 0 or not lines:
            print(done.stdout)
            raise SystemExit("step %s ended with status %d: nothing more is started" % (step, done.returncode))
        print("\n".join(lines[:-1]))
        merged.update(json.loads(lines[-1]))
    print(json.dumps(merged))


if __name__ == "__main__":
    main()
