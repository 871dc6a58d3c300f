"""Measure the colour effects on 16 sample-sized pages (2200 x 1712 x 3 uint8), resident on the device.

  python tools/bench_effect.py [--batch 16] [--iters 20] [--out-dir rocprof_out] [--oracle-pages 1]

The parent process never opens the GPU: it starts every step as a child under `timeout -k` and stops at the first one that fails.
  (1) kernels    rocprofv3 --kernel-trace --stats around rtn_visual_effect_u8 with all four steps on: per kernel the time per
                 page, the algorithmic bytes it moves and the share of the HBM rate (6.29 TB/s measured for a float4 copy) they imply
  (2) device     without the profiler: the entry for the batch between stream events, and the augmented generator batch
                 (warp -> resize -> anchor targets, as tools/bench_generator.py --augment) with and without apply_visual_effect
  (3) oracle     the NumPy oracle (tests/effect_ref.py) on one thread, per page (no GPU)
The last line is one JSON object with the same figures.
"""
import argparse
import csv
import glob
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 2200, 1712
HBM_BYTES_PER_S = 6.29e12
STEP_MS = 25.9                                                               # the training step at batch 16 (README)
KERNELS = ("colsum_kernel", "tables_kernel", "pixels_kernel")
TRAIN_KW = dict(min_rotation=-0.1, max_rotation=0.1, min_translation=(-0.1, -0.1), max_translation=(0.1, 0.1), min_shear=-0.1,
                max_shear=0.1, min_scaling=(0.9, 0.9), max_scaling=(1.1, 1.1), flip_x_chance=0.5, flip_y_chance=0.5)
RANGES = dict(contrast_range=(0.9, 1.1), brightness_range=(-.1, .1), hue_range=(-0.05, 0.05), saturation_range=(0.95, 1.05))


def kernel_bytes():
    """Algorithmic bytes per page of each kernel: pages read and written once, the sums added once per strip of 32 rows."""
    page, strips = H * W * 3, (H + 31) // 32
    return {"colsum_kernel": page + strips * 3 * W * 4, "tables_kernel": 3 * W * 4 + 5 * 256, "pixels_kernel": 2 * page + 5 * 256}


def make_pages(n, np):
    rng = np.random.RandomState(0)
    pages, boxes = [], []
    for _ in range(n):
        base = np.clip(rng.exponential(12.0, (H // 8, W // 8, 3)) * 6 + rng.uniform(0, 120, (1, 1, 3)), 0, 255)
        pages.append(np.kron(base, np.ones((8, 8, 1))).astype(np.uint8))
        g = rng.randint(1, 7)
        w, h = rng.uniform(200, 1400, g), rng.uniform(150, 1200, g)
        x1, y1 = rng.uniform(0, W - w), rng.uniform(0, H - h)
        boxes.append(np.stack([x1, y1, x1 + w, y1 + h], 1))
    return pages, boxes


def draw_params(n, np):
    np.random.seed(2)
    order = ("contrast_range", "brightness_range", "hue_range", "saturation_range")
    return [[np.random.uniform(*RANGES[k]) for k in order] for _ in range(n)]


# ---- the children -----------------------------------------------------------------------------------------------------------------------
def step_kernels(a):
    """Under the profiler: the entry alone, a.iters + 2 calls."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    T = importlib.import_module("retinanet-for-table-detection_amd.model.transform")
    if not torch.cuda.is_available():
        raise SystemExit("bench_effect.py measures on the GPU: none found")
    pages, _ = make_pages(a.batch, np)
    dev = [torch.as_tensor(p).cuda() for p in pages]
    params = draw_params(a.batch, np)
    for _ in range(a.iters + 2):
        T.visual_effect_batch(dev, params)
    torch.cuda.synchronize()


def step_device(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    CG = importlib.import_module("retinanet-for-table-detection_amd.csv_generator")
    T = importlib.import_module("retinanet-for-table-detection_amd.model.transform")
    import effect_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bench_effect.py measures on the GPU: none found")

    class MemoryGenerator(CG.Generator):
        """Pages and boxes held on the device: isolates the batch work from file decoding (tools/bench_generator.py)."""

        def __init__(self, pages, boxes, **kw):
            self.pages, self.boxes = pages, boxes
            super().__init__(**kw)

        def size(self):
            return len(self.pages)

        def num_classes(self):
            return 1

        def image_aspect_ratio(self, i):
            return self.pages[i].shape[1] / self.pages[i].shape[0]

        def load_image(self, i):
            return self.pages[i]

        def load_annotations(self, i):
            return {"labels": np.zeros(len(self.boxes[i])), "bboxes": self.boxes[i].copy()}

    pages, boxes = make_pages(a.batch, np)
    dev = [torch.as_tensor(p).cuda() for p in pages]
    params = draw_params(a.batch, np)
    out = {}
    got = T.visual_effect_batch(dev[:1], params[:1])[0].cpu().numpy()
    out["equal"] = bool(np.array_equal(got, R.effect(pages[0], params[0])))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(a.iters + 2):
        ev[0].record()
        T.visual_effect_batch(dev, params)
        ev[1].record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(ev[0].elapsed_time(ev[1]))
    out["entry_ms"] = [round(float(np.median(ms)), 3), round(min(ms), 3), round(max(ms), 3)]
    gens = {}
    for label, on in (("without", False), ("with", True)):
        gens[label] = MemoryGenerator(dev, boxes, batch_size=a.batch, group_method="none", shuffle_groups=False, dtype=torch.bfloat16,
                                      transform_generator=T.random_transform_generator(prng=np.random.RandomState(1), **TRAIN_KW),
                                      transform_parameters=T.TransformParameters(),
                                      visual_effect_generator=T.random_visual_effect_generator(**RANGES), apply_visual_effect=on)
    times = {"without": [], "with": []}
    for i in range(a.iters + 3):                                             # the two generators alternate: the same noise for both
        for label, gen in gens.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gen[0]
            torch.cuda.synchronize()
            if i >= 3:
                times[label].append((time.perf_counter() - t0) * 1e3)
    for label, gen in gens.items():
        v = times[label]
        out["generator_%s_ms" % label] = [round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)]
        gen.close()
    print("DEVICE " + json.dumps(out))


def step_oracle(a):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import effect_ref as R
    try:
        import torch
        torch.set_num_threads(1)
    except ImportError:
        pass
    pages, _ = make_pages(a.oracle_pages, np)
    params = draw_params(a.oracle_pages, np)
    t0 = time.perf_counter()
    for p, q in zip(pages, params):
        R.effect(p, q)
    print("ORACLE " + json.dumps({"oracle_ms_per_page": round((time.perf_counter() - t0) / a.oracle_pages * 1e3, 1)}))


# ---- the parent ---------------------------------------------------------------------------------------------------------------------
def child(limit_s, argv, a, capture=False):
    cmd = ["timeout", "-k", "10", str(limit_s)] + argv + ["--batch", str(a.batch), "--iters", str(a.iters), "--oracle-pages", str(a.oracle_pages)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE if capture else None, text=True)
    if r.returncode != 0:
        raise SystemExit("bench_effect.py: step failed with exit status %d, nothing more is started: %s" % (r.returncode, " ".join(cmd)))
    return r.stdout or ""


def tagged(text, tag):
    for line in text.splitlines():
        if line.startswith(tag + " "):
            return json.loads(line[len(tag) + 1:])
    raise SystemExit("bench_effect.py: no %s line in the step's output" % tag)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--oracle-pages", type=int, default=1)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "rocprof_out"))
    ap.add_argument("--step", choices=("kernels", "device", "oracle"))
    a = ap.parse_args()
    if a.step:
        return {"kernels": step_kernels, "device": step_device, "oracle": step_oracle}[a.step](a)
    me = [sys.executable, os.path.abspath(__file__)]
    out = {"batch": a.batch, "iters": a.iters, "page": [H, W, 3]}
    print("batch: %d pages of %dx%dx3, all four steps on (the generator's default ranges)" % (a.batch, H, W))

    prof = os.path.join(a.out_dir, "effect")
    child(600, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "effect", "--"] + me + ["--step", "kernels"], a,
          capture=True)
    files = sorted(glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    if not files:
        raise SystemExit("bench_effect.py: the profiler left no kernel_stats.csv under %s" % prof)
    rows = {}
    with open(files[-1], newline="") as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k in row["Name"]:
                    rows[k] = row
    nbytes = kernel_bytes()
    print("(1) per kernel, from %d launches each of %d pages (rocprofv3 --kernel-trace --stats):" % (int(rows[KERNELS[2]]["Calls"]), a.batch))
    for k in KERNELS:
        avg, lo = float(rows[k]["AverageNs"]) / 1e3 / a.batch, float(rows[k]["MinNs"]) / 1e3 / a.batch
        rate = nbytes[k] / (avg * 1e-6)
        print("    %-14s %8.3f us per page (best launch %.3f), %10.3f MB per page -> %7.1f GB/s, %5.1f %% of the HBM rate" %
              (k, avg, lo, nbytes[k] / 1e6, rate / 1e9, 100 * rate / HBM_BYTES_PER_S))
        out[k] = {"us_per_page": round(avg, 3), "best_us_per_page": round(lo, 3), "bytes_per_page": nbytes[k],
                  "hbm_share": round(rate / HBM_BYTES_PER_S, 4)}

    dev = tagged(child(900, me + ["--step", "device"], a, capture=True), "DEVICE")
    out.update(dev)
    e, g0, g1 = dev["entry_ms"], dev["generator_without_ms"], dev["generator_with_ms"]
    print("(2) rtn_visual_effect_u8 for the batch: %.3f ms (%.3f .. %.3f), %.1f us per page; page 0 equals the oracle: %s" %
          (e[0], e[1], e[2], e[0] * 1e3 / a.batch, dev["equal"]))
    print("    augmented generator batch: %.2f ms (%.2f .. %.2f) without effects, %.2f ms (%.2f .. %.2f) with apply_visual_effect;"
          " the training step at batch 16 is %.1f ms: the generator %s hidden behind it" %
          (g0[0], g0[1], g0[2], g1[0], g1[1], g1[2], STEP_MS, "stays" if g1[0] < STEP_MS else "is NOT"))
    if a.oracle_pages > 0:
        o = tagged(child(900, me + ["--step", "oracle"], a, capture=True), "ORACLE")
        out.update(o)
        print("(3) the NumPy oracle, one thread: %.0f ms per page (device entry: %.0fx)" %
              (o["oracle_ms_per_page"], o["oracle_ms_per_page"] * a.batch / e[0]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
