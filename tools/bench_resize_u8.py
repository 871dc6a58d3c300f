"""Measure the 8-bit bicubic resize on the reference's two low-resolution scan sizes: 16 pages of 612 x 792 x 3 enlarged
by 4.17 (to 2552 x 3303) and 16 of 850 x 1100 x 3 by 3 (to 2550 x 3300).

  python tools/bench_resize_u8.py [--batch 16] [--iters 20] [--cpu-pages 2] [--detect-batch 8] > profiles/resize_u8_bench.txt

The parent process never opens the GPU: it starts every step as a child under `timeout -k` and stops at the first one that fails.
  (1) device   rtn_resize_u8 for the batch between stream events (pages and outputs resident, 3 warm-up calls), the bytes it
               writes per second as a share of 6.3 TB/s; page 0 against the CPU twin; interpolate_files JPEG -> JPEG, wall clock
  (2) detect   detect_raw_files against interpolate_files + preprocess_files + detect_files on the 612 x 792 scans (random
               weights, bf16), wall clock of the second run of each
  (3) cpu      on one thread, per page: the CPU twin (rtn_resize_u8_host), Pillow's Image.resize(BICUBIC) (a time comparator only:
               its kernel is not cv2's), and the file loop Pillow read / twin / Pillow write at quality 95 (no GPU)
The last line is one JSON object with the same figures.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "retinanet-for-table-detection_amd"
HBM_BYTES_PER_S = 6.3e12
WORKLOADS = (("72 dpi", 612, 792, 4.17), ("100 dpi", 850, 1100, 3.0))          # name, width, height, factor


def make_page(np, w, h, seed):
    """A scan-like page: paper with noise, lines of dark word-sized blobs, a ruled table."""
    rng = np.random.RandomState(seed)
    page = np.clip(235 + rng.normal(0, 4, (h, w, 1)) + rng.normal(0, 2, (h, w, 3)), 0, 255)
    for y in range(h // 12, h - h // 12, max(h // 60, 6)):
        x = w // 10
        while x < w - w // 10:
            n = rng.randint(w // 60 + 1, w // 12 + 2)
            page[y:y + max(h // 160, 2), x:min(x + n, w - w // 10)] = rng.uniform(20, 90)
            x += n + rng.randint(3, w // 40 + 4)
    for y in range(h // 2, h // 2 + h // 5, h // 25):
        page[y:y + 1, w // 8:w - w // 8] = 30
    return page.astype(np.uint8)


def host_arrays(np, pages, f):
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    ho, wo = [int(np.rint(p.shape[0] * f)) for p in pages], [int(np.rint(p.shape[1] * f)) for p in pages]
    n = len(pages)
    return (i32([p.shape[0] for p in pages]), i32([p.shape[1] for p in pages]), i32([3] * n), i32(ho), i32(wo),
            np.full(n, 1.0 / f), np.full(n, 1.0 / f)), ho, wo


def stats(np, v):
    return [round(float(np.median(v)), 3), round(float(min(v)), 3), round(float(max(v)), 3)]


# ---- the children -----------------------------------------------------------------------------------------------------------------------
def step_device(a):
    import numpy as np
    import torch
    from PIL import Image
    sys.path.insert(0, ROOT)
    P = importlib.import_module(PKG + ".model.preprocess")
    rt = importlib.import_module(PKG + ".model._rt")
    L = rt.L
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize_u8.py measures on the GPU: none found")
    out = {}
    for name, w, h, f in WORKLOADS:
        pages = [make_page(np, w, h, 10 + i) for i in range(a.batch)]
        dev = [torch.as_tensor(p).cuda() for p in pages]
        arrays, ho, wo = host_arrays(np, pages, f)
        outs = [torch.empty(ho[i], wo[i], 3, dtype=torch.uint8, device="cuda") for i in range(a.batch)]
        hd = rt.handle()
        wsb = int(L.lib.rtn_resize_u8_workspace_bytes(a.batch))
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        sp = (C.c_void_p * a.batch)(*[d.data_ptr() for d in dev])
        dp = (C.c_void_p * a.batch)(*[o.data_ptr() for o in outs])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = []
        for i in range(a.iters + 3):
            ev[0].record()
            hd.check(L.lib.rtn_resize_u8(hd.raw, a.batch, sp, *[v.ctypes.data for v in arrays], dp, ws.data_ptr(), wsb))
            ev[1].record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(ev[0].elapsed_time(ev[1]))
        twin = np.zeros((ho[0], wo[0], 3), np.uint8)
        one = [v[:1].copy() for v in arrays]
        assert L.lib.rtn_resize_u8_host(1, (C.c_void_p * 1)(pages[0].ctypes.data), *[v.ctypes.data for v in one], (C.c_void_p * 1)(twin.ctypes.data)) == 0
        written = sum(ho[i] * wo[i] * 3 for i in range(a.batch))
        read = sum(p.size for p in pages)
        d = tempfile.mkdtemp()
        src = [os.path.join(d, "p%02d-in.jpg" % i) for i in range(a.batch)]
        dst = [os.path.join(d, "p%02d-out.jpg" % i) for i in range(a.batch)]
        for p, s in zip(pages, src):
            Image.fromarray(p[:, :, ::-1]).save(s, "JPEG", quality=95)
        wall = []
        for i in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P.interpolate_files(src, dst, factors=[f] * a.batch)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"page": [h, w, 3], "factor": f, "out": [ho[0], wo[0], 3], "launch_ms": stats(np, ms), "written_bytes": written,
                     "read_bytes": read, "equal_twin": bool(np.array_equal(outs[0].cpu().numpy(), twin)),
                     "files_ms": [round(v, 1) for v in wall], "file_bytes_out": sum(os.path.getsize(p) for p in dst)}
    print("DEVICE " + json.dumps(out))


def step_detect(a):
    import numpy as np
    import torch
    from PIL import Image
    sys.path.insert(0, ROOT)
    P = importlib.import_module(PKG + ".model.preprocess")
    U = importlib.import_module(PKG + ".model.utils")
    D = importlib.import_module(PKG + ".model.defineModel")
    Wt = importlib.import_module(PKG + ".weights")
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize_u8.py measures on the GPU: none found")
    name, w, h, f = WORKLOADS[0]
    d = tempfile.mkdtemp()
    src = [os.path.join(d, "scan%02d-72.jpg" % i) for i in range(a.batch)]
    for i, s in enumerate(src):
        Image.fromarray(make_page(np, w, h, 10 + i)[:, :, ::-1]).save(s, "JPEG", quality=95)
    m = D.Model("resnet50", 1, 9, dtype="bf16")
    m._state = Wt.init_state("resnet50", 1, 9, seed=0, tame=True)             # the default bias: few detections, as after training
    pm = D.retinanet_bbox(model=m)
    big = [os.path.join(d, "big_" + os.path.basename(s)) for s in src]
    proc = [os.path.join(d, "proc_" + os.path.basename(s)) for s in src]
    times = {"raw": [], "files": [], "files_interpolate": [], "files_preprocess": [], "files_detect": []}
    for i in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        U.detect_raw_files(pm, src, os.path.join(d, "raw%d" % i), batch_size=a.detect_batch)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        P.interpolate_files(src, big)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        P.preprocess_files(big, proc)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        U.detect_files(pm, proc, big, os.path.join(d, "files%d" % i), batch_size=a.detect_batch)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        for k, v in (("raw", t1 - t0), ("files", t4 - t1), ("files_interpolate", t2 - t1), ("files_preprocess", t3 - t2), ("files_detect", t4 - t3)):
            times[k].append(round(v * 1e3, 1))
    print("DETECT " + json.dumps({"pages": a.batch, "detect_batch": a.detect_batch, **times}))


def step_cpu(a):
    import numpy as np
    from PIL import Image
    sys.path.insert(0, ROOT)
    try:
        import torch
        torch.set_num_threads(1)
    except ImportError:
        pass
    L = importlib.import_module(PKG)._lib
    out = {}
    for name, w, h, f in WORKLOADS:
        twin_ms, pillow_ms, loop_ms = [], [], []
        d = tempfile.mkdtemp()
        for i in range(a.cpu_pages):
            page = make_page(np, w, h, 10 + i)
            arrays, ho, wo = host_arrays(np, [page], f)
            res = np.zeros((ho[0], wo[0], 3), np.uint8)
            call = lambda p, r: L.lib.rtn_resize_u8_host(1, (C.c_void_p * 1)(p.ctypes.data), *[v.ctypes.data for v in arrays], (C.c_void_p * 1)(r.ctypes.data))
            t0 = time.perf_counter()
            assert call(page, res) == 0
            twin_ms.append((time.perf_counter() - t0) * 1e3)
            im = Image.fromarray(page)
            t0 = time.perf_counter()
            im.resize((wo[0], ho[0]), Image.BICUBIC)
            pillow_ms.append((time.perf_counter() - t0) * 1e3)
            s, t = os.path.join(d, "in%d.jpg" % i), os.path.join(d, "out%d.jpg" % i)
            Image.fromarray(page[:, :, ::-1]).save(s, "JPEG", quality=95)
            t0 = time.perf_counter()
            with Image.open(s) as fimg:
                bgr = np.ascontiguousarray(np.asarray(fimg.convert("RGB"))[:, :, ::-1])
            assert call(bgr, res) == 0
            Image.fromarray(res[:, :, ::-1]).save(t, "JPEG", quality=95, subsampling=2)
            loop_ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"twin_ms_per_page": round(float(np.median(twin_ms)), 1), "pillow_bicubic_ms_per_page": round(float(np.median(pillow_ms)), 1),
                     "file_loop_ms_per_page": round(float(np.median(loop_ms)), 1)}
    print("CPU " + json.dumps(out))


# ---- the parent ---------------------------------------------------------------------------------------------------------------------
def child(limit_s, argv, a):
    cmd = ["timeout", "-k", "10", str(limit_s)] + argv + ["--batch", str(a.batch), "--iters", str(a.iters), "--cpu-pages", str(a.cpu_pages),
                                                          "--detect-batch", str(a.detect_batch)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit("bench_resize_u8.py: step failed with exit status %d, nothing more is started: %s" % (r.returncode, " ".join(cmd)))
    return r.stdout or ""


def tagged(text, tag):
    for line in text.splitlines():
        if line.startswith(tag + " "):
            return json.loads(line[len(tag) + 1:])
    raise SystemExit("bench_resize_u8.py: no %s line in the step's output" % tag)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-pages", type=int, default=2)
    ap.add_argument("--detect-batch", type=int, default=8)
    ap.add_argument("--step", choices=("device", "detect", "cpu"))
    a = ap.parse_args()
    if a.step:
        return {"device": step_device, "detect": step_detect, "cpu": step_cpu}[a.step](a)
    me = [sys.executable, os.path.abspath(__file__)]
    out = {"batch": a.batch, "iters": a.iters}
    dev = tagged(child(600, me + ["--step", "device"], a), "DEVICE")
    cpu = tagged(child(900, me + ["--step", "cpu"], a), "CPU") if a.cpu_pages > 0 else {}
    out["device"], out["cpu"] = dev, cpu
    print("(1) rtn_resize_u8, %d pages per launch, %d launches after 3 warm-up calls (stream events around the call):" % (a.batch, a.iters))
    for name, _w, _h, _f in WORKLOADS:
        v = dev[name]
        rate = v["written_bytes"] / (v["launch_ms"][0] * 1e-3)
        print("    %-8s %dx%dx3 by %g -> %dx%dx3: %.3f ms (%.3f .. %.3f), %.1f us per page; reads %.1f MB, writes %.1f MB -> %.0f GB/s"
              " written, %.1f %% of 6.3 TB/s; page 0 equals the CPU twin: %s" %
              (name, v["page"][1], v["page"][0], v["factor"], v["out"][1], v["out"][0], v["launch_ms"][0], v["launch_ms"][1], v["launch_ms"][2],
               v["launch_ms"][0] * 1e3 / a.batch, v["read_bytes"] / 1e6, v["written_bytes"] / 1e6, rate / 1e9, 100 * rate / HBM_BYTES_PER_S,
               v["equal_twin"]))
        print("             interpolate_files JPEG -> JPEG (quality 95), %d files: %s ms wall clock (three runs), %.1f MB of files written" %
              (a.batch, " / ".join("%.1f" % x for x in v["files_ms"]), v["file_bytes_out"] / 1e6))
        if cpu:
            c = cpu[name]
            print("             one CPU thread, per page: twin %.1f ms, Pillow BICUBIC %.1f ms (another kernel: time only), Pillow read / twin /"
                  " Pillow write %.1f ms; the launch is %.0fx the twin, interpolate_files %.1fx the file loop" %
                  (c["twin_ms_per_page"], c["pillow_bicubic_ms_per_page"], c["file_loop_ms_per_page"],
                   c["twin_ms_per_page"] * a.batch / v["launch_ms"][0], c["file_loop_ms_per_page"] * a.batch / min(v["files_ms"])))
    det = tagged(child(900, me + ["--step", "detect"], a), "DETECT")
    out["detect"] = det
    print("(2) %d scans of 612x792 named *-72.jpg, batches of %d, random weights, bf16, wall clock of the second run:" % (det["pages"], det["detect_batch"]))
    print("    detect_raw_files %.1f ms; interpolate_files + preprocess_files + detect_files through JPEG files %.1f ms (%.1f + %.1f + %.1f)" %
          (det["raw"][1], det["files"][1], det["files_interpolate"][1], det["files_preprocess"][1], det["files_detect"][1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
