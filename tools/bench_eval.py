"""Time the detection evaluators (model/eval.py):
  host    evaluate(): predict_on_batch page by page + evaluate_detections' Python loop (one IoU call per image and class), t = 0.5
  device  evaluate_generator(): the generator's canvases, Engine.detect with in_flight batches, DeviceEvaluator (csrc/rtn_eval.hip)
both on the same N synthetic pages (written as PNG files + a CSV, read by a CSVGenerator, batch 1 for host, --batch for device),
seeded weights with classification bias 0 (every page yields 300 detections), and
  kernels rtn_eval_match + rtn_eval_finalize alone on detect-format arrays (--images x 300 detections, K = 1, T = 1 and 10),
          CUDA events, mean of 5 after a warm-up.
Every GPU step runs in a child process under `timeout -k`; the parent only starts them and prints their lines.
  python3 tools/bench_eval.py [--pages 64] [--batch 8] [--images 10000]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "retinanet-for-table-detection_amd"


def make_pages(d, n, seed=0):
    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        h, w = int(rng.randint(900, 1100)), int(rng.randint(700, 850))
        base = np.clip(rng.exponential(12.0, (h // 8 + 2, w // 8 + 2, 3)) * 6, 0, 255)
        page = np.kron(base, np.ones((8, 8, 1)))[:h, :w].astype(np.uint8)
        name = "page_%03d.png" % i
        Image.fromarray(page[:, :, ::-1]).save(os.path.join(d, name))
        for _ in range(int(rng.randint(1, 4))):
            bw, bh = rng.uniform(100, 500), rng.uniform(80, 400)
            x1, y1 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
            rows.append("%s,%.2f,%.2f,%.2f,%.2f,table" % (name, x1, y1, x1 + bw, y1 + bh))
    with open(os.path.join(d, "val.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")


def _setup():
    sys.path.insert(0, ROOT)
    import importlib
    import torch
    E = importlib.import_module(PKG + ".model.eval")
    DM = importlib.import_module(PKG + ".model.defineModel")
    Wt = importlib.import_module(PKG + ".weights")
    CG = importlib.import_module(PKG + ".csv_generator")
    return torch, E, DM, Wt, CG


def step_pages(d, batch, mode, in_flight):
    import warnings
    import numpy as np
    torch, E, DM, Wt, CG = _setup()
    m = DM.Model("resnet50", 1, 9)
    m._state = Wt.init_state("resnet50", 1, 9, seed=2, randomize_bn=True, cls_bias=0.0, tame=True)
    infer = DM.retinanet_bbox(model=m)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gen = CG.CSVGenerator(os.path.join(d, "val.csv"), d, {"table": 0}, batch_size=1 if mode == "host" else batch,
                              group_method="none", shuffle_groups=False)
    if mode == "host":
        images, anns, scales = [], [], []
        for group in gen.groups:
            canvas, sc, an = E._generator_batch(gen, group)
            images.append(canvas[0].float().cpu().numpy())
            scales += sc
            anns += [np.concatenate([a["bboxes"], np.asarray(a["labels"], np.float64)[:, None]], 1) for a in an]
        E.evaluate(infer, images[:1], anns[:1], scales=scales[:1])          # warm-up: plans, first launches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = E.evaluate(infer, images, anns, scales=scales)
        dt = time.perf_counter() - t0
        print("host   evaluate            %4d pages  %8.1f ms  %6.2f ms/page  AP50 %.6f  (page loading not timed)"
              % (len(images), dt * 1e3, dt * 1e3 / len(images), r[0][0]))
    else:
        E.evaluate_generator(infer, gen, in_flight=in_flight, steps=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = E.evaluate_generator(infer, gen, iou_thresholds=E.COCO_IOU_THRESHOLDS, in_flight=in_flight)
        dt = time.perf_counter() - t0
        n = sum(len(g) for g in gen.groups)
        print("device evaluate_generator  %4d pages  %8.1f ms  %6.2f ms/page  AP50 %.6f  mAP50:95 %.6f  (batch %d, in_flight %d, "
              "page loading timed)" % (n, dt * 1e3, dt * 1e3 / n, r["average_precision"][0.5][0][0], r["map_50_95"], batch, in_flight))
    gen.close()


def step_kernels(n_img):
    import numpy as np
    torch, E, _, _, _ = _setup()
    rng = np.random.default_rng(0)
    D = 300
    for T in (1, 10):
        thresholds = E.COCO_IOU_THRESHOLDS[:T]
        boxes = torch.as_tensor(rng.uniform(0, 800, (n_img, D, 4)).astype(np.float32)).cuda()
        boxes[..., 2:] += boxes[..., :2]
        scores = torch.as_tensor(np.sort(rng.uniform(0.06, 1, (n_img, D)).astype(np.float32), 1)[:, ::-1].copy()).cuda()
        labels = torch.zeros(n_img, D, dtype=torch.int32, device="cuda")
        anns = []
        for i in range(n_img):
            g = rng.uniform(0, 800, (4, 2))
            anns.append(np.concatenate([g, g + rng.uniform(50, 400, (4, 2)), np.zeros((4, 1))], 1))
        scales = [1.0] * n_img
        times = []
        for rep in range(6):
            ev = E.DeviceEvaluator(1, thresholds)
            ev.reserve(n_img)
            ev.add(boxes[:1], scores[:1], labels[:1], scales[:1], anns[:1])       # H2D of the annotations: outside the events
            torch.cuda.synchronize()
            ev2 = E.DeviceEvaluator(1, thresholds)
            ev2.reserve(n_img)
            # stage (a) per batch of 8 pages as in training-time evaluation, then stage (b); annotation uploads are included
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            for lo in range(0, n_img, 8):
                ev2.add(boxes[lo:lo + 8], scores[lo:lo + 8], labels[lo:lo + 8], scales[lo:lo + 8], anns[lo:lo + 8])
            e1.record()
            ws = int(E._rt.L.lib.rtn_eval_workspace_bytes(n_img * D, 1, T))
            ev2._ws = torch.empty(ws, dtype=torch.uint8, device="cuda")
            ev2._join()
            r = ev2.result()
            e2.record()
            torch.cuda.synchronize()
            if rep:
                times.append((e0.elapsed_time(e1), e1.elapsed_time(e2)))
        a, b = np.mean(times, 0)
        print("kernels %5d images x %d dets, T=%2d: stage (a) %7.2f ms (%4d adds of 8)  stage (b) + result copy %6.2f ms  AP50 %.6f"
              % (n_img, D, T, a, (n_img + 7) // 8, b, r["average_precision"][0.5][0][0]))


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, cwd=ROOT)
    if p.returncode != 0:
        print("step %s ended with status %d: stopping" % (" ".join(args), p.returncode))
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--step", default=None)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--in-flight", type=int, default=2)
    a = ap.parse_args()
    if a.step == "host":
        return step_pages(a.dir, a.batch, "host", 1)
    if a.step == "device":
        return step_pages(a.dir, a.batch, "device", a.in_flight)
    if a.step == "kernels":
        return step_kernels(a.images)
    with tempfile.TemporaryDirectory() as d:
        make_pages(d, a.pages)
        child(["--step", "host", "--dir", d], 900)
        child(["--step", "device", "--dir", d, "--batch", str(a.batch), "--in-flight", str(a.in_flight)], 600)
        child(["--step", "device", "--dir", d, "--batch", str(a.batch), "--in-flight", "1"], 600)
    child(["--step", "kernels", "--images", str(a.images)], 600)


if __name__ == "__main__":
    main()
