"""Time one validation pass over N synthetic pages (tools/bench_eval.py's, 800 x 1333 canvases, --batch pages per group), three ways:
  (a) two passes, the way before validate_generator: per batch generator[j] (dense targets on the device), predict_on_batch (outputs
      to the host), the two functors of model/losses.py (outputs uploaded again, rtn_retina_loss_fwd twice); then evaluate_generator
      over the same pages for mAP (a second forward)
  (b) evaluate_generator alone: mAP, no loss
  (c) validate_generator: loss and mAP from one forward per group
warmed, then repeated and alternated (a b c a b c ...); wall time per pass, page loading included in all three; median and the
min .. max spread of the repeats.  And the device time (events, mean after a warm-up) of
  rtn_retina_loss_boxes_fwd             on one batch, next to
  rtn_anchor_targets + rtn_retina_loss_fwd   on the same batch (the dense targets written, then read).
Every GPU step runs in a child process under `timeout -k`; the parent only starts them and prints their lines.
  python3 tools/bench_validate.py [--pages 32] [--batch 8] [--repeats 5]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "retinanet-for-table-detection_amd"
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _setup():
    sys.path.insert(0, ROOT)
    import importlib
    import torch
    mods = [importlib.import_module(PKG + "." + n) for n in ("model.eval", "model.defineModel", "weights", "csv_generator", "model.losses")]
    return [torch] + mods


def step_variants(d, batch, repeats, in_flight):
    import warnings
    import numpy as np
    torch, E, DM, Wt, CG, Ls = _setup()
    m = DM.Model("resnet50", 1, 9)
    m._state = Wt.init_state("resnet50", 1, 9, seed=2, randomize_bn=True, cls_bias=0.0, tame=True)
    infer = DM.retinanet_bbox(model=m)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gen = CG.CSVGenerator(os.path.join(d, "val.csv"), d, {"table": 0}, batch_size=batch, group_method="none", shuffle_groups=False)
    n = sum(len(g) for g in gen.groups)

    def two_passes(steps=None):
        k = len(gen) if steps is None else steps
        v = np.zeros(2)
        for j in range(k):
            x, y = gen[j]
            r, c = m.predict_on_batch(x)
            v += np.array([float(Ls.smooth_l1()(y[0], r)), float(Ls.focal()(y[1], c))])
        r = E.evaluate_generator(infer, gen, in_flight=in_flight, steps=steps)
        return float(v.sum() / k), r["mAP"]

    def evaluate_only(steps=None):
        return None, E.evaluate_generator(infer, gen, in_flight=in_flight, steps=steps)["mAP"]

    def one_pass(steps=None):
        r = E.validate_generator(infer, gen, in_flight=in_flight, steps=steps)
        return r["loss"], r["mAP"]
    variants = [("(a) loss pass + evaluate_generator", two_passes), ("(b) evaluate_generator alone", evaluate_only),
                ("(c) validate_generator", one_pass)]
    for _, fn in variants:                                   # warm-up: plans, streams, first launches
        fn(steps=1)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    last = {}
    for _ in range(repeats):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    print("%d pages, batch %d, in_flight %d, %d repeats, alternated; wall ms per pass (page loading included)" % (n, batch, in_flight, repeats))
    for name, _ in variants:
        t = np.asarray(times[name])
        loss, mAP = last[name]
        print("%-36s median %8.1f ms  min %8.1f  max %8.1f  %6.2f ms/page   val_loss %s  mAP %.6f"
              % (name, np.median(t), t.min(), t.max(), np.median(t) / n, "%.6f" % loss if loss is not None else "-", mAP))
    gen.close()


def step_kernel(batch, reps):
    import ctypes as C
    import importlib
    import numpy as np
    torch = _setup()[0]
    pkg = importlib.import_module(PKG)
    Eng = importlib.import_module(PKG + ".engine")
    canvas, K = (800, 1333), 1
    cfg, N = Eng.make_anchor_cfg(canvas)
    rng = np.random.RandomState(0)
    gb = np.zeros((batch, 64, 4), np.float64)
    gl = np.zeros((batch, 64), np.int32)
    gc = np.zeros((batch,), np.int32)
    for i in range(batch):
        g = int(rng.randint(1, 4))                           # the pages of this benchmark carry 1 to 3 tables
        bw, bh = rng.uniform(100, 500, g), rng.uniform(80, 400, g)
        x1, y1 = rng.uniform(0, canvas[1] - bw), rng.uniform(0, canvas[0] - bh)
        gb[i, :g], gc[i] = np.stack([x1, y1, x1 + bw, y1 + bh], 1), g
    hw = np.asarray([canvas] * batch, np.int32)
    t = [torch.as_tensor(a).cuda() for a in (gb, gl, gc, hw)]
    cls = torch.rand(batch, N, K, device="cuda") * 0.98 + 0.01
    pred = torch.randn(batch, N, 4, device="cuda")
    h = pkg.Handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    reg = torch.empty(batch, N, 5, dtype=torch.float32, device="cuda")
    lab = torch.empty(batch, N, K + 1, dtype=torch.float32, device="cuda")
    ws1 = torch.empty(pkg.lib.rtn_retina_loss_workspace_bytes(batch * N), dtype=torch.uint8, device="cuda")
    ws2 = torch.empty(pkg.lib.rtn_retina_loss_boxes_workspace_bytes(batch, N), dtype=torch.uint8, device="cuda")
    sums = torch.zeros(4, dtype=torch.float64, device="cuda")
    image_sums = torch.zeros(batch, 4, dtype=torch.float64, device="cuda")

    def dense():
        h.check(pkg.lib.rtn_anchor_targets(h.raw, C.byref(cfg), batch, K, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                           t[3].data_ptr(), 0.4, 0.5, reg.data_ptr(), lab.data_ptr()))
        h.check(pkg.lib.rtn_retina_loss_fwd(h.raw, batch * N, K, lab.data_ptr(), reg.data_ptr(), cls.data_ptr(), pred.data_ptr(),
                                            0.25, 2.0, 3.0, sums.data_ptr(), ws1.data_ptr(), ws1.numel()))

    def boxes():
        h.check(pkg.lib.rtn_retina_loss_boxes_fwd(h.raw, C.byref(cfg), batch, K, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                                  t[3].data_ptr(), 0.4, 0.5, cls.data_ptr(), pred.data_ptr(), 0.25, 2.0, 3.0,
                                                  image_sums.data_ptr(), ws2.data_ptr(), ws2.numel()))
    out = {}
    for name, fn in (("rtn_anchor_targets + rtn_retina_loss_fwd", dense), ("rtn_retina_loss_boxes_fwd", boxes)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        out[name] = np.asarray(ts)
    print("one batch of %d at %d x %d (%d anchors per image, K = %d, 1 to 3 boxes per image); event time, %d launches after a warm-up"
          % (batch, canvas[0], canvas[1], N, K, reps))
    for name, ts in out.items():
        print("%-42s median %7.1f us  min %7.1f  max %7.1f" % (name, np.median(ts), ts.min(), ts.max()))
    torch.cuda.synchronize()
    a, b = sums.cpu().numpy(), image_sums.cpu().numpy().sum(0)
    print("sums over the batch: dense %r  boxes %r" % (a.tolist(), b.tolist()))
    h.close()


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, cwd=ROOT)
    if p.returncode != 0:
        print("step %s ended with status %d: stopping" % (" ".join(args), p.returncode))
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--in-flight", type=int, default=2)
    ap.add_argument("--step", default=None)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    if a.step == "variants":
        return step_variants(a.dir, a.batch, a.repeats, a.in_flight)
    if a.step == "kernel":
        return step_kernel(a.batch, 20)
    from bench_eval import make_pages
    with tempfile.TemporaryDirectory() as d:
        make_pages(d, a.pages)
        child(["--step", "variants", "--dir", d, "--batch", str(a.batch), "--repeats", str(a.repeats), "--in-flight", str(a.in_flight)], 600)
    child(["--step", "kernel", "--batch", str(a.batch)], 300)


if __name__ == "__main__":
    main()
