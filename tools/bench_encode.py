"""Measure the device JPEG encoder (csrc/rtn_jpeg_enc.hip) on the sample-sized page: 2200x1712, built by tiling
tests/golden/sample_page_crop.npz's processed_rgb, encoded q95 4:2:0 (what cv2.imwrite writes for a .jpg name), 16 pages a batch.

  python tools/bench_encode.py [--batch 16] [--iters 10]

Reports, device and host paths alternating inside every iteration, medians over --iters after a warm-up:
  (1) GPU time of the five encode kernels per batch (events around rtn_jpeg_encode, pages resident on the device), and the
      achieved GB/s over the algorithmic bytes: pages read, coefficients written and read twice, the packed stream zeroed,
      written and read, the files written;
  (2) wall time of model.page_io.write_images_bgr for the 16 device pages (encode, length read-back, one copy, 16 file writes);
  (3) the parent commit's path for the same files: Pillow save at the same quality and subsampling, one thread;
  (4) model.preprocess.preprocess_files of 16 JPEG pages (tests/golden/sample_0717_023_orig.jpg) against the parent's path:
      read_images_bgr + preprocess_pages + Pillow save.
For the per-kernel split: rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -o jpeg_enc --
  python tools/bench_encode.py --iters 3
"""
import argparse
import ctypes as C
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
PIO = importlib.import_module(PKG + ".model.page_io")
P = importlib.import_module(PKG + ".model.preprocess")
Q, SS = 95, 2


def make_page():
    crop = np.load(os.path.join(ROOT, "tests", "golden", "sample_page_crop.npz"))["processed_rgb"]
    h, w = 2200, 1712
    return np.ascontiguousarray(np.tile(crop, (h // crop.shape[0] + 1, w // crop.shape[1] + 1, 1))[:h, :w])


def pillow_save(path, page, quality=Q):
    Image.fromarray(page[:, :, ::-1]).save(path, "JPEG", quality=quality, subsampling=SS)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    n = a.batch
    dev = torch.device("cuda", 0)
    page = make_page()
    H, W = page.shape[:2]
    b = io.BytesIO()
    pillow_save(b, page)
    want = b.getvalue()
    tmp = tempfile.mkdtemp(prefix="bench_encode_")

    # (1) kernels alone, pages resident
    pages = [torch.from_numpy(page).to(dev) for _ in range(n)]
    arr = lambda v: np.asarray([v] * n, np.int32)                        # noqa: E731
    Wa, Ha, Ca, Sa, Qa = arr(W), arr(H), arr(3), arr(SS), arr(Q)
    bound = int(L.lib.rtn_jpeg_encode_bound(W, H, 3, SS))
    offs = np.arange(n + 1, dtype=np.int64) * bound
    out = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)
    lengths = torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    wsb = int(L.lib.rtn_jpeg_encode_workspace_bytes(n, Wa.ctypes.data, Ha.ctypes.data, Ca.ctypes.data, Sa.ctypes.data))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in pages])
    h = L.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def encode():
        h.check(L.lib.rtn_jpeg_encode(h.raw, n, ptrs, Wa.ctypes.data, Ha.ctypes.data, Ca.ctypes.data, Sa.ctypes.data, Qa.ctypes.data,
                                      out.data_ptr(), offs.ctypes.data, lengths.data_ptr(), status.data_ptr(), ws.data_ptr(), wsb))
    for _ in range(3):
        encode()
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    ln = lengths.cpu().numpy()
    assert all(int(v) == len(want) for v in ln), (ln, len(want))
    assert bytes(out[int(offs[n - 1]):int(offs[n - 1]) + len(want)].cpu().numpy()) == want
    mcux, mcuy = (W + 15) // 16, (H + 15) // 16
    nblocks = mcux * mcuy * 6
    scan = len(want) - 623 - 2
    alg_bytes = n * (H * W * 3 + 3 * nblocks * 128 + 3 * scan + len(want))
    print("page: %dx%d B,G,R, q%d 4:2:0: %d blocks, file %d B, bound %d B, workspace %.1f MB per page" %
          (W, H, Q, nblocks, len(want), bound, wsb / n / 1e6))

    paths = [os.path.join(tmp, "out_%02d.jpg" % i) for i in range(n)]
    ref_paths = [os.path.join(tmp, "ref_%02d.jpg" % i) for i in range(n)]
    host_pages = [page.copy() for _ in range(n)]
    src = os.path.join(ROOT, "tests", "golden", "sample_0717_023_orig.jpg")
    srcs = [shutil.copy(src, os.path.join(tmp, "src_%02d.jpg" % i)) for i in range(n)]
    pre_dst = [os.path.join(tmp, "pre_%02d.jpg" % i) for i in range(n)]
    pre_ref = [os.path.join(tmp, "preref_%02d.jpg" % i) for i in range(n)]

    def parent_preprocess():
        dp = PIO.read_images_bgr(srcs)
        processed = P.preprocess_pages(torch.stack(dp).cpu().numpy())
        for p, d in zip(processed, pre_ref):
            pillow_save(d, p)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    k_ms, w_ms, p_ms, f_ms, r_ms = [], [], [], [], []
    for it in range(a.iters + 1):                        # iteration 0 warms every path up
        ev[0].record()
        encode()
        ev[1].record()
        torch.cuda.synchronize()
        k = ev[0].elapsed_time(ev[1])
        w = wall_ms(lambda: PIO.write_images_bgr(paths, pages))
        p = wall_ms(lambda: [pillow_save(d, hp) for d, hp in zip(ref_paths, host_pages)])
        f = wall_ms(lambda: P.preprocess_files(srcs, pre_dst))
        r = wall_ms(parent_preprocess)
        if it:
            k_ms.append(k); w_ms.append(w); p_ms.append(p); f_ms.append(f); r_ms.append(r)
    for d, r in zip(paths + pre_dst, ref_paths + pre_ref):
        assert open(d, "rb").read() == open(r, "rb").read(), d
    med = lambda v: float(np.median(v))                                   # noqa: E731
    kern, wr, pil, pf, par = med(k_ms), med(w_ms), med(p_ms), med(f_ms), med(r_ms)
    print("(1) encode kernels: %.3f ms per batch of %d (%.0f pages/s on the GPU), %.0f GB/s over %.1f MB of algorithmic traffic" %
          (kern, n, n / kern * 1e3, alg_bytes / kern / 1e6, alg_bytes / 1e6))
    print("(2) write_images_bgr: %.1f ms per %d files (%.0f pages/s)" % (wr, n, n / wr * 1e3))
    print("(3) Pillow save, one thread: %.1f ms per %d files (%.1f ms per page, %.1f pages/s)" % (pil, n, pil / n, n / pil * 1e3))
    print("    (2) is %.1fx (3)" % (pil / wr))
    print("(4) preprocess_files: %.1f ms per %d JPEG pages; parent path (read_images_bgr + preprocess_pages + Pillow save) %.1f ms "
          "(%.1fx)" % (pf, n, par, par / pf))
    print(json.dumps({"batch": n, "quality": Q, "subsampling": SS, "kernels_ms": round(kern, 3),
                      "kernels_gb_s": round(alg_bytes / kern / 1e6, 1), "write_images_bgr_ms": round(wr, 2),
                      "write_images_bgr_pages_s": round(n / wr * 1e3, 1), "pillow_ms_per_page": round(pil / n, 2),
                      "pillow_pages_s": round(n / pil * 1e3, 2), "speedup_2_over_3": round(pil / wr, 1),
                      "preprocess_files_ms": round(pf, 1), "parent_preprocess_ms": round(par, 1),
                      "speedup_4": round(par / pf, 1)}))
    h.close()
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
