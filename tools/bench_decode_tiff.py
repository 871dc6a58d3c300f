"""Measure the device TIFF decoder (csrc/rtn_tiff.hip) on sample-sized pages: the 2200x1712 sample page
(tests/golden/sample_0717_023_orig.jpg) converted with Pillow to the kinds of TIFF a scan archive holds:

  g4                 bilevel, CCITT Group 4, Pillow's default strips        g4_one_strip       the same page as ONE strip
  packbits_bilevel   bilevel, PackBits                                      lzw_gray           8-bit gray, LZW
  lzw_rgb_predictor  R,G,B, LZW with predictor 2                            deflate_rgb        R,G,B, Deflate
  raw_rgb            R,G,B, no compression

  python tools/bench_decode_tiff.py [--iters 10] [--kinds g4,lzw_gray,...] [--batches 1,2,4,8,16]

For every kind and for 1, 2, 4, 8 and 16 files it reports medians and the min..max spread over the iterations after a warm-up, every
path on the same machine and the same files:
  (a) wall time of read_images_bgr with RTN_TIFF_MIN=1 and RTN_TIFF_G4_ONE_STRIP=1 (read, inspect, one copy, decode, status read-back);
  (b) read_image_bgr (Pillow) on one thread, which is what read_images_bgr does with these files without the device path;
  (c) the same decode spread over 16 host threads;
and, at 16 files, the GPU time of the two decode kernels alone (events around rtn_tiff_decode, blobs already on the device) and the
host time of rtn_tiff_inspect per page.  The last line of a kind says from which batch size on the device path beats (b).
For the per-kernel split: rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -o tiff_dec --
  python tools/bench_decode_tiff.py --iters 3 --batches 16
"""
import argparse
import ctypes as C
import importlib
import io
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "retinanet-for-table-detection_amd"
L = importlib.import_module(PKG + "._lib")
PIO = importlib.import_module(PKG + ".model.page_io")
GOLDEN = os.path.join(ROOT, "tests", "golden")
KINDS = ("g4", "g4_one_strip", "packbits_bilevel", "lzw_gray", "lzw_rgb_predictor", "deflate_rgb", "raw_rgb")


def stat(v):
    return (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def times_ms(fn, iters):
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def tiff(im, compression, **tiffinfo):
    b = io.BytesIO()
    im.save(b, "TIFF", compression=compression, tiffinfo={int(k[1:]): v for k, v in tiffinfo.items()})
    return b.getvalue()


def sample_tiffs():
    with Image.open(os.path.join(GOLDEN, "sample_0717_023_orig.jpg")) as im:
        rgb = im.convert("RGB")
    gray = rgb.convert("L")
    bw = gray.point(lambda v: 255 if v > 128 else 0).convert("1")
    return {
        "g4": tiff(bw, "group4"),
        "g4_one_strip": tiff(bw, "group4", t278=bw.size[1]),
        "packbits_bilevel": tiff(bw, "packbits"),
        "lzw_gray": tiff(gray, "tiff_lzw"),
        "lzw_rgb_predictor": tiff(rgb, "tiff_lzw", t317=2),
        "deflate_rgb": tiff(rgb, "tiff_adobe_deflate"),
        "raw_rgb": tiff(rgb, "raw"),
    }


def bench(kind, data, a, pool):
    dev = torch.device("cuda", 0)
    info, blob = PIO.tiff_inspect(data)
    assert info is not None, blob
    want = PIO._pillow_bgr(io.BytesIO(data))
    print("== %s: %dx%d, %d sample(s) of %d bit(s), compression %d, %d strip(s), file %d B, blob %d B, workspace %.1f MB per page" %
          (kind, info.width, info.height, info.components, info.bits, info.compression, info.strips, len(data), info.blob_bytes,
           info.workspace_bytes / 1e6))
    tmp = tempfile.mkdtemp(prefix="bench_decode_tiff_")
    paths = []
    for i in range(max(a.batches)):
        p = os.path.join(tmp, "page_%02d.tif" % i)
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
    wins = []
    for n in a.batches:
        sub = paths[:n]
        for _ in range(2):
            got = PIO.read_images_bgr(sub)
        torch.cuda.synchronize()
        assert np.array_equal(got[-1].cpu().numpy(), want), "%s: the device page differs from Pillow's" % kind

        def read_all():
            PIO.read_images_bgr(sub)
            torch.cuda.synchronize()
        d = stat(times_ms(read_all, a.iters))
        p1 = stat(times_ms(lambda: [PIO.read_image_bgr(p) for p in sub], max(2, a.iters // 2)))
        p16 = stat(times_ms(lambda: list(pool.map(PIO.read_image_bgr, sub)), max(2, a.iters // 2)))
        print("  %2d file(s): device %8.2f ms (%7.2f .. %7.2f)   Pillow x1 %8.2f ms (%7.2f .. %7.2f)   Pillow x16 %8.2f ms (%7.2f .. %7.2f)   %s" %
              ((n,) + d + p1 + p16 + ("device wins" if d[0] < p1[0] else "Pillow x1 wins",)))
        wins.append(d[0] < p1[0])
    n = max(a.batches)
    host = np.concatenate([blob] * n)
    offs = np.arange(n, dtype=np.int64) * blob.size
    dblobs = torch.from_numpy(host).to(dev)
    wsb = int(L.lib.rtn_tiff_decode_workspace_bytes(n, host.ctypes.data, offs.ctypes.data))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    pages = [torch.empty(info.height, info.width, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
    ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in pages])
    status = torch.empty(n, dtype=torch.int32, device=dev)
    h = L.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def decode():
        h.check(L.lib.rtn_tiff_decode(h.raw, n, host.ctypes.data, dblobs.data_ptr(), offs.ctypes.data, ptrs, status.data_ptr(), ws.data_ptr(), wsb))
    for _ in range(2):
        decode()
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0 and np.array_equal(pages[n - 1].cpu().numpy(), want)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    k_ms = []
    for _ in range(a.iters):
        ev[0].record()
        decode()
        ev[1].record()
        torch.cuda.synchronize()
        k_ms.append(ev[0].elapsed_time(ev[1]))
    out = np.empty(L.lib.rtn_tiff_blob_bound(len(data)), np.uint8)
    ti = L.TiffInfo()
    i_ms = stat(times_ms(lambda: L.lib.rtn_tiff_inspect(None, data, len(data), C.byref(ti), out.ctypes.data, out.size), max(a.iters, 5)))
    print("  kernels alone, %d pages: %.2f ms (%.2f .. %.2f); rtn_tiff_inspect per page: %.3f ms (%.3f .. %.3f)" % ((n,) + stat(k_ms) + i_ms))
    first = next((b for b, w, rest in ((b, w, wins[i:]) for i, (b, w) in enumerate(zip(a.batches, wins))) if all(rest)), None)
    print("  -> %s" % ("the device beats Pillow on one thread from %d file(s) on" % first if first else
                       "Pillow on one thread wins at every batch size measured"))
    h.close()
    shutil.rmtree(tmp, ignore_errors=True)
    return first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--batches", default="1,2,4,8,16")
    a = ap.parse_args()
    a.batches = [int(v) for v in a.batches.split(",")]
    os.environ["RTN_TIFF_MIN"] = "1"
    os.environ["RTN_TIFF_G4_ONE_STRIP"] = "1"
    files = sample_tiffs()
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    firsts = {}
    with ThreadPoolExecutor(16) as pool:
        for kind in a.kinds.split(","):
            firsts[kind] = bench(kind, files[kind], a, pool)
    print("first batch size at which the device wins, per kind: %s" % firsts)


if __name__ == "__main__":
    main()
