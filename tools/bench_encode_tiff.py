"""Measure the device Group 4 TIFF encoder (csrc/rtn_tiff_enc.hip) on sample-sized pages: 16 copies of the 2200x1712
sample page (tests/golden/sample_0717_023_orig.jpg) as a gray page thresholded at 128, the bilevel page of tests/tiff_ref.sample_tiffs.

  python tools/bench_encode_tiff.py [--iters 10] [--pages 16] [--out profiles/tiff_encode_bench.txt]

It reports medians and the min..max spread over the iterations after a warm-up, every path on the same machine and the same pages:
  (a) wall time of encode_tiff_bgr from CUDA tensors (six kernels, the lengths' copy, one copy of the files to the host) and from host
      arrays (the upload as well);
  (b) Image.fromarray(page >= 128).save(f, "TIFF", compression="group4") on one thread and spread over 16 threads (Pillow's default
      photometric, BlackIsZero), and on one thread with tiffinfo={262: 0}, the device's default, which takes Pillow another path;
  (c) the GPU time of the kernels alone (events around rtn_tiff_encode), with a lane per row (RTN_TIFF_ENC_WAVE_ROW=0) and with a wave
      per row (RTN_TIFF_ENC_WAVE_ROW=1), the two taking turns, on the sample pages and on pages of noise at 50% ink (the most codes
      a page can need: rows that share no edge);
  (d) decode_tiff_bgr of the files written (64 rows per strip: one wave per strip), of Pillow's files of the same pages (its default
      strips) and Pillow's own decode of either on one thread;
  (e) the file sizes at 64 rows per strip against Pillow's default strips and against one strip.
The lines go to stdout and to --out.  For the per-kernel split: rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out
-o tiff_enc -- python tools/bench_encode_tiff.py --iters 3
"""
import argparse
import ctypes as C
import importlib
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "retinanet-for-table-detection_amd"
L = importlib.import_module(PKG + "._lib")
PIO = importlib.import_module(PKG + ".model.page_io")
GOLDEN = os.path.join(ROOT, "tests", "golden")
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def stat(v):
    return (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def times_ms(fn, iters):
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def sample_page():
    """The sample page as uint8 gray of 0 / 255: ink where the page's gray is at most 128 (tests/tiff_ref.sample_tiffs)."""
    with Image.open(os.path.join(GOLDEN, "sample_0717_023_orig.jpg")) as im:
        gray = im.convert("RGB").convert("L")
    return np.ascontiguousarray(np.asarray(gray.point(lambda v: 255 if v > 128 else 0)))


def pillow_g4(page, **tiffinfo):
    """Pillow's Group 4 file of a page; without t262 its default for mode "1", BlackIsZero, which is also its fastest path."""
    b = io.BytesIO()
    Image.fromarray(page >= 128).save(b, "TIFF", compression="group4", tiffinfo={int(k[1:]): v for k, v in tiffinfo.items()})
    return b.getvalue()


def kernels_ms(pages, iters):
    """GPU time of rtn_tiff_encode alone over the pages (CUDA tensors), per variant, the variants taking turns: {name: [ms]}."""
    n = len(pages)
    H, W = pages[0].shape
    Wa, Ha, Ca = (np.full(n, v, np.int32) for v in (W, H, 1))
    Ta, Ra, Pa = (np.full(n, v, np.int32) for v in (128, PIO.TIFF_ROWS_PER_STRIP, 0))
    bound = int(L.lib.rtn_tiff_encode_bound(W, H, PIO.TIFF_ROWS_PER_STRIP))
    slot = (bound + 255) & ~255
    offs = np.arange(n + 1, dtype=np.int64) * slot
    out = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
    nb = torch.empty(n, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    wsb = int(L.lib.rtn_tiff_encode_workspace_bytes(n, Wa.ctypes.data, Ha.ctypes.data, Ca.ctypes.data, Ra.ctypes.data))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in pages])
    h = L.Handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)

    def run():
        h.check(L.lib.rtn_tiff_encode(h.raw, n, ptrs, Wa.ctypes.data, Ha.ctypes.data, Ca.ctypes.data, Ta.ctypes.data, Ra.ctypes.data,
                                      Pa.ctypes.data, out.data_ptr(), offs.ctypes.data, nb.data_ptr(), status.data_ptr(), ws.data_ptr(), wsb))
    variants = (("lane per row", "0"), ("wave per row", "1"))
    res, files = {name: [] for name, _ in variants}, {}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for it in range(iters + 2):
        for name, flag in variants:
            os.environ["RTN_TIFF_ENC_WAVE_ROW"] = flag
            ev[0].record()
            run()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= 2:
                res[name].append(ev[0].elapsed_time(ev[1]))
            files[name] = bytes(out[:int(nb[0])].cpu().numpy())
    os.environ.pop("RTN_TIFF_ENC_WAVE_ROW")
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0 and files["lane per row"] == files["wave per row"]
    h.close()
    return res, wsb, bound, files["lane per row"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiff_encode_bench.txt"))
    a = ap.parse_args()
    os.environ["RTN_TIFF_MIN"] = "1"
    page = sample_page()
    H, W = page.shape
    n = a.pages
    host = [page.copy() for _ in range(n)]
    dev = [torch.from_numpy(p).cuda() for p in host]
    say("device: %s; torch %s; Pillow %s" % (torch.cuda.get_device_name(0), torch.__version__, PIL.__version__))
    say("workload: %d pages of %dx%d, gray thresholded at 128 (%.1f%% ink), Group 4, WhiteIsZero" % (n, H, W, 100.0 * float((page < 128).mean())))

    for _ in range(2):
        files = PIO.encode_tiff_bgr(dev)
    ref = pillow_g4(page, t262=0, t278=PIO.TIFF_ROWS_PER_STRIP)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tiff_encode_ref as R
    assert R.strips_of(files[0]) == R.strips_of(ref) and files.count(files[0]) == n, "the device's strips are not Pillow's"

    def dev_encode(src):
        def fn():
            PIO.encode_tiff_bgr(src)
            torch.cuda.synchronize()
        return fn
    d_cuda = stat(times_ms(dev_encode(dev), a.iters))
    d_host = stat(times_ms(dev_encode(host), a.iters))
    with ThreadPoolExecutor(16) as pool:
        p1 = stat(times_ms(lambda: [pillow_g4(p) for p in host], max(2, a.iters // 2)))
        p16 = stat(times_ms(lambda: list(pool.map(pillow_g4, host)), max(2, a.iters // 2)))
    p0 = stat(times_ms(lambda: [pillow_g4(p, t262=0) for p in host], 2))
    say("encode, %d pages, wall time, median (min .. max) of %d:" % (n, a.iters))
    say("  encode_tiff_bgr from CUDA tensors   %8.2f ms (%7.2f .. %7.2f)" % d_cuda)
    say("  encode_tiff_bgr from host arrays    %8.2f ms (%7.2f .. %7.2f)" % d_host)
    say("  Pillow group4, one thread           %8.2f ms (%7.2f .. %7.2f)" % p1)
    say("  Pillow group4, 16 threads           %8.2f ms (%7.2f .. %7.2f)" % p16)
    say("  Pillow group4, WhiteIsZero, 1 thread%8.2f ms (%7.2f .. %7.2f)   (2 iterations)" % p0)
    say("  -> from CUDA tensors the device %s Pillow on one thread and %s Pillow on 16 threads" %
        ("beats" if d_cuda[0] < p1[0] else "loses to", "beats" if d_cuda[0] < p16[0] else "loses to"))

    noise = torch.from_numpy(np.where(np.random.RandomState(0).random_sample((H, W)) < 0.5, 0, 255).astype(np.uint8)).cuda()
    for what, pages, want in (("the sample pages", dev, files[0]), ("pages of noise, 50% ink", [noise] * n, None)):
        k, wsb, bound, one = kernels_ms(pages, a.iters)
        assert want is None or one == want
        say("kernels alone (events around rtn_tiff_encode), %d x %s, file %d B; workspace %.1f MB, output slots %.1f MB (bound %d B per page):" %
            (n, what, len(one), wsb / 1e6, n * bound / 1e6, bound))
        for name in k:
            say("  %s                        %8.3f ms (%7.3f .. %7.3f)" % ((name,) + stat(k[name])))
        lane, wave = stat(k["lane per row"])[0], stat(k["wave per row"])[0]
        say("  -> %s is faster, %.2fx; pixels in: %.1f MB, at the faster time %.1f GB/s of page bytes" %
            ((("a lane per row", wave / lane) if lane <= wave else ("a wave per row", lane / wave)) + (n * H * W / 1e6, n * H * W / 1e6 / min(lane, wave))))

    default = pillow_g4(page, t262=0)
    one_strip = pillow_g4(page, t262=0, t278=H)
    for name, data in (("device files, 64 rows per strip", files[0]), ("Pillow files, default strips", default)):
        batch = [data] * n
        for _ in range(2):
            pages, st = PIO.decode_tiff_bgr(batch, return_status=True)
        assert st == [0] * n and np.array_equal(pages[-1].cpu().numpy()[:, :, 0], page)

        def dec():
            PIO.decode_tiff_bgr(batch)
            torch.cuda.synchronize()
        d = stat(times_ms(dec, a.iters))
        p = stat(times_ms(lambda: [PIO._pillow_bgr(io.BytesIO(f)) for f in batch], max(2, a.iters // 2)))
        say("decode, %d x %s (%d strips): decode_tiff_bgr %8.2f ms (%7.2f .. %7.2f)   Pillow, one thread %8.2f ms (%7.2f .. %7.2f)" %
            ((n, name, PIO.tiff_inspect(data)[0].strips) + d + p))
    say("file size, WhiteIsZero: device, 64 rows per strip %d B; Pillow, 64 rows per strip %d B; Pillow, default strips %d B; Pillow, one strip %d B"
        % (len(files[0]), len(ref), len(default), len(one_strip)))
    say("file size, BlackIsZero: Pillow, default strips %d B" % len(pillow_g4(page)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
