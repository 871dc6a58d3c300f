"""Measure the device PNG decoder (csrc/rtn_png_dec.hip) on sample-sized pages: the 2200x1712 distance map
(tests/golden/sample_0717_023.jpg, the file a training run reads), the page itself, or the gray page, written 16 times as PNG of
the chunked layout by the device encoder (model.page_io.encode_png_bgr).

  python tools/bench_decode_png.py [--batch 16] [--iters 10] [--host-pages 4] [--content map|page|gray|all]

Reports medians and the min..max spread over the iterations after a warm-up, every path on the same machine:
  (a) GPU time of the four decode kernels per batch (events around rtn_png_decode, blobs already on the device);
  (b) host time of rtn_png_inspect per page (parse and copy of the deflate payloads; the chunk CRCs are left to the device);
  (c) wall time of read_images_bgr for the batch's files (read, inspect, one copy, decode, status read-back);
  (d) read_image_bgr (Pillow) on one thread on the same files: the parent commit's path for them;
  (e) one CSVGenerator batch of those files end to end, with the device decoder and with every page decoded by read_image_bgr.
For the per-kernel split: rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -o png_dec --
  python tools/bench_decode_png.py --iters 3 --host-pages 0 --content map

  python tools/bench_decode_png.py --stream [--iters 10] [--content map|page|gray|all] [--segments 16384,65536,262144]

measures the stream PNG decoder (csrc/rtn_png_stream.hip) instead, on the same pages saved 16 times by Pillow with
default settings: read_images_bgr with RTN_PNG_STREAM_MIN=1 at batch sizes 1, 2, 4, 8 and 16 for every RTN_PNG_SEGMENT value asked
for, the decode kernels alone at batch 16, and the yardsticks on the same files: read_image_bgr (Pillow) on one thread, which is
what read_images_bgr does with these files without the device path, and the same decode spread over 16 host threads.

  python tools/bench_decode_png.py --layout [--iters 10] [--kinds gray1,palette16,rgba,interlaced_rgb]

measures the pixel-layout decoder (DESIGN §3.4f "Pixel layouts") on 16 copies of the sample page as 1-bit gray, 16-colour palette,
R,G,B,A and Adam7 R,G,B files: see bench_layout.  For the per-kernel split: rocprofv3 --kernel-trace --stats --output-format csv
-d rocprof_out -o png_layout -- python tools/bench_decode_png.py --layout --iters 3
"""
import argparse
import ctypes as C
import importlib
import json
import os
import shutil
import sys
import tempfile
import time
import warnings

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "retinanet-for-table-detection_amd"
CG = importlib.import_module(PKG + ".csv_generator")
L = importlib.import_module(PKG + "._lib")
PIO = importlib.import_module(PKG + ".model.page_io")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def stat(v):
    return (float(np.median(v)), float(np.min(v)), float(np.max(v))) if len(v) else (float("nan"),) * 3


def times_ms(fn, iters):
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def load(content):
    if content == "map":
        return np.ascontiguousarray(np.asarray(Image.open(os.path.join(GOLDEN, "sample_0717_023.jpg")).convert("RGB"))[:, :, ::-1])
    o = Image.open(os.path.join(GOLDEN, "sample_0717_023_orig.jpg"))
    if content == "page":
        return np.ascontiguousarray(np.asarray(o.convert("RGB"))[:, :, ::-1])
    return np.ascontiguousarray(np.asarray(o.convert("L")))


def bench(content, a):
    n = a.batch
    dev = torch.device("cuda", 0)
    page = load(content)
    (data,) = PIO.encode_png_bgr([page])
    want = page if page.ndim == 3 else np.repeat(page[:, :, None], 3, axis=2)
    tmp = tempfile.mkdtemp(prefix="bench_decode_png_")
    paths = []
    for i in range(n):
        p = os.path.join(tmp, "page_%02d.png" % i)
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
    info, blob = PIO.png_inspect(data)
    assert info is not None, blob
    print("== %s: %dx%d, %d component(s), file %d B, %d chunks, deflate payload %d B, blob %d B, workspace %.1f MB per page" %
          (content, info.width, info.height, info.components, len(data), info.chunks, info.payload_bytes, info.blob_bytes,
           info.workspace_bytes / 1e6))

    # (a) kernels alone
    host = np.concatenate([blob] * n)
    offs = np.arange(n, dtype=np.int64) * blob.size
    dblobs = torch.from_numpy(host).to(dev)
    wsb = int(L.lib.rtn_png_decode_workspace_bytes(n, host.ctypes.data, offs.ctypes.data))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    pages = [torch.empty(info.height, info.width, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
    ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in pages])
    status = torch.empty(n, dtype=torch.int32, device=dev)
    h = L.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def decode():
        h.check(L.lib.rtn_png_decode(h.raw, n, host.ctypes.data, dblobs.data_ptr(), offs.ctypes.data, ptrs, status.data_ptr(),
                                     ws.data_ptr(), wsb))
    for _ in range(3):
        decode()
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    assert np.array_equal(pages[n - 1].cpu().numpy(), want)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    k_ms = []
    for _ in range(a.iters):
        ev[0].record()
        decode()
        ev[1].record()
        torch.cuda.synchronize()
        k_ms.append(ev[0].elapsed_time(ev[1]))

    # (b) host inspect, per page
    out = np.empty(L.png_blob_bound(len(data)), np.uint8)
    pinfo = L.PngInfo()
    i_ms = times_ms(lambda: L.lib.rtn_png_inspect(None, data, len(data), C.byref(pinfo), out.ctypes.data, out.size), max(a.iters, 5))

    # (c) read_images_bgr, files to device pages
    for _ in range(2):
        got = PIO.read_images_bgr(paths)
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), want)

    def read_all():
        PIO.read_images_bgr(paths)
        torch.cuda.synchronize()
    r_ms = times_ms(read_all, a.iters)

    # (d) Pillow, one thread
    p_ms = []
    if a.host_pages:
        PIO.read_image_bgr(paths[0])
        p_ms = times_ms(lambda: PIO.read_image_bgr(paths[0]), a.host_pages)

    # (e) one CSVGenerator batch from the files
    csvf = os.path.join(tmp, "train.csv")
    with open(csvf, "w") as f:
        f.write("image_id,xmin,ymin,xmax,ymax,label\n")
        for p in paths:
            f.write("%s,100,120,900,700,table\n" % os.path.basename(p))

    def gen_ms(device_decode, iters):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gen = CG.CSVGenerator(csvf, tmp, {"table": 0}, batch_size=n, group_method="none", shuffle_groups=False)
            if not device_decode:
                gen.load_image_group = lambda group: CG.Generator.load_image_group(gen, group)
            keep = []

            def one():
                x, (reg, lab) = gen[0]
                torch.cuda.current_stream(dev).synchronize()
                keep.append(x)
            one()
            ms = times_ms(one, iters)
            gen.close()
        return ms, keep[-1]
    g_ms, x_dev = gen_ms(True, a.iters)
    gh_ms = []
    if a.host_pages:
        gh_ms, x_host = gen_ms(False, 1)
        assert torch.equal(x_dev, x_host)

    res = {"content": content, "batch": n, "file_bytes": len(data)}
    for key, label, v, per in (("kernels_ms", "(a) decode kernels alone", k_ms, n),
                               ("inspect_ms_per_page", "(b) rtn_png_inspect on the host", i_ms, 1),
                               ("read_images_bgr_ms", "(c) read_images_bgr", r_ms, n),
                               ("pillow_ms_per_page", "(d) read_image_bgr (Pillow), one thread", p_ms, 1),
                               ("generator_batch_ms_device", "(e) CSVGenerator batch, device decoder", g_ms, n),
                               ("generator_batch_ms_pillow", "(e) CSVGenerator batch, read_image_bgr", gh_ms, n)):
        m, lo, hi = stat(v)
        print("%-44s %9.3f ms per %2d page(s) (min %.3f, max %.3f, %d runs): %.1f pages/s" % (label, m, per, lo, hi, len(v), per / m * 1e3))
        res[key] = round(m, 3)
    if p_ms:
        print("(c) is %.0fx (d); the training step that has to hide (c) takes 25.9 ms" % (stat(p_ms)[0] * n / stat(r_ms)[0]))
    print(json.dumps(res))
    h.close()
    shutil.rmtree(tmp, ignore_errors=True)


def bench_stream(content, a):
    from concurrent.futures import ThreadPoolExecutor
    dev = torch.device("cuda", 0)
    page = load(content)
    want = page if page.ndim == 3 else np.repeat(page[:, :, None], 3, axis=2)
    tmp = tempfile.mkdtemp(prefix="bench_decode_png_stream_")
    paths = []
    for i in range(16):
        p = os.path.join(tmp, "page_%02d.png" % i)
        if i == 0:
            PIO.write_image(p, page)
        else:
            shutil.copy(paths[0], p)
        paths.append(p)
    data = open(paths[0], "rb").read()
    res = {"content": content, "file_bytes": len(data)}

    def line(key, label, v, per):
        m, lo, hi = stat(v)
        print("%-58s %9.3f ms per %2d page(s) (min %.3f, max %.3f, %d runs): %.1f pages/s" % (label, m, per, lo, hi, len(v), per / m * 1e3))
        res[key] = round(m, 3)
        return m

    os.environ["RTN_PNG_STREAM_MIN"] = "0"
    PIO.read_image_bgr(paths[0])
    one = line("pillow_ms_per_page", "read_image_bgr (Pillow), one thread", times_ms(lambda: PIO.read_image_bgr(paths[0]), a.iters), 1)
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(PIO.read_image_bgr, paths))
        line("pillow_16_threads_ms", "read_image_bgr (Pillow), 16 threads", times_ms(lambda: list(pool.map(PIO.read_image_bgr, paths)), a.iters), 16)

    def read_n(n):
        PIO.read_images_bgr(paths[:n])
        torch.cuda.synchronize()
    read_n(16)
    line("parent_read_images_bgr_ms", "read_images_bgr, device path off (the parent's path)", times_ms(lambda: read_n(16), max(2, a.iters // 3)), 16)
    os.environ["RTN_PNG_STREAM_MIN"] = "1"
    for seg in a.segments:
        os.environ["RTN_PNG_SEGMENT"] = str(seg)
        info, blob = PIO.png_stream_inspect(data)
        assert info is not None, blob
        print("== %s, RTN_PNG_SEGMENT=%d: %dx%d, %d component(s), file %d B, %d segments, blob %d B, workspace %.1f MB per page" %
              (content, seg, info.width, info.height, info.components, len(data), info.chunks, info.blob_bytes, info.workspace_bytes / 1e6))
        got, words = PIO.decode_png_bgr([data], return_status=True)
        assert words == [0] and np.array_equal(got[0].cpu().numpy(), want)
        for n in (1, 2, 4, 8, 16):
            read_n(n)
            m = line("read_images_bgr_ms_S%d_B%d" % (seg, n), "read_images_bgr, device path, batch %d" % n, times_ms(lambda: read_n(n), a.iters), n)
            print("    %.2fx the one-thread Pillow decode of the same files" % (one * n / m))
        # the kernels alone, batch 16
        n = 16
        host = np.concatenate([blob] * n)
        offs = np.arange(n, dtype=np.int64) * blob.size
        dblobs = torch.from_numpy(host).to(dev)
        wsb = int(L.lib.rtn_png_stream_decode_workspace_bytes(n, host.ctypes.data, offs.ctypes.data))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        pages = [torch.empty(info.height, info.width, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in pages])
        status = torch.empty(n, dtype=torch.int32, device=dev)
        h = L.Handle(0)
        h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        k_ms = []
        for it in range(a.iters + 2):
            ev[0].record()
            h.check(L.lib.rtn_png_stream_decode(h.raw, n, host.ctypes.data, dblobs.data_ptr(), offs.ctypes.data, ptrs, status.data_ptr(),
                                                ws.data_ptr(), wsb))
            ev[1].record()
            torch.cuda.synchronize()
            if it >= 2:
                k_ms.append(ev[0].elapsed_time(ev[1]))
        assert int(status.abs().sum()) == 0 and np.array_equal(pages[n - 1].cpu().numpy(), want)
        line("kernels_ms_S%d" % seg, "decode kernels alone, batch 16", k_ms, n)
        pinfo = L.PngInfo()
        out = np.empty(L.png_blob_bound(len(data)), np.uint8)
        line("inspect_ms_per_page_S%d" % seg, "rtn_png_stream_inspect on the host",
             times_ms(lambda: L.lib.rtn_png_stream_inspect(None, data, len(data), C.byref(pinfo), out.ctypes.data, out.size), max(a.iters, 5)), 1)
        h.close()
    print(json.dumps(res))
    shutil.rmtree(tmp, ignore_errors=True)


def interlaced_rgb_png(rgb):
    """An Adam7 R,G,B file of the page (Pillow writes none): filter Sub on every row of every pass, zlib level 6."""
    import struct
    import zlib

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)
    h, w = rgb.shape[:2]
    raw = []
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = rgb[y0::dy, x0::dx].astype(np.int16)
        if sub.size == 0:
            continue
        left = np.zeros_like(sub)
        left[:, 1:] = sub[:, :-1]
        rows = np.empty((sub.shape[0], 1 + 3 * sub.shape[1]), np.uint8)
        rows[:, 0] = 1
        rows[:, 1:] = ((sub - left) & 255).reshape(sub.shape[0], -1)
        raw.append(rows.tobytes())
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 1)) +
            chunk(b"IDAT", zlib.compress(b"".join(raw), 6)) + chunk(b"IEND", b""))


def bench_layout(a):
    """--layout: the pixel layouts of DESIGN §3.4f "Pixel layouts" on 16 copies of the sample page in four forms: 1-bit gray,
    16-colour palette, R,G,B,A (all written by Pillow) and Adam7 R,G,B.  decode_png_bgr with RTN_PNG_LAYOUT_MIN=1 at batch sizes 1, 2,
    4, 8 and 16 against Pillow on one thread and on 16 threads in the same run, and the decode kernels alone at batch 16."""
    import io
    from concurrent.futures import ThreadPoolExecutor
    dev = torch.device("cuda", 0)
    o = Image.open(os.path.join(GOLDEN, "sample_0717_023_orig.jpg"))

    def png(img):
        b = io.BytesIO()
        img.save(b, "PNG")
        return b.getvalue()
    kinds = {"gray1": lambda: png(o.convert("L").convert("1")), "palette16": lambda: png(o.convert("RGB").quantize(16)),
             "rgba": lambda: png(o.convert("RGBA")), "interlaced_rgb": lambda: interlaced_rgb_png(np.asarray(o.convert("RGB")))}
    res = {}
    wins = {}
    for kind in a.kinds:
        data = kinds[kind]()
        files = [data] * 16
        want = PIO._pillow_bgr(io.BytesIO(data))

        def line(key, label, v, per):
            m, lo, hi = stat(v)
            print("%-58s %9.3f ms per %2d page(s) (min %.3f, max %.3f, %d runs): %.1f pages/s" % (label, m, per, lo, hi, len(v), per / m * 1e3))
            res[kind + "_" + key] = round(m, 3)
            return m
        info, blob = PIO.png_layout_inspect(data)
        assert info is not None, blob
        print("== %s: %dx%d, depth %d, colour type %d, interlace %d, file %d B, %d segments, blob %d B, workspace %.1f MB per page" %
              (kind, info.width, info.height, data[24], data[25], data[28], len(data), info.chunks, info.blob_bytes, info.workspace_bytes / 1e6))

        def pillow(d):
            return PIO._pillow_bgr(io.BytesIO(d))
        one = line("pillow_ms_per_page", "Pillow from memory, one thread", times_ms(lambda: pillow(data), a.iters), 1)
        with ThreadPoolExecutor(16) as pool:
            list(pool.map(pillow, files))
            line("pillow_16_threads_ms", "Pillow from memory, 16 threads", times_ms(lambda: list(pool.map(pillow, files)), a.iters), 16)
        os.environ["RTN_PNG_LAYOUT_MIN"] = "0"

        def read_n(n):
            PIO.decode_png_bgr(files[:n])
            torch.cuda.synchronize()
        read_n(16)
        line("host_path_ms", "decode_png_bgr, device path off (Pillow, then upload)", times_ms(lambda: read_n(16), max(2, a.iters // 3)), 16)
        os.environ["RTN_PNG_LAYOUT_MIN"] = "1"
        got, words = PIO.decode_png_bgr([data], return_status=True)
        assert words == [0] and np.array_equal(got[0].cpu().numpy(), want)
        for n in (1, 2, 4, 8, 16):
            read_n(n)
            m = line("decode_png_bgr_ms_B%d" % n, "decode_png_bgr, device path, batch %d" % n, times_ms(lambda: read_n(n), a.iters), n)
            print("    %.2fx the one-thread Pillow decode of the same files" % (one * n / m))
            if one * n / m > 1.0:
                wins.setdefault(kind, n)
        n = 16
        host = np.concatenate([blob] * n)
        offs = np.arange(n, dtype=np.int64) * blob.size
        dblobs = torch.from_numpy(host).to(dev)
        wsb = int(L.lib.rtn_png_layout_decode_workspace_bytes(n, host.ctypes.data, offs.ctypes.data))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        pages = [torch.empty(info.height, info.width, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in pages])
        status = torch.empty(n, dtype=torch.int32, device=dev)
        h = L.Handle(0)
        h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        k_ms = []
        for it in range(a.iters + 2):
            ev[0].record()
            h.check(L.lib.rtn_png_layout_decode(h.raw, n, host.ctypes.data, dblobs.data_ptr(), offs.ctypes.data, ptrs, status.data_ptr(),
                                                ws.data_ptr(), wsb))
            ev[1].record()
            torch.cuda.synchronize()
            if it >= 2:
                k_ms.append(ev[0].elapsed_time(ev[1]))
        assert int(status.abs().sum()) == 0 and np.array_equal(pages[n - 1].cpu().numpy(), want)
        line("kernels_ms", "decode kernels alone, batch 16", k_ms, n)
        pinfo = L.PngInfo()
        out = np.empty(int(L.lib.rtn_png_layout_blob_bound(len(data))), np.uint8)
        line("inspect_ms_per_page", "rtn_png_layout_inspect on the host",
             times_ms(lambda: L.lib.rtn_png_layout_inspect(None, data, len(data), C.byref(pinfo), out.ctypes.data, out.size), max(a.iters, 5)), 1)
        h.close()
    res["smallest_winning_batch"] = {k: wins.get(k) for k in a.kinds}
    print("smallest batch at which the device beats Pillow on one thread, per kind: %s" % res["smallest_winning_batch"])
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-pages", type=int, default=4)
    ap.add_argument("--content", choices=("map", "page", "gray", "all"), default="all")
    ap.add_argument("--stream", action="store_true", help="measure the stream PNG decoder on Pillow-written files")
    ap.add_argument("--segments", type=lambda v: [int(x) for x in v.split(",")], default=[16384], help="RTN_PNG_SEGMENT values (--stream)")
    ap.add_argument("--layout", action="store_true", help="measure the pixel-layout decoder on the sample page in four forms")
    ap.add_argument("--kinds", type=lambda v: v.split(","), default=["gray1", "palette16", "rgba", "interlaced_rgb"], help="forms (--layout)")
    a = ap.parse_args()
    if a.layout:
        return bench_layout(a)
    for content in (("map", "page", "gray") if a.content == "all" else (a.content,)):
        (bench_stream if a.stream else bench)(content, a)


if __name__ == "__main__":
    main()
