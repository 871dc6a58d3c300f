"""Measure scanned-PDF input (model/pdf.py, csrc/rtn_compose.hip) on sample-sized pages: the 2200x1712 sample page
(tests/golden/sample_0717_023_orig.jpg) as 16-page PDFs of four kinds:

  g4_one_strip     bilevel, what Pillow's Image.save(f, "PDF") writes for mode "1": CCITTFaxDecode, every page one strip
  g4_strips        the same pages from write_pages_pdf(tiff="g4"): one image XObject per 64 rows, stacked by cm
  dct_gray         8-bit gray, what Pillow writes for mode "L": DCTDecode
  flate_rgb_png15  R,G,B, FlateDecode with /Predictor 15 (the IDAT stream of Pillow's PNG of the page)

  python tools/bench_read_pdf.py [--iters 7] [--pages 16] [--batches 1,2,4,8,16]

For every kind it reports medians and the min..max spread over the iterations after a warm-up, between stream events around the call:
  (a) read_pdf_pages of the file held in memory (parse, wrap, inspect, one copy, decode, status read-back, compose where needed), with
      RTN_PDF_G4_MIN=1 so that one-strip Group 4 goes to the device from RTN_TIFF_MIN files on;
  (b) the host route for the same file: Pillow on the wrapped streams (pdf.memory_files) on one thread, plus the upload of the pages
      (the wrapping itself is not counted on either side's account but (a)'s);
for g4_one_strip at 1, 2, 4, 8 and 16 pages, to see where the serial decoder crosses Pillow (RTN_PDF_G4_MIN's default); and the compose
kernel alone on 16 resident pages under /Rotate 90 (every image turned a quarter, through the LDS tile), in GB/s written, next to a
plain device copy of the same bytes."""
import argparse
import importlib
import io
import os
import sys
import zlib

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "retinanet-for-table-detection_amd"
P = importlib.import_module(PKG + ".model.pdf")
PIO = importlib.import_module(PKG + ".model.page_io")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def stat(v):
    return (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def event_ms(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(iters):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    return stat(ts)


def pillow_pdf(im, n):
    f = io.BytesIO()
    im.save(f, "PDF", save_all=n > 1, append_images=[im] * (n - 1), resolution=300.0)
    return f.getvalue()


def flate_pdf(rgb, n):
    """n pages, each one FlateDecode image with /Predictor 15 whose stream is the IDAT stream of Pillow's PNG of the page."""
    f = io.BytesIO()
    rgb.save(f, "PNG")
    png, pos, idat = f.getvalue(), 8, b""
    while pos < len(png):
        size = int.from_bytes(png[pos:pos + 4], "big")
        if png[pos + 4:pos + 8] == b"IDAT":
            idat += png[pos + 8:pos + 8 + size]
        pos += 12 + size
    w, h = rgb.size
    unit = 72.0 / 300.0
    objs = ["<< /Type /Catalog /Pages 2 0 R >>".encode(), None]
    kids = []
    for _ in range(n):
        first = len(objs) + 1
        kids.append(first)
        content = ("q %.4f 0 0 %.4f 0 0 cm /Im0 Do Q" % (w * unit, h * unit)).encode()
        objs.append(("<< /Type /Page /Parent 2 0 R /MediaBox [0 0 %.4f %.4f] /Resources << /XObject << /Im0 %d 0 R >> >> /Contents %d 0 R >>"
                     % (w * unit, h * unit, first + 2, first + 1)).encode())
        objs.append(b"<< /Length %d >>\nstream\n" % len(content) + content + b"\nendstream")
        objs.append(("<< /Type /XObject /Subtype /Image /Width %d /Height %d /ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /FlateDecode "
                     "/DecodeParms << /Predictor 15 /Colors 3 /Columns %d >> /Length %d >>\nstream\n" % (w, h, w, len(idat))).encode() + idat + b"\nendstream")
    objs[1] = ("<< /Type /Pages /Count %d /Kids [%s] >>" % (n, " ".join("%d 0 R" % k for k in kids))).encode()
    out, offsets = bytearray(b"%PDF-1.4\n"), []
    for k, body in enumerate(objs):
        offsets.append(len(out))
        out += b"%d 0 obj\n" % (k + 1) + body + b"\nendobj\n"
    at = len(out)
    out += b"xref\n0 %d\n0000000000 65535 f \n" % (len(objs) + 1) + b"".join(b"%010d 00000 n \n" % o for o in offsets)
    out += b"trailer\n<< /Size %d /Root 1 0 R >>\nstartxref\n%d\n%%%%EOF\n" % (len(objs) + 1, at)
    return bytes(out)


def compare(kind, data, iters):
    files = [f for page in P.memory_files(data) for f in page]
    want = P.read_pdf_pages_host(data)
    got, info = P.read_pdf_pages(data, return_info=True)
    torch.cuda.synchronize()
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)), "%s: the device pages differ from the host route's" % kind
    routes = sorted({im.route for p in info.pages for im in p.images})
    d = event_ms(lambda: P.read_pdf_pages(data), iters)
    hst = event_ms(lambda: [torch.from_numpy(PIO._pillow_bgr(io.BytesIO(f))).cuda() for f in files], max(2, iters // 2), warm=1)
    print("  %-16s %2d page(s), %3d image(s), file %8d B, decoded on: %s" % (kind, len(got), len(files), len(data), "/".join(routes)))
    print("      read_pdf_pages %8.2f ms (%7.2f .. %7.2f)   Pillow x1 on the wrapped streams + upload %8.2f ms (%7.2f .. %7.2f)   %s"
          % (d + hst + ("device wins" if d[0] < hst[0] else "host wins",)))
    return d[0] < hst[0]


def compose_alone(pages, iters):
    dev = pages[0].device
    h = PIO.L.Handle(dev.index or 0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    jobs = []
    for p in pages:
        H, W = int(p.shape[0]), int(p.shape[1])
        jobs.append((torch.empty(W, H, 3, dtype=torch.uint8, device=dev), [(p, 6, False, 0, 0, 0, 0, H, W)]))
    t = event_ms(lambda: P._compose(dev, h, jobs), iters)
    assert np.array_equal(jobs[0][0].cpu().numpy(), np.rot90(pages[0].cpu().numpy(), -1))
    nbytes = sum(p.numel() for p in pages)
    src, dst = torch.cat([p.reshape(-1) for p in pages]), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    c = event_ms(lambda: dst.copy_(src), iters)
    print("  compose alone, /Rotate 90, %d resident pages of %d x %d: %.3f ms (%.3f .. %.3f) = %.1f GB/s written (table upload and launch included)"
          % ((len(pages), pages[0].shape[1], pages[0].shape[0]) + t + (nbytes / t[0] / 1e6,)))
    print("  a plain device copy of the same %d bytes: %.3f ms (%.3f .. %.3f) = %.1f GB/s written" % ((nbytes,) + c + (nbytes / c[0] / 1e6,)))
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--batches", default="1,2,4,8,16")
    a = ap.parse_args()
    os.environ["RTN_PDF_G4_MIN"] = "1"
    with Image.open(os.path.join(GOLDEN, "sample_0717_023_orig.jpg")) as im:
        rgb = im.convert("RGB")
    gray = rgb.convert("L")
    bw = gray.point(lambda v: 255 if v > 128 else 0).convert("1")
    n = a.pages
    print("device: %s; torch %s; page %d x %d; zlib %s" % (torch.cuda.get_device_name(0), torch.__version__, rgb.size[0], rgb.size[1], zlib.ZLIB_VERSION))
    page = torch.from_numpy(np.array(gray)).cuda()
    kinds = {
        "g4_one_strip": pillow_pdf(bw, n),
        "g4_strips": P.write_pages_pdf(None, [page] * n, tiff="g4"),
        "dct_gray": pillow_pdf(gray, n),
        "flate_rgb_png15": flate_pdf(rgb, n),
    }
    print("== %d pages per file" % n)
    for kind, data in kinds.items():
        compare(kind, data, a.iters)
    print("== g4_one_strip by batch (RTN_PDF_G4_MIN=1: the device takes every batch that RTN_TIFF_MIN lets through)")
    wins = []
    for b in [int(v) for v in a.batches.split(",")]:
        wins.append((b, compare("g4_one_strip", pillow_pdf(bw, b), a.iters)))
    first = next((b for i, (b, w) in enumerate(wins) if all(x for _b, x in wins[i:])), None)
    print("  -> %s" % ("the device beats the host route from %d page(s) on" % first if first else "the host route wins at every batch measured"))
    print("== the compose kernel")
    compose_alone([torch.from_numpy(np.ascontiguousarray(np.asarray(rgb)[:, :, ::-1])).cuda() for _ in range(n)], a.iters)


if __name__ == "__main__":
    main()
