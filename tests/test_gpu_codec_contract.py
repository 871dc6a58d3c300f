"""The argument contract of the eight device entries of the page codecs (rtn_jpeg_decode, rtn_png_decode, rtn_png_stream_decode,
rtn_png_layout_decode, rtn_tiff_decode, rtn_jpeg_encode, rtn_png_encode, rtn_tiff_encode) and of their eight *_workspace_bytes
functions, each on the smallest page it accepts (8 x 8 gray; the layout decoder's is an 8 x 8 palette page).  No refusal launches a
kernel, so the device blobs of the decoder cases are never read:
  (a) n = -1: RTN_EINVAL, "n < 0"; n = 0 with every pointer null: RTN_OK;
  (b) each pointer argument null in turn: RTN_EINVAL, "NULL argument";
  (c) workspace + 16, and for the decoders dev_blobs + 8: RTN_EINVAL, "aligned";
  (d) decoders: offsets[0] = 8 and -16 ("offset not 16-byte aligned"), a blob whose first header word is overwritten ("blob 0 is not
      an <inspector> blob"), pages[0] = NULL ("page 0 is NULL");
  (e) encoders: 2 components, pages[0] = NULL, an output slot one byte under the bound (PNG, TIFF: the message names *_encode_bound),
      a reversed slot (JPEG: "[a, b)"), and for TIFF a slot that is not 4-byte aligned, threshold 0 and photometric 2;
  (f) workspace_bytes = need - 1: RTN_ENOMEM with both numbers in the text;
  (g) after every refusal the pages or files, status and out_bytes still hold the pattern they were filled with;
  (h) the order of the checks: a misaligned workspace together with a bad blob (page argument) 1 reports the alignment, a null page
      0 together with a bad blob (page argument) 1 reports page 0;
  (i) every *_workspace_bytes function: 0 for n = 0, for a null table, for a bad blob or page argument and for a negative offset;
      the sum of the inspectors' workspace_bytes (of the single-page answers) for a three-page call of two sizes.  For
      rtn_jpeg_workspace_bytes and rtn_png_decode_workspace_bytes, which read the header before they look at the offset's sign
      where this file was written, the negative offset points at zeros inside the allocation: the answer, 0, is what is pinned;
  (j) the second launch of the batch loop: 33 pages of two alternating sizes per entry through model/page_io.py, every page or
      file equal to Pillow's or the host twin's, every status word 0, pages 31 and 32 asserted by name.
The file was written against the eight entries as they stood before csrc/rtn_codec_launch.h existed, each with its own copy of
the prologue and the batch loop, and passed there unchanged: it pins that behaviour."""
import ctypes as C
import importlib
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_ref as PR  # noqa: E402
import tiff_encode_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
EINVAL, ENOMEM = -1, -3
DECODERS = ["rtn_jpeg_decode", "rtn_png_decode", "rtn_png_stream_decode", "rtn_png_layout_decode", "rtn_tiff_decode"]
ENCODERS = ["rtn_jpeg_encode", "rtn_png_encode", "rtn_tiff_encode"]
SIZES = ((8, 8), (33, 70), (8, 8))                       # (H, W) of the three pages of a case: two sizes, two workspace sizes


@pytest.fixture(scope="module")
def PIO():
    return importlib.import_module("retinanet-for-table-detection_amd.model.page_io")


def pattern(nbytes):
    return torch.full((int(nbytes),), PATTERN, dtype=torch.uint8, device="cuda")


def i32(v):
    return np.ascontiguousarray(v, np.int32).reshape(-1)


def table(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def pillow_file(page, fmt, **kw):
    b = io.BytesIO()
    Image.fromarray(page[:, :, ::-1] if page.ndim == 3 else page).save(b, fmt, **kw)
    return b.getvalue()


def palette_file(rng, h, w):
    im = Image.frombytes("P", (w, h), rng.randint(0, 16, (h, w)).astype(np.uint8).tobytes())
    im.putpalette(rng.randint(0, 256, 48).astype(np.uint8).tobytes())
    b = io.BytesIO()
    im.save(b, "PNG")
    return b.getvalue()


def page_of(rng, h, w, gray):
    """A smooth page (so the JPEG stays in the range the device vouches for), gray or B,G,R."""
    y, x = np.mgrid[0:h, 0:w]
    base = (40 + 3 * x + 2 * y + rng.randint(0, 8, (h, w))) % 256
    if gray:
        return base.astype(np.uint8)
    return np.stack([base, 255 - base, base // 2], axis=2).astype(np.uint8)


def decoder_file(name, rng, h, w, gray):
    page = page_of(rng, h, w, gray)
    if name == "rtn_jpeg_decode":
        return pillow_file(page, "JPEG", quality=90)
    if name == "rtn_png_decode":
        return PR.build_file(page)
    if name == "rtn_png_stream_decode":
        return pillow_file(page, "PNG")
    if name == "rtn_png_layout_decode":
        return palette_file(rng, h, w)
    return pillow_file(page, "TIFF")                     # uncompressed, one strip


class Decoder:
    """Three blobs (SIZES) in one host buffer; the arguments between the handle and the workspace by name."""
    order = ("host_blobs", "dev_blobs", "offsets", "pages", "status")

    def __init__(self, lib, PIO, name):
        inspect = {"rtn_jpeg_decode": PIO.jpeg_inspect, "rtn_png_decode": PIO.png_inspect, "rtn_png_stream_decode": PIO.png_stream_inspect,
                   "rtn_png_layout_decode": PIO.png_layout_inspect, "rtn_tiff_decode": PIO.tiff_inspect}[name]
        self.name, self.f = name, getattr(lib, name)
        self.inspector = {"rtn_jpeg_decode": "rtn_jpeg_inspect", "rtn_png_decode": "rtn_png_inspect"}.get(name, name.replace("_decode", "_inspect"))
        self.size = getattr(lib, {"rtn_jpeg_decode": "rtn_jpeg_workspace_bytes"}.get(name, name + "_workspace_bytes"))
        rng = np.random.RandomState(3)
        found = [inspect(decoder_file(name, rng, h, w, True)) for h, w in SIZES]
        assert all(info is not None for info, _ in found), found
        self.infos = [info for info, _ in found]
        offs, pos = [], 0
        for _, blob in found:
            offs.append(pos)
            pos += (len(blob) + 15) & ~15
        self.host = np.zeros(pos + 1024, np.uint8)
        for off, (_, blob) in zip(offs, found):
            self.host[off:off + len(blob)] = blob
        self.offsets = np.ascontiguousarray(offs, np.int64)
        self.dev = pattern(pos + 1024)
        self.pages = [pattern(i.height * i.width * 3) for i in self.infos]
        self.status = pattern(4 * len(SIZES))
        self.outs = self.pages + [self.status]
        self.ptrs = table([p.data_ptr() for p in self.pages])
        self.base = dict(host_blobs=self.host.ctypes.data, dev_blobs=self.dev.data_ptr(), offsets=self.offsets.ctypes.data, pages=self.ptrs,
                         status=self.status.data_ptr())
        assert self.dev.data_ptr() % 16 == 0

    def need(self, n):
        return int(self.size(n, self.host.ctypes.data, self.offsets.ctypes.data))

    def bad_blob(self, i):
        """host_blobs with the first header word of blob i overwritten -> (array to keep alive, pointer)"""
        host = self.host.copy()
        host[int(self.offsets[i]):int(self.offsets[i]) + 4] ^= 0xFF
        return host, host.ctypes.data

    def bad_second(self):
        host, p = self.bad_blob(1)
        return host, dict(host_blobs=p)


class Encoder:
    """Three pages (SIZES: gray, B,G,R, gray), one slot of the bound rounded up to 256 bytes each."""

    def __init__(self, lib, name):
        self.name, self.f = name, getattr(lib, name)
        self.size = getattr(lib, name + "_workspace_bytes")
        self.W, self.H, self.Cc = i32([w for _, w in SIZES]), i32([h for h, _ in SIZES]), i32([1, 3, 1])
        n = len(SIZES)
        if name == "rtn_jpeg_encode":
            self.extra = dict(subsampling=i32([2] * n), quality=i32([90] * n))
            self.size_extra = ("subsampling",)
            bound = lambda k: lib.rtn_jpeg_encode_bound(int(self.W[k]), int(self.H[k]), int(self.Cc[k]), 2)
        elif name == "rtn_png_encode":
            self.extra, self.size_extra = {}, ()
            bound = lambda k: lib.rtn_png_encode_bound(int(self.W[k]), int(self.H[k]), int(self.Cc[k]))
        else:
            self.extra = dict(thresholds=i32([128] * n), rows_per_strip=i32([64] * n), photometric=i32([0] * n))
            self.size_extra = ("rows_per_strip",)
            bound = lambda k: lib.rtn_tiff_encode_bound(int(self.W[k]), int(self.H[k]), 64)
        self.bounds = [int(bound(k)) for k in range(n)]
        assert all(b > 0 for b in self.bounds)
        self.offs = np.zeros(n + 1, np.int64)
        self.offs[1:] = np.cumsum([(b + 255) & ~255 for b in self.bounds])
        self.src = [pattern(h * w * c) for (h, w), c in zip(SIZES, self.Cc)]
        self.out, self.out_bytes, self.status = pattern(int(self.offs[-1]) + 256), pattern(8 * n), pattern(4 * n)
        self.outs = [self.out, self.out_bytes, self.status]
        self.ptrs = table([p.data_ptr() for p in self.src])
        self.order = ("pages", "widths", "heights", "components") + tuple(self.extra) + ("out", "out_offsets", "out_bytes", "status")
        self.base = dict(pages=self.ptrs, widths=self.W.ctypes.data, heights=self.H.ctypes.data, components=self.Cc.ctypes.data,
                         out=self.out.data_ptr(), out_offsets=self.offs.ctypes.data, out_bytes=self.out_bytes.data_ptr(),
                         status=self.status.data_ptr(), **{k: v.ctypes.data for k, v in self.extra.items()})
        assert self.out.data_ptr() % 4 == 0

    def size_args(self, **kw):
        a = dict(widths=self.W.ctypes.data, heights=self.H.ctypes.data, components=self.Cc.ctypes.data,
                 **{k: self.extra[k].ctypes.data for k in self.size_extra})
        a.update(kw)
        return [a[k] for k in ("widths", "heights", "components") + self.size_extra]

    def need(self, n):
        return int(self.size(n, *self.size_args()))

    def changed(self, key, index, value):
        """one per-page int32 or int64 argument with entry `index` replaced -> (array to keep alive, {key: pointer})"""
        src = {"components": self.Cc, "out_offsets": self.offs, **self.extra}[key]
        a = src.copy()
        a[index] = value
        return a, {key: a.ctypes.data}

    def bad_second(self):
        return self.changed("components", 1, 2)


@pytest.fixture(scope="module")
def cases(pkg, PIO):
    lib = pkg.lib
    made = {name: Decoder(lib, PIO, name) for name in DECODERS}
    made.update({name: Encoder(lib, name) for name in ENCODERS})
    return made


class Caller:
    """One entry on one case: call(n, ws, wsb, **replaced arguments); refused() also checks that nothing was written."""

    def __init__(self, pkg, handle, case):
        self.lib, self.h, self.case = pkg.lib, handle.raw, case
        self.wsb = case.need(1)
        assert self.wsb > 0
        self.ws = torch.empty(case.need(3) + 256, dtype=torch.uint8, device="cuda")
        assert self.ws.data_ptr() % 256 == 0

    def err(self):
        return self.lib.rtn_last_error(self.h)

    def call(self, n=1, ws=0, wsb=None, **kw):
        a = dict(self.case.base)
        a.update(kw)
        return self.case.f(self.h, n, *[a[k] for k in self.case.order], self.ws.data_ptr() + ws if ws is not None else None,
                           self.wsb if wsb is None else wsb)

    def refused(self, text, code=EINVAL, **kw):
        rc = self.call(**kw)
        assert rc == code, (self.case.name, kw, rc, self.err())
        for t in ([text] if isinstance(text, str) else text):
            assert t.encode() in self.err(), (self.case.name, kw, t, self.err())
        torch.cuda.synchronize()
        assert all(bool((o == PATTERN).all()) for o in self.case.outs), (self.case.name, kw)                            # (g)


def common_refusals(c):
    case = c.case
    c.refused("n < 0", n=-1)                                                                                            # (a)
    assert case.f(c.h, 0, *[None] * len(case.order), None, 0) == 0, c.err()
    assert case.f(None, 1, *[case.base[k] for k in case.order], c.ws.data_ptr(), c.wsb) == EINVAL                      # no handle
    for k in case.order:                                                                                                # (b)
        c.refused("NULL argument", **{k: None})
    c.refused("NULL argument", ws=None)
    c.refused("aligned", ws=16)                                                                                         # (c)
    c.refused(["workspace %d < %d bytes" % (c.wsb - 1, c.wsb)], code=ENOMEM, wsb=c.wsb - 1)                             # (f)
    keep, bad = case.bad_second()                                                                                       # (h)
    need2 = case.need(2)
    c.refused("aligned", n=2, ws=16, wsb=need2, **bad)
    c.refused("page 0 is NULL", n=2, wsb=need2, pages=table([None, case.ptrs[1]]), **bad)
    del keep


@pytest.mark.parametrize("name", DECODERS)
def test_decoder_refusals(pkg, handle, cases, name):
    case = cases[name]
    c = Caller(pkg, handle, case)
    common_refusals(c)
    c.refused("aligned", dev_blobs=case.dev.data_ptr() + 8)                                                             # (c)
    for off in (8, -16):                                                                                                # (d)
        offs = case.offsets.copy()
        offs[0] = off
        c.refused("blob 0 offset not 16-byte aligned", offsets=offs.ctypes.data)
    keep, p = case.bad_blob(0)
    c.refused("blob 0 is not an %s blob" % case.inspector, host_blobs=p)
    c.refused("page 0 is NULL", pages=table([None]))
    del keep


@pytest.mark.parametrize("name", ENCODERS)
def test_encoder_refusals(pkg, handle, cases, name):
    case = cases[name]
    c = Caller(pkg, handle, case)
    common_refusals(c)
    changed = lambda *a: case.changed(*a)[1]                                                                            # noqa: E731
    c.refused("", **changed("components", 0, 2))                                                                        # (e)
    c.refused("", pages=table([None]))
    b = case.bounds[0]
    if name == "rtn_jpeg_encode":
        offs = np.ascontiguousarray([16, 0], np.int64)
        c.refused("output slot 0 is [16, 0)", out_offsets=offs.ctypes.data)
    else:
        offs = np.ascontiguousarray([0, b - 1], np.int64)
        c.refused(["output slot 0 is [0, %d)" % (b - 1), name + "_bound asks for %d bytes" % b], out_offsets=offs.ctypes.data)
    if name == "rtn_tiff_encode":
        offs = np.ascontiguousarray([2, 2 + b], np.int64)
        c.refused("output slot 0 is not 4-byte aligned", out_offsets=offs.ctypes.data)
        c.refused("threshold 0", **changed("thresholds", 0, 0))
        c.refused("photometric 2", **changed("photometric", 0, 2))


@pytest.mark.parametrize("name", DECODERS)
def test_decoder_workspace_bytes(cases, name):                                                                          # (i)
    case = cases[name]
    host, offs = case.host.ctypes.data, case.offsets.ctypes.data
    assert case.size(0, host, offs) == 0 and case.size(3, None, offs) == 0 and case.size(3, host, None) == 0
    want = [int(i.workspace_bytes) for i in case.infos]
    assert all(w > 0 for w in want)
    assert [case.size(1, host, case.offsets[k:].ctypes.data) for k in range(3)] == want
    assert case.size(3, host, offs) == sum(want)
    keep, p = case.bad_blob(1)
    assert case.size(3, p, offs) == 0 and case.size(1, p, offs) == want[0]
    # a negative offset: 64 bytes into zeros, so an entry that reads the header before it looks at the sign stays inside the array
    zeros = np.zeros(2048, np.uint8)
    neg = np.ascontiguousarray([-16], np.int64)
    assert case.size(1, zeros.ctypes.data + 64, neg.ctypes.data) == 0


@pytest.mark.parametrize("name", ENCODERS)
def test_encoder_workspace_bytes(cases, name):                                                                          # (i)
    case = cases[name]
    keys = ("widths", "heights", "components") + case.size_extra
    assert case.size(0, *case.size_args()) == 0
    for k in keys:
        assert case.size(3, *case.size_args(**{k: None})) == 0, k
    per_page = {"widths": case.W, "heights": case.H, "components": case.Cc, **case.extra}
    single = [int(case.size(1, *[per_page[k][j:].ctypes.data for k in keys])) for j in range(3)]
    assert all(s > 0 for s in single) and single[0] == single[2] != single[1]
    assert case.size(3, *case.size_args()) == sum(single)
    bad = case.Cc.copy()
    bad[1] = 2
    assert case.size(3, *case.size_args(components=bad.ctypes.data)) == 0
    assert case.size(1, *case.size_args(components=bad.ctypes.data)) == single[0]


# ---- (j) 33 pages: the second launch of the batch loop ----------------------------------------------------------------------------------
N = 33
BIG, SMALL = (33, 47), (16, 9)                           # (H, W), alternating


def by_name(got, want):
    assert len(got) == len(want) == N
    assert got[31] == want[31], "page 31, the last of the first launch"
    assert got[32] == want[32], "page 32, the first of the second launch"
    bad = [i for i in range(N) if got[i] != want[i]]
    assert not bad, bad


@pytest.mark.parametrize("name", DECODERS)
def test_decoder_second_launch(PIO, monkeypatch, name):
    for knob in ("RTN_PNG_STREAM_MIN", "RTN_PNG_LAYOUT_MIN", "RTN_TIFF_MIN"):
        monkeypatch.setenv(knob, "1")
    rng = np.random.RandomState(11)
    files = [decoder_file(name, rng, *(SMALL if i % 2 else BIG), gray=bool(i % 2)) for i in range(N)]
    fmt = {"rtn_jpeg_decode": PIO._JPEG, "rtn_png_decode": PIO._PNG, "rtn_png_stream_decode": PIO._PNG_STREAM,
           "rtn_png_layout_decode": PIO._PNG_LAYOUT, "rtn_tiff_decode": PIO._TIFF}[name]
    calls = []
    monkeypatch.setattr(PIO, "_ALL_FORMATS", tuple(f._replace(decode=lambda *a, f=f: calls.append((f.name, a[1])) or f.decode(*a))
                                                   for f in PIO._ALL_FORMATS))
    pages, words = PIO.decode_png_bgr(files, return_status=True)
    assert calls == [(fmt.name, N)], calls                               # one call of this entry took all 33 files
    assert words == [0] * N, words
    want = [PIO._pillow_bgr(io.BytesIO(f)) for f in files]
    by_name([p.cpu().numpy().tobytes() for p in pages], [w.tobytes() for w in want])
    assert all(p.shape == w.shape for p, w in zip(pages, want))


@pytest.mark.parametrize("name", ENCODERS)
def test_encoder_second_launch(pkg, PIO, monkeypatch, name):
    rng = np.random.RandomState(12)
    pages = [page_of(rng, *(SMALL if i % 2 else BIG), gray=bool(i % 2)) for i in range(N)]
    dev = [torch.from_numpy(p).cuda() for p in pages]
    if name == "rtn_jpeg_encode":
        want = [PIO._pillow_jpeg(p, 90, 2) for p in pages]

        def no_host(*a):
            raise AssertionError("a page was flagged and left to Pillow")
        monkeypatch.setattr(PIO, "_pillow_jpeg", no_host)                # so every status word was 0
        by_name(PIO.encode_jpeg_bgr(dev, quality=90, subsampling=2), want)
    elif name == "rtn_png_encode":
        files = PIO.encode_png_bgr(dev)                                  # raises unless every length is in (0, bound]
        by_name([PIO._pillow_bgr(io.BytesIO(f)).tobytes() for f in files],
                [np.ascontiguousarray(p if p.ndim == 3 else np.repeat(p[:, :, None], 3, axis=2)).tobytes() for p in pages])
        for f, p in zip(files, pages):
            PR.check_file(f, p)
    else:
        cs = [TR.Case("page %d" % i, p, 100 + i, (64, 5)[i % 2], i % 2) for i, p in enumerate(pages)]
        files = PIO.encode_tiff_bgr(dev, threshold=[c.threshold for c in cs], rows_per_strip=[c.rows_per_strip for c in cs],
                                    photometric=[c.photometric for c in cs])
        by_name(files, [TR.twin_file(pkg, c) for c in cs])
