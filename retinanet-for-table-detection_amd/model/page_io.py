"""Page files, read and written as cv2.imread / cv2.imwrite do, with the seven device codecs behind them: baseline
JPEG and chunked-layout PNG pages are decoded and encoded on the device, ordinary 8-bit gray and R,G,B PNG pages (one zlib stream,
all five row filters) are decoded there in calls of at least RTN_PNG_STREAM_MIN files (default 4), PNG pages of the other pixel
layouts (1-, 2- and 4-bit gray, palette, alpha, 16-bit R,G,B, Adam7 interlace, tRNS) by the same decoder with another last stage in
calls of at least RTN_PNG_LAYOUT_MIN files (default 2), strip TIFF pages (uncompressed, PackBits, LZW, Deflate or CCITT Group 4;
bilevel, 8-bit gray, palette or R,G,B) in calls of at least RTN_TIFF_MIN files (default 2), bilevel pages are
written as CCITT Group 4 TIFFs on the device on request (encode_tiff_bgr, write_images_bgr(tiff="g4")), every other
file (16-bit gray PNG, tiled, JPEG-in-TIFF or 16-bit TIFF, BMP, ...) is left to Pillow.  Scanned PDFs are model/pdf.py's, which
wraps their image streams as such files held in memory and hands them to _decode_datas.  csv_generator.py,
model/utils.py and model/preprocess.py import from here; the public names stay importable from the first two (re-exports)."""
import contextlib
import ctypes as C
import io
import os
import threading
from collections import namedtuple

import numpy as np
import torch
from PIL import Image

from . import _rt

L = _rt.L


def _pillow_bgr(fp):
    with Image.open(fp) as im:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1])


def read_image_bgr(path):
    """cv2.imread(path): uint8 (H,W,3) in B,G,R order.  Decoded with Pillow (OpenCV is not a dependency of this package)."""
    return _pillow_bgr(path)


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"

PNG_STREAM_MIN_DEFAULT = 4


def png_stream_min():
    """RTN_PNG_STREAM_MIN: the fewest files in one call for which its ordinary (single-stream) PNGs are decoded on the device;
    0 leaves them all to Pillow.  The default, 4, is the batch at which the device first beat Pillow on one thread on both kinds
    of sample-sized page (profiles/png_stream_decode_bench.txt)."""
    try:
        return max(0, int(os.environ.get("RTN_PNG_STREAM_MIN", "") or PNG_STREAM_MIN_DEFAULT))
    except ValueError:
        return PNG_STREAM_MIN_DEFAULT


PNG_LAYOUT_MIN_DEFAULT = 2


def png_layout_min():
    """RTN_PNG_LAYOUT_MIN: the fewest files in one call for which its PNGs of the other pixel layouts (sub-byte gray, palette, alpha,
    16-bit R,G,B, Adam7; DESIGN §3.4f, "Pixel layouts") are decoded on the device; 0 leaves them all to Pillow.  Same semantics as
    RTN_PNG_STREAM_MIN.  The default, 2, is the smallest batch at which the device beat Pillow on one thread on all four kinds of
    sample-sized page measured (1-bit gray, 16-colour palette, R,G,B,A, Adam7 R,G,B: profiles/png_layout_decode_bench.txt)."""
    try:
        return max(0, int(os.environ.get("RTN_PNG_LAYOUT_MIN", "") or PNG_LAYOUT_MIN_DEFAULT))
    except ValueError:
        return PNG_LAYOUT_MIN_DEFAULT


TIFF_MIN_DEFAULT = 2


def tiff_min():
    """RTN_TIFF_MIN: the fewest files in one call for which its TIFFs are decoded on the device; 0 leaves them all
    to Pillow.  Same semantics as RTN_PNG_STREAM_MIN.  The default, 2, is the smallest batch at which the device beat Pillow on one
    thread on every kind of sample-sized page it takes by default (Group 4 needs 2 files, every other kind 1; a Group 4 page written
    as one strip wins only at 16 and is refused by the inspector unless RTN_TIFF_G4_ONE_STRIP=1: profiles/tiff_decode_bench.txt)."""
    try:
        return max(0, int(os.environ.get("RTN_TIFF_MIN", "") or TIFF_MIN_DEFAULT))
    except ValueError:
        return TIFF_MIN_DEFAULT


# One record per format the device decodes, in the order _decode_datas tries them: JPEG first, then PNG of the chunked layout,
# then any other PNG.  min_files(): the fewest files in one call for which the format is tried at all (0: never).
_Format = namedtuple("_Format", "name Info inspect blob_bound workspace_bytes decode min_files")
_FORMATS = (
    _Format("jpeg", L.JpegInfo, L.lib.rtn_jpeg_inspect, L.jpeg_blob_bound, L.lib.rtn_jpeg_workspace_bytes, L.lib.rtn_jpeg_decode,
            lambda: 1),
    _Format("png", L.PngInfo, L.lib.rtn_png_inspect, L.png_blob_bound, L.lib.rtn_png_decode_workspace_bytes, L.lib.rtn_png_decode,
            lambda: 1),
    _Format("png_stream", L.PngInfo, L.lib.rtn_png_stream_inspect, L.lib.rtn_png_stream_blob_bound,
            L.lib.rtn_png_stream_decode_workspace_bytes, L.lib.rtn_png_stream_decode, png_stream_min),
)
_JPEG, _PNG, _PNG_STREAM = _FORMATS
# The formats tried after those of _FORMATS (the dispatch loops run over _ALL_FORMATS, below): the PNGs whose pixels are not
# whole 8-bit gray or R,G,B samples, or that are interlaced.
def _layout_only_inspect(h, data, n, info, blob, capacity):
    """rtn_png_layout_inspect for the files rtn_png_stream_inspect refuses.  The layout inspector takes ordinary PNGs too, but where
    those are decoded is RTN_PNG_STREAM_MIN's to say: in a call too small for it they stay on Pillow, as before."""
    if L.lib.rtn_png_stream_inspect(h, data, n, C.byref(L.PngInfo()), None, 0) == 0:
        return -1                                                     # *info is read only after a 0
    return L.lib.rtn_png_layout_inspect(h, data, n, info, blob, capacity)


_MORE_FORMATS = (
    _Format("png_layout", L.PngInfo, _layout_only_inspect, L.lib.rtn_png_layout_blob_bound,
            L.lib.rtn_png_layout_decode_workspace_bytes, L.lib.rtn_png_layout_decode, png_layout_min),
)
_PNG_LAYOUT, = _MORE_FORMATS
# Tried after every PNG format: strip TIFFs.  _ALL_FORMATS is what the dispatch loops run over.
_TIFF_FORMATS = (
    _Format("tiff", L.TiffInfo, L.lib.rtn_tiff_inspect, L.lib.rtn_tiff_blob_bound, L.lib.rtn_tiff_decode_workspace_bytes,
            L.lib.rtn_tiff_decode, tiff_min),
)
_TIFF, = _TIFF_FORMATS
_ALL_FORMATS = _FORMATS + _MORE_FORMATS + _TIFF_FORMATS
TIFF_SIGNATURES = (b"II*\0", b"MM\0*")


def _inspect(fmt, data):
    info = fmt.Info()
    blob = np.empty(fmt.blob_bound(len(data)), np.uint8)
    rc = fmt.inspect(None, data, len(data), C.byref(info), blob.ctypes.data, blob.size)
    if rc != 0:
        return None, L.lib.rtn_last_error(None).decode("utf-8", "replace")
    return info, blob[:info.blob_bytes]


def jpeg_inspect(data):
    """Parse one file's bytes with rtn_jpeg_inspect (host only) -> (JpegInfo, blob bytes) for a baseline JPEG the device decodes,
    or (None, reason) for anything else."""
    return _inspect(_JPEG, data)


def png_inspect(data):
    """Parse one file's bytes with rtn_png_inspect (host only) -> (PngInfo, blob bytes) for a PNG of the chunked layout (DESIGN
    §3.4d) that the device decodes, or (None, reason) for anything else."""
    return _inspect(_PNG, data)


def png_stream_inspect(data):
    """Parse one file's bytes with rtn_png_stream_inspect (host only) -> (PngInfo, blob bytes) for an ordinary 8-bit gray or R,G,B
    PNG (one zlib stream over any number of IDATs, harmless ancillary chunks) that the device can decode, or
    (None, reason) for anything else.  PngInfo.chunks counts the segments of RTN_PNG_SEGMENT compressed bytes."""
    return _inspect(_PNG_STREAM, data)


def png_layout_inspect(data):
    """Parse one file's bytes with rtn_png_layout_inspect (host only) -> (PngInfo, blob bytes) for a PNG of any pixel layout the
    device decodes (what png_stream_inspect accepts, and 1-, 2- and 4-bit gray, palette, gray + alpha, R,G,B,A, 16-bit R,G,B, each
    with or without Adam7 interlace, with tRNS; DESIGN §3.4f, "Pixel layouts"), or (None, reason) for anything else (16-bit gray,
    bKGD, unknown chunks, ...).  PngInfo.components is the file's samples per pixel."""
    return _inspect(_PNG_LAYOUT._replace(inspect=L.lib.rtn_png_layout_inspect), data)


def tiff_inspect(data):
    """Parse one file's bytes with rtn_tiff_inspect (host only) -> (TiffInfo, blob bytes) for a strip TIFF the device decodes
    (first IFD; Compression 1, 32773, 5, 8 / 32946 or 4; bilevel, 8-bit gray, palette or R,G,B), or (None, reason)
    for anything else (tiles, BigTIFF, Group 3, JPEG-in-TIFF, old-style LZW, 2-, 4- or 16-bit samples, CMYK / YCbCr / Lab, extra
    samples, planar 2, Orientation other than 1, offsets outside the file, ...)."""
    return _inspect(_TIFF, data)


def _blob_bound(d):
    """The most blob bytes any inspector of _ALL_FORMATS writes for the file d: formats are told apart by signature."""
    if d[:8] == PNG_SIGNATURE:
        return max(_PNG.blob_bound(len(d)), _PNG_LAYOUT.blob_bound(len(d)))
    if d[:4] in TIFF_SIGNATURES:
        return _TIFF.blob_bound(len(d))
    return _JPEG.blob_bound(len(d))


def _decode_datas(datas, host_decode, device, handle, stream, formats=None):
    """The pages of the files `datas` (list of bytes, or None for a file left to the host): every file that the inspector of one
    of `formats` (by default _ALL_FORMATS; model/pdf.py passes the same records with another TIFF inspector) accepts (the first that does takes it; a format whose min_files() is 0 or above len(datas) is not tried) is decoded on the device, each decoder running at most once, after ONE host->device copy of all blobs; the status
    words of all are read once, on `stream`; the other pages (and the pages whose status is non-zero) come
    from host_decode(i), in page order, and are uploaded.  Returns (pages, status) with status[i] the device's word for page i
    (None where no device decoder took the file)."""
    out, words = [None] * len(datas), [None] * len(datas)
    on_host = [i for i, d in enumerate(datas) if d is None]        # host_decode raises the file's exception below, in page order
    limit = Image.MAX_IMAGE_PIXELS
    # a file with the PNG or a TIFF signature fails rtn_jpeg_inspect at its first two bytes, before anything is written, and the
    # other inspectors refuse at the signature likewise (a PNG blob is bounded by the larger of its inspectors' bounds)
    cap = sum(_blob_bound(d) for d in datas if d is not None)
    every = _ALL_FORMATS if formats is None else formats
    with torch.cuda.stream(stream):
        host = torch.empty(max(cap, 16), dtype=torch.uint8, pin_memory=True)
        hp = host.data_ptr()
        pos = 0
        kinds = {fmt.name: ([], [], []) for fmt in every}            # blob offsets, pages, file indices
        formats = [fmt for fmt in every if 1 <= fmt.min_files() <= len(datas)]
        for i, data in enumerate(datas):
            if data is None:
                continue
            for fmt in formats:
                info = fmt.Info()
                rc = fmt.inspect(None, data, len(data), C.byref(info), hp + pos, cap - pos)
                if rc == 0:
                    break
            if rc != 0 or (limit and info.width * info.height > limit):
                on_host.append(i)
                continue
            offsets, pages, which = kinds[fmt.name]
            offsets.append(pos)
            pos += info.blob_bytes
            pages.append(torch.empty(info.height, info.width, 3, dtype=torch.uint8, device=device))
            which.append(i)
        taken = [(page, i) for _, pages, which in kinds.values() for page, i in zip(pages, which)]      # in the order of the status words
        n = len(taken)
        if n:
            dev_blobs = host[:pos].to(device, non_blocking=True)
            status = torch.empty(n, dtype=torch.int32, device=device)
            handle.set_stream(stream.cuda_stream)
            keep = []                                                  # the workspaces live until the stream is synchronised
            first = 0
            for fmt in every:
                offsets, pages, which = kinds[fmt.name]
                m = len(which)
                if not m:
                    continue
                offs = np.asarray(offsets, np.int64)
                ws_bytes = int(fmt.workspace_bytes(m, hp, offs.ctypes.data))
                ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=device)
                ptrs = (C.c_void_p * m)(*[p.data_ptr() for p in pages])
                handle.check(fmt.decode(handle.raw, m, hp, dev_blobs.data_ptr(), offs.ctypes.data, ptrs,
                                        status[first:first + m].data_ptr(), ws.data_ptr(), ws_bytes))
                keep.append(ws)
                first += m
            st = torch.empty(n, dtype=torch.int32, pin_memory=True)
            st.copy_(status, non_blocking=True)
            stream.synchronize()
            for k, (page, i) in enumerate(taken):
                words[i] = int(st[k])
                if words[i] == 0:
                    out[i] = page
                else:
                    on_host.append(i)
        for i in sorted(on_host):
            out[i] = torch.from_numpy(host_decode(i)).to(device)
    return out, words


def _decode_batch(paths, device, handle, stream):
    """read_images_bgr on an explicit handle and stream (see _decode_datas); a file that cannot be read is left to
    read_image_bgr, which raises the same exception."""
    datas = []
    for path in paths:
        try:
            with open(path, 'rb') as f:
                datas.append(f.read())
        except OSError:
            datas.append(None)
    return _decode_datas(datas, lambda i: read_image_bgr(paths[i]), device, handle, stream)[0]


_readers = {}
_readers_lock = threading.Lock()


@contextlib.contextmanager
def _reader(device):
    """`device` (None, an int or a torch.device) as an indexed CUDA device, and that device's reader handle: (device, Handle).
    _readers_lock is held while the caller is inside the `with`, that is for the whole decode."""
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device or "cuda")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    with _readers_lock:
        h = _readers.get(dev.index)
        if h is None:
            h = _readers[dev.index] = L.Handle(dev.index)
        yield dev, h


def read_images_bgr(paths, device=None):
    """read_image_bgr for a list of files, as CUDA uint8 (H,W,3) B,G,R tensors with the same bits.  Baseline JPEGs (the files
    cv2.imwrite writes for a .jpg name) and PNGs of the chunked layout of DESIGN §3.4d (the files write_images_bgr(png="device")
    and preprocess_files(png="device") write) are decoded on the device, one batched call per format (csrc/rtn_jpeg.hip,
    csrc/rtn_png_dec.hip) on the current stream after one copy of the files' entropy-coded bytes.  Ordinary PNGs (what Pillow,
    libpng and cv2.imwrite write: 8-bit gray or R,G,B, one zlib stream, any of the five row filters, harmless ancillary chunks)
    take the same road through csrc/rtn_png_stream.hip when the call holds at least RTN_PNG_STREAM_MIN files
    (default 4; 0: never).  PNGs of the other pixel layouts (1-, 2- and 4-bit gray, palette, gray + alpha, R,G,B,A, 16-bit R,G,B,
    each with or without Adam7 interlace or a tRNS chunk: what ImageMagick, pdftoppm -mono, optipng, pngquant, screenshot tools
    and cv2.imwrite of four channels write) go through the same decoder with its pixel-layout stage (rtn_png_layout_decode, DESIGN
    §3.4f "Pixel layouts") when the call holds at least RTN_PNG_LAYOUT_MIN files (default 2; 0: never).  Strip TIFFs (what scanners
    and scan archives write: first IFD, uncompressed, PackBits, LZW, Deflate or CCITT Group 4; bilevel with either photometric and
    fill order, 8-bit gray, palette or R,G,B; predictor 2; any RowsPerStrip, byte order and field type) go through
    csrc/rtn_tiff.hip, one wave per strip, when the call holds at least RTN_TIFF_MIN files (default 2; 0: never); the inspector
    refuses tiles, BigTIFF, Group 3, JPEG-in-TIFF, old-style LZW, 2-, 4- and 16-bit samples, CMYK / YCbCr / Lab, extra samples,
    planar 2, Orientation other than 1, offsets outside the file and, unless RTN_TIFF_G4_ONE_STRIP=1, Group 4 pages written as one
    strip (one serial decoder per page).  Every other file (16-bit
    gray PNGs, PNGs with bKGD or unknown chunks, BMP, ...), and any file whose stream a device decode flags, is decoded by read_image_bgr on one thread and uploaded; a PNG dataset can
    also be converted once with write_images_bgr(paths, read_images_bgr(paths), png="device").  A file Pillow cannot open raises
    what read_image_bgr raises."""
    with _reader(device) as (dev, h):
        return _decode_batch(list(paths), dev, h, torch.cuda.current_stream(dev))


def decode_png_bgr(files, device=None, return_status=False):
    """The pages of PNG files held in memory (list of bytes) as CUDA uint8 (H,W,3) B,G,R tensors with the bits Pillow gives:
    the counterpart of encode_png_bgr, on read_images_bgr's path.  Files of the chunked layout are decoded in one
    batched rtn_png_decode on the current stream (csrc/rtn_png_dec.hip), ordinary 8-bit gray and R,G,B PNGs in one batched
    rtn_png_stream_decode (csrc/rtn_png_stream.hip) when the call holds at least RTN_PNG_STREAM_MIN files (default 4;
    0: never), PNGs of the other pixel layouts (sub-byte gray, palette, alpha, 16-bit R,G,B, Adam7, tRNS) in one batched
    rtn_png_layout_decode when the call holds at least RTN_PNG_LAYOUT_MIN files (default 2; 0: never); any other file (16-bit gray,
    ...), or one that the device flags, is decoded by Pillow from the bytes.  return_status=True returns (pages, status) instead, status[i] being the
    device's status word for file i (0 = the device's page was kept) or None where the device did not take the file."""
    files = [bytes(f) for f in files]
    with _reader(device) as (dev, h):
        pages, words = _decode_datas(files, lambda i: _pillow_bgr(io.BytesIO(files[i])), dev, h, torch.cuda.current_stream(dev))
    return (pages, words) if return_status else pages


def decode_tiff_bgr(files, device=None, return_status=False):
    """The pages of TIFF files held in memory (list of bytes) as CUDA uint8 (H,W,3) B,G,R tensors with the bits Pillow gives: the
    counterpart of decode_png_bgr, on read_images_bgr's path.  The files tiff_inspect accepts are decoded in one batched
    rtn_tiff_decode on the current stream (csrc/rtn_tiff.hip) when the call holds at least RTN_TIFF_MIN files (0:
    never); any other file, or one that the device flags, is decoded by Pillow from the bytes.  return_status=True returns (pages,
    status) instead, status[i] being the device's status word for file i (0 = the device's page was kept) or None where the device
    did not take the file."""
    return decode_png_bgr(files, device=device, return_status=return_status)


def write_image(path, image):
    """cv2.imwrite of a uint8 (H,W[,3]) array whose channels the caller treats in OpenCV's B,G,R order."""
    a = np.ascontiguousarray(image)
    Image.fromarray(a[:, :, ::-1] if a.ndim == 3 else a).save(path)


JPEG_EXTENSIONS = ('.jpg', '.jpeg', '.jpe')
JPEG_MAX_SIDE = 65500                                   # libjpeg's JPEG_MAX_DIMENSION


def _check_page(i, p):
    """(H, W, components) of one page for encode_jpeg_bgr / encode_png_bgr, or ValueError."""
    if not isinstance(p, (torch.Tensor, np.ndarray)):
        p = np.asarray(p)
    dtype, shape = p.dtype, tuple(p.shape)
    if dtype != (torch.uint8 if isinstance(p, torch.Tensor) else np.uint8):
        raise ValueError("page %d: uint8 pixels expected, got %s" % (i, dtype))
    if not (len(shape) == 2 or (len(shape) == 3 and shape[2] == 3)):
        raise ValueError("page %d: shape (H,W,3) B,G,R or (H,W) gray expected, got %s" % (i, shape))
    if not (1 <= shape[0] <= JPEG_MAX_SIDE and 1 <= shape[1] <= JPEG_MAX_SIDE):
        raise ValueError("page %d: %dx%d: sides must be 1..%d (the image writers' limit, JPEG's)" % (i, shape[0], shape[1], JPEG_MAX_SIDE))
    return shape[0], shape[1], 1 if len(shape) == 2 else 3


def _check_settings(quality, subsampling, n=None):
    """(qualities, subsamplings) as lists of n, from ints or per-page sequences; ValueError for anything else."""
    def per_page(v, name):
        if isinstance(v, (list, tuple, np.ndarray)):
            v = list(v)
            if n is not None and len(v) != n:
                raise ValueError("%d %s values for %d pages" % (len(v), name, n))
            return v
        return [v] * (n or 0)
    qs, ss = per_page(quality, "quality"), per_page(subsampling, "subsampling")
    for q in (qs if isinstance(quality, (list, tuple, np.ndarray)) else [quality]):
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 1 <= q <= 100:
            raise ValueError("quality must be an integer 1..100, got %r" % (q,))
    for s in (ss if isinstance(subsampling, (list, tuple, np.ndarray)) else [subsampling]):
        if isinstance(s, bool) or s not in (0, 1, 2):
            raise ValueError("subsampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), got %r" % (s,))
    return [int(q) for q in qs], [int(s) for s in ss]


def _host_page(p):
    return p.cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)


def _pillow_jpeg(page, quality, subsampling):
    """The host path: Pillow's JPEG of a B,G,R (or gray) page."""
    a = np.ascontiguousarray(_host_page(page))
    b = io.BytesIO()
    Image.fromarray(a[:, :, ::-1] if a.ndim == 3 else a).save(b, "JPEG", quality=int(quality), subsampling=subsampling)
    return b.getvalue()


def _encode_batch(pages, dims, *, extra, bound, slot, workspace_bytes, encode):
    """The body encode_jpeg_bgr and encode_png_bgr share: upload the pages, lay out one slot of slot(bound(i, W, H, components))
    bytes per page, run `encode` once on the current stream (`extra`: the format's own per-page int32 arrays) and copy the n file
    lengths back.  Returns (device buffer, slot offsets, host lengths, bounds); length 0 = flagged (status != 0), and what
    happens to such a page is the caller's policy."""
    n = len(pages)
    h = _rt.handle()
    dev = []
    for p in pages:
        t = p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(p))
        dev.append(t.to(device="cuda", non_blocking=True).contiguous())
    W, H, Cc = [np.ascontiguousarray([d[k] for d in dims], np.int32) for k in (1, 0, 2)]
    bounds = [int(bound(i, int(w), int(hh), int(c))) for i, (w, hh, c) in enumerate(zip(W, H, Cc))]
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([slot(b) for b in bounds])
    out = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")
    lengths = torch.empty(n, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    whc = (W.ctypes.data, H.ctypes.data, Cc.ctypes.data)
    wsb = int(workspace_bytes(n, *whc))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in dev])
    h.check(encode(h.raw, n, ptrs, *whc, *[e.ctypes.data for e in extra], out.data_ptr(), offs.ctypes.data, lengths.data_ptr(),
                   status.data_ptr(), ws.data_ptr(), wsb))
    nb = torch.empty(n, dtype=torch.int64, pin_memory=True)
    nb.copy_(lengths, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return out, offs, nb.numpy().copy(), bounds


def _files_to_host(out, offs, nb, ok, n):
    """The files of pages `ok` (slot offsets offs, lengths nb in the device buffer out) as bytes, through one copy of the used
    bytes to pinned host memory; None for every other page."""
    files = [None] * n
    if ok:
        used = torch.cat([out[int(offs[i]):int(offs[i]) + int(nb[i])] for i in ok]) if len(ok) > 1 else \
            out[int(offs[ok[0]]):int(offs[ok[0]]) + int(nb[ok[0]])]
        host = torch.empty(used.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(used, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        buf = host.numpy()
        pos = 0
        for i in ok:
            files[i] = buf[pos:pos + int(nb[i])].tobytes()
            pos += int(nb[i])
    return files


def encode_jpeg_bgr(pages, quality=95, subsampling=2):
    """Baseline JPEG files of uint8 (H,W,3) B,G,R or (H,W) gray pages (CUDA or host tensors or arrays), byte-identical to
    Image.fromarray(rgb).save(f, "JPEG", quality=quality, subsampling=subsampling): one batched rtn_jpeg_encode on the current
    stream (csrc/rtn_jpeg_enc.hip), one small copy of the n file lengths, then one copy of the used bytes to pinned host
    memory.  A page the device flags is encoded by Pillow.  The defaults are cv2.imwrite's for a .jpg name; quality and
    subsampling may also be sequences of one value per page.  Returns list[bytes]."""
    pages = list(pages)
    n = len(pages)
    qs, ss = _check_settings(quality, subsampling, n)
    dims = [_check_page(i, p) for i, p in enumerate(pages)]
    if n == 0:
        return []
    S, Q = np.ascontiguousarray(ss, np.int32), np.ascontiguousarray(qs, np.int32)
    out, offs, nb, _ = _encode_batch(
        pages, dims, extra=(S, Q), encode=L.lib.rtn_jpeg_encode,
        bound=lambda i, w, hh, c: L.lib.rtn_jpeg_encode_bound(w, hh, c, ss[i]), slot=lambda b: b,
        workspace_bytes=lambda m, w, hh, c: L.lib.rtn_jpeg_encode_workspace_bytes(m, w, hh, c, S.ctypes.data))
    files = _files_to_host(out, offs, nb, [i for i in range(n) if nb[i] > 0], n)
    return [f if f is not None else _pillow_jpeg(pages[i], qs[i], ss[i]) for i, f in enumerate(files)]


def encode_png_bgr(pages):
    """PNG files of uint8 (H,W,3) B,G,R or (H,W) gray pages (CUDA or host tensors or arrays), lossless, in the chunked layout of
    DESIGN §3.4d that every PNG reader reads: one batched rtn_png_encode on the current stream (csrc/rtn_png_enc.hip), one small
    copy of the n file lengths, then one copy of the used bytes to pinned host memory.  There is no host path: a valid page
    always fits its slot (rtn_png_encode_bound).  Returns list[bytes]."""
    pages = list(pages)
    n = len(pages)
    dims = [_check_page(i, p) for i, p in enumerate(pages)]
    if n == 0:
        return []

    def bound(i, w, hh, c):
        b = L.lib.rtn_png_encode_bound(w, hh, c)
        if b == 0:
            raise ValueError("page %d: %dx%d is too large for one PNG stream" % (i, hh, w))
        return b

    out, offs, nb, bounds = _encode_batch(pages, dims, extra=(), encode=L.lib.rtn_png_encode, bound=bound, slot=lambda b: (b + 255) & ~255,
                                          workspace_bytes=L.lib.rtn_png_encode_workspace_bytes)
    if not all(0 < int(nb[i]) <= bounds[i] for i in range(n)):
        raise RuntimeError("rtn_png_encode: file lengths %s outside (0, bound]" % nb.tolist())
    return _files_to_host(out, offs, nb, list(range(n)), n)


TIFF_EXTENSIONS = ('.tif', '.tiff')
TIFF_ROWS_PER_STRIP = 64                                # the largest strip tiff_inspect takes for Group 4: the reader's one wave per 64 rows


def _check_tiff_settings(threshold, rows_per_strip, photometric, n):
    """(thresholds, rows per strip, photometrics) as lists of n ints, from ints or per-page sequences; ValueError for anything else."""
    def per_page(v, name, lo, hi):
        seq = isinstance(v, (list, tuple, np.ndarray))
        vs = list(v) if seq else [v] * n
        if len(vs) != n:
            raise ValueError("%d %s values for %d pages" % (len(vs), name, n))
        for x in (vs if seq else [v]):
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= x <= hi:
                raise ValueError("%s must be an integer %d..%d, got %r" % (name, lo, hi, x))
        return [int(x) for x in vs]
    return (per_page(threshold, "threshold", 1, 255), per_page(rows_per_strip, "rows_per_strip", 1, 65535),
            per_page(photometric, "photometric", 0, 1))


def encode_tiff_bgr(pages, threshold=128, rows_per_strip=TIFF_ROWS_PER_STRIP, photometric=0):
    """CCITT Group 4 (T.6) TIFF files of uint8 (H,W,3) B,G,R or (H,W) gray pages (CUDA or host tensors or arrays), thresholded on the
    device: ink is gray < threshold (gray as estimate_skew's, 1 <= threshold <= 255); photometric 0 (WhiteIsZero) or 1 (what Pillow's
    mode "1" writes by default); strips of rows_per_strip rows (1..65535; above the height: one strip).  The strips' bytes are those
    of Image.fromarray(gray >= threshold).save(f, "TIFF", compression="group4", tiffinfo={262: photometric, 278: rows_per_strip}).
    One batched rtn_tiff_encode on the current stream (csrc/rtn_tiff_enc.hip), one small copy of the n file lengths,
    then one copy of the used bytes to pinned host memory.  Every setting is an int or a sequence of one value per page.  The
    default of 64 rows per strip is the largest strip tiff_inspect takes for Group 4, so read_images_bgr decodes the files on the
    device, one wave per strip.  There is no host path: a valid page always fits its slot (rtn_tiff_encode_bound).  Returns
    list[bytes]."""
    pages = list(pages)
    n = len(pages)
    ts, rs, ps = _check_tiff_settings(threshold, rows_per_strip, photometric, n)
    dims = [_check_page(i, p) for i, p in enumerate(pages)]
    if n == 0:
        return []

    def bound(i, w, hh, c):
        b = L.lib.rtn_tiff_encode_bound(w, hh, rs[i])
        if b == 0:
            raise ValueError("page %d: %dx%d at %d rows per strip can give a TIFF of 4 GiB or more" % (i, hh, w, rs[i]))
        return b

    T, R, P = (np.ascontiguousarray(v, np.int32) for v in (ts, rs, ps))
    out, offs, nb, bounds = _encode_batch(
        pages, dims, extra=(T, R, P), encode=L.lib.rtn_tiff_encode, bound=bound, slot=lambda b: (b + 255) & ~255,
        workspace_bytes=lambda m, w, hh, c: L.lib.rtn_tiff_encode_workspace_bytes(m, w, hh, c, R.ctypes.data))
    if not all(0 < int(nb[i]) <= bounds[i] for i in range(n)):
        raise RuntimeError("rtn_tiff_encode: file lengths %s outside (0, bound]" % nb.tolist())
    return _files_to_host(out, offs, nb, list(range(n)), n)


def write_images_bgr(paths, pages, quality=95, subsampling=2, png="host", tiff="host"):
    """cv2.imwrite for a list of pages (uint8 (H,W,3) B,G,R or (H,W) gray; CUDA or host tensors or arrays): the .jpg / .jpeg /
    .jpe files through one encode_jpeg_bgr call (the device encoder), every other file through write_image, unchanged.
    png="device" sends the .png files through one encode_png_bgr call instead (lossless, other bytes than write_image's);
    png="host" (the default) leaves them with write_image.  tiff="g4" sends the .tif / .tiff files through one encode_tiff_bgr
    call with its defaults (bilevel: ink is gray < 128; Group 4, WhiteIsZero, 64 rows per strip); tiff="host" (the default)
    leaves them with write_image."""
    paths, pages = list(paths), list(pages)
    if png not in ("host", "device"):
        raise ValueError("png must be 'host' or 'device', got %r" % (png,))
    if tiff not in ("host", "g4"):
        raise ValueError("tiff must be 'host' or 'g4', got %r" % (tiff,))
    if len(paths) != len(pages):
        raise ValueError("%d paths for %d pages" % (len(paths), len(pages)))
    qs, ss = _check_settings(quality, subsampling, len(pages))
    for i, p in enumerate(pages):
        _check_page(i, p)
    ext = [os.path.splitext(str(path))[1].lower() for path in paths]
    jpg = [i for i, e in enumerate(ext) if e in JPEG_EXTENSIONS]
    dpng = [i for i, e in enumerate(ext) if e == ".png"] if png == "device" else []
    for i, data in zip(jpg, encode_jpeg_bgr([pages[i] for i in jpg], quality=[qs[i] for i in jpg], subsampling=[ss[i] for i in jpg])):
        with open(paths[i], 'wb') as f:
            f.write(data)
    for i, data in zip(dpng, encode_png_bgr([pages[i] for i in dpng])):
        with open(paths[i], 'wb') as f:
            f.write(data)
    g4 = [i for i, e in enumerate(ext) if e in TIFF_EXTENSIONS] if tiff == "g4" else []
    for i, data in zip(g4, encode_tiff_bgr([pages[i] for i in g4])):
        with open(paths[i], 'wb') as f:
            f.write(data)
    for i in sorted(set(range(len(paths))) - set(jpg) - set(dpng) - set(g4)):
        write_image(paths[i], _host_page(pages[i]))
