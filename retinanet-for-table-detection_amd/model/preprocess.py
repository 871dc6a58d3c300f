"""Page preprocessing of the reference on the device: DetectTablesUtils.preProcessSampleImages (DetectTablesUtils.py:229-261)
and utils.resize_image's cv2.resize (model/utils.py:152), plus Generator.compute_inputs' zero-padded batch
(csv_generator.py:320-336)."""
import numpy as np
import torch

from . import _pages, _rt
from ._pages import i32, pointers
from .page_io import read_images_bgr, write_images_bgr

L = _rt.L


def preprocess_pages(pages, return_binary=False):
    """pages: uint8 (B,H,W,3) BGR or (B,H,W) gray, or one (H,W[,3]) page.  Returns uint8 (B,H,W,3): b=L2, g=L1, r=C distance
    maps of the Gaussian adaptive threshold, saturated to uint8 as cv2.imwrite stores them."""
    a = np.asarray(pages)
    single = a.ndim == 2 or (a.ndim == 3 and a.shape[-1] == 3)        # one gray (H,W) or one BGR (H,W,3) page
    if single:
        a = a[None]
    ch = 3 if a.ndim == 4 else 1
    if a.dtype != np.uint8:
        raise ValueError("pages must be uint8")
    B, H, W = a.shape[:3]
    h = _rt.handle()
    src = _rt.dev(a, torch.uint8)
    dst = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
    binary = torch.empty(B, H, W, dtype=torch.uint8, device="cuda")
    wsb = L.lib.rtn_preprocess_dt3_workspace_bytes(B, H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    h.check(L.lib.rtn_preprocess_dt3(h.raw, src.data_ptr(), ch, B, H, W, dst.data_ptr(), binary.data_ptr(), ws.data_ptr(), wsb))
    out, bo = _rt.host(dst), _rt.host(binary)
    if single:
        out, bo = out[0], bo[0]
    return (out, bo) if return_binary else out


def preprocess_files(src_paths, dst_paths, quality=95, png="host"):
    """DetectTablesUtils.preProcessSampleImages / preProcessTrainValImages as a batch: read every page (page_io.read_images_bgr:
    baseline JPEGs decoded on the device), run rtn_preprocess_dt3 on the device (one call per page size), and write the distance
    maps (page_io.write_images_bgr: .jpg / .jpeg / .jpe names encoded on the device at `quality`, 4:2:0, other names through
    write_image; png="device" encodes the .png names on the device too, page_io.encode_png_bgr).  On the JPEG -> JPEG path, and
    with png="device" on the JPEG -> PNG and PNG -> PNG paths, the processed pixels never come to the host.  A page wider than
    rtn_preprocess_dt3 takes raises what preprocess_pages raises for it."""
    src_paths, dst_paths = list(src_paths), list(dst_paths)
    if png not in ("host", "device"):
        raise ValueError("png must be 'host' or 'device', got %r" % (png,))
    if len(src_paths) != len(dst_paths):
        raise ValueError("%d source paths for %d destination paths" % (len(src_paths), len(dst_paths)))
    if not src_paths:
        return
    write_images_bgr(dst_paths, preprocess_device_pages(read_images_bgr(src_paths)), quality=quality, png=png)


def binarize_files(src_paths, dst_paths, tiff="g4"):
    """Scan to archive: read every page (page_io.read_images_bgr), take the Gaussian adaptive threshold of each
    (preprocess_pages(return_binary=True), one call per page size) and write the binary pages (page_io.write_images_bgr).  With
    tiff="g4" (the default) the .tif / .tiff names become CCITT Group 4 TIFFs of 64 rows per strip, encoded on the device
    (page_io.encode_tiff_bgr), which read_images_bgr decodes there; tiff="host" leaves them with write_image."""
    src_paths, dst_paths = list(src_paths), list(dst_paths)
    if tiff not in ("host", "g4"):
        raise ValueError("tiff must be 'host' or 'g4', got %r" % (tiff,))
    if len(src_paths) != len(dst_paths):
        raise ValueError("%d source paths for %d destination paths" % (len(src_paths), len(dst_paths)))
    if not src_paths:
        return
    pages = read_images_bgr(src_paths)
    groups = {}
    for i, p in enumerate(pages):
        groups.setdefault(tuple(p.shape[:2]), []).append(i)
    out = [None] * len(pages)
    for idx in groups.values():
        binary = preprocess_pages(torch.stack([pages[i] for i in idx]).cpu().numpy(), return_binary=True)[1]
        for k, i in enumerate(idx):
            out[i] = binary[k]
    write_images_bgr(dst_paths, out, tiff=tiff)


def preprocess_device_pages(pages):
    """The distance maps of a list of CUDA uint8 (H,W,3) B,G,R pages of any sizes, as CUDA uint8 (H,W,3) tensors in the same order:
    rtn_preprocess_dt3 on the current stream, one call per page size.  No pixel comes to the host."""
    pages = list(pages)
    if not pages:
        return []
    h = _rt.handle()
    groups = {}
    for i, p in enumerate(pages):
        groups.setdefault(tuple(p.shape[:2]), []).append(i)
    out = [None] * len(pages)
    for (H, W), idx in groups.items():
        for k0 in range(0, len(idx), 21845):                    # rtn_preprocess_dt3 takes B * 3 <= 65535
            part = idx[k0:k0 + 21845]
            B = len(part)
            src = torch.stack([pages[i] for i in part]) if B > 1 else pages[part[0]][None]
            dst = torch.empty(B, H, W, 3, dtype=torch.uint8, device=src.device)
            wsb = L.lib.rtn_preprocess_dt3_workspace_bytes(B, H, W)
            ws = torch.empty(wsb, dtype=torch.uint8, device=src.device)
            h.check(L.lib.rtn_preprocess_dt3(h.raw, src.data_ptr(), 3, B, H, W, dst.data_ptr(), None, ws.data_ptr(), wsb))
            for k, i in enumerate(part):
                out[i] = dst[k]
    return out


# ---- DetectTablesUtils.interpolateImages (DetectTablesUtils.py:296-316) on the device: csrc/rtn_resize_u8.hip, DESIGN §3.4k --------------
RESIZE_MAX_SIDE = 65500


def interpolation_factor(name):
    """The factor interpolateImages enlarges a low-resolution scan by, from its file name: 4.17 for names ending "-72.jpg", 3 for
    "-100.jpg" (72- and 100-dpi pages), 1.0 for every other name.  The reference keeps the last factor for the following files that
    have neither suffix, in os.listdir order; that is not reproduced: a name without a suffix always gives 1.0."""
    name = str(name)
    if name.endswith("-72.jpg"):
        return 4.17
    if name.endswith("-100.jpg"):
        return 3.0
    return 1.0


def interpolated_size(height, width, fx, fy=None):
    """(Ho, Wo) of cv2.resize(..., fx=fx, fy=fy): saturate_cast<int> of the products, half to even.  ValueError where a side
    leaves 1 .. 65500."""
    fy = fx if fy is None else fy
    ho, wo = int(np.rint(height * float(fy))), int(np.rint(width * float(fx)))
    if not (1 <= ho <= RESIZE_MAX_SIDE and 1 <= wo <= RESIZE_MAX_SIDE):
        raise ValueError("%dx%d by (%g, %g) gives %dx%d: sides must be 1..%d" % (height, width, fx, fy, ho, wo, RESIZE_MAX_SIDE))
    return ho, wo


def _per_page(v, n, name):
    if isinstance(v, (list, tuple, np.ndarray)) and not (name == "dsize" and len(v) == 2 and np.ndim(v[0]) == 0):
        v = list(v)
        if len(v) != n:
            raise ValueError("%d %s values for %d pages" % (len(v), name, n))
        return v
    return [v] * n


def interpolate_images(pages, fx=None, fy=None, dsize=None):
    """cv2.resize(page, None, fx=fx, fy=fy, interpolation=cv2.INTER_CUBIC) of a list of uint8 (H,W,3) or (H,W) pages (NumPy arrays or
    CUDA tensors, sizes may differ), as interpolateImages applies it to low-resolution scans; with dsize, cv2.resize(page, dsize,
    interpolation=cv2.INTER_CUBIC) instead.  fx, fy: scalars or one value per page, fy defaults to fx.  dsize: (width, height) for
    all pages or one pair per page; fx and fy are then not taken.  One rtn_resize_u8 launch on the current stream resizes the whole
    batch; pages already on the device are not copied to the host.  Returns a list of CUDA uint8 tensors.  The arithmetic is
    OpenCV's 8-bit fixed-point form as recalled (csrc/rtn_resize_u8.h)."""
    if dsize is not None:
        if fx is not None or fy is not None:
            raise ValueError("either factors or dsize, not both")
    elif fx is None:
        raise ValueError("fx or dsize is required")
    src, shapes = _pages.check_pages(pages, 1, RESIZE_MAX_SIDE)
    n = len(src)
    if n == 0:
        return []
    sizes, inv_x, inv_y = [], [], []
    if dsize is not None:
        for p, d in zip(src, _per_page(dsize, n, "dsize")):
            wo, ho = int(d[0]), int(d[1])
            if not (1 <= ho <= RESIZE_MAX_SIDE and 1 <= wo <= RESIZE_MAX_SIDE):
                raise ValueError("dsize %s: sides must be 1..%d" % ((wo, ho), RESIZE_MAX_SIDE))
            sizes.append((ho, wo))
            inv_x.append(p.shape[1] / float(wo))
            inv_y.append(p.shape[0] / float(ho))
    else:
        fxs = _per_page(fx, n, "fx")
        fys = fxs if fy is None else _per_page(fy, n, "fy")
        for p, a, b in zip(src, fxs, fys):
            a, b = float(a), float(b)
            if not (np.isfinite(a) and np.isfinite(b) and a > 0 and b > 0):
                raise ValueError("factors must be positive and finite, got (%r, %r)" % (a, b))
            sizes.append(interpolated_size(p.shape[0], p.shape[1], a, b))
            inv_x.append(1.0 / a)
            inv_y.append(1.0 / b)
    be = _pages.Device(src[0].device)
    outs = [torch.empty((ho, wo) + tuple(p.shape[2:]), dtype=torch.uint8, device=p.device) for p, (ho, wo) in zip(src, sizes)]
    arrays = (i32([s[0] for s in shapes]), i32([s[1] for s in shapes]), i32([s[2] for s in shapes]),
              i32([s[0] for s in sizes]), i32([s[1] for s in sizes]), np.ascontiguousarray(inv_x, np.float64),
              np.ascontiguousarray(inv_y, np.float64))
    be.call("rtn_resize_u8", [n, pointers(be, src), *[a.ctypes.data for a in arrays], pointers(be, outs)],
            lambda: L.lib.rtn_resize_u8_workspace_bytes(n))
    return outs                                                 # queued on the current stream, like the sources' uploads


def interpolate_files(src_paths, dst_paths, factors=None, quality=95, png="host"):
    """DetectTablesUtils.interpolateImages as a batch: read every page (page_io.read_images_bgr), enlarge all of them in one
    rtn_resize_u8 launch (interpolate_images) and write them (page_io.write_images_bgr: .jpg names encoded on the device at
    `quality`, 4:2:0, cv2.imwrite's defaults; png="device" encodes the .png names on the device too).  factors: one per file, by
    default interpolation_factor of the source's base name (4.17 / 3 / 1.0; a factor of 1 copies the page).  On the JPEG -> JPEG
    path no pixel comes to the host."""
    import os
    src_paths, dst_paths = list(src_paths), list(dst_paths)
    if png not in ("host", "device"):
        raise ValueError("png must be 'host' or 'device', got %r" % (png,))
    if len(src_paths) != len(dst_paths):
        raise ValueError("%d source paths for %d destination paths" % (len(src_paths), len(dst_paths)))
    if factors is None:
        factors = [interpolation_factor(os.path.basename(str(p))) for p in src_paths]
    factors = _per_page(factors, len(src_paths), "factors")
    if not src_paths:
        return
    write_images_bgr(dst_paths, interpolate_images(read_images_bgr(src_paths), factors), quality=quality, png=png)


# ---- skew of a scanned page: csrc/rtn_skew.hip, DESIGN §3.4m ------------------------------------------------------------------------------
SKEW_MAX_SIDE, SKEW_MAX_ANGLE, SKEW_MAX_ANGLES, SKEW_MAX_SHEAR = 32767, 15.0, 401, 17561


def skew_shears(max_angle=5.0, step=0.1):
    """(shear_q16, n_steps) of rtn_skew_estimate: entry k is rint(tan(radians((k - n_steps) * step)) * 65536) in float64, with
    n_steps = floor(max_angle / step + 1e-9).  ValueError for max_angle > 15, a step that is not positive, or more than 401 angles."""
    max_angle, step = float(max_angle), float(step)
    if not (np.isfinite(max_angle) and np.isfinite(step) and step > 0 and 0 <= max_angle <= SKEW_MAX_ANGLE):
        raise ValueError("max_angle must be 0..%g degrees and step positive, got (%r, %r)" % (SKEW_MAX_ANGLE, max_angle, step))
    n_steps = int(np.floor(max_angle / step + 1e-9))
    if 2 * n_steps + 1 > SKEW_MAX_ANGLES:
        raise ValueError("%d angles: at most %d" % (2 * n_steps + 1, SKEW_MAX_ANGLES))
    k = np.arange(-n_steps, n_steps + 1, dtype=np.float64)
    shear = np.rint(np.tan(np.radians(k * step)) * 65536.0).astype(np.int32)
    if np.abs(shear).max() > SKEW_MAX_SHEAR:
        raise ValueError("a shear factor beyond 15 degrees")
    return np.ascontiguousarray(shear), n_steps


def _estimate_skew(src, max_angle, step, threshold, band, return_scores):
    if band not in (8, 16, 32, 64):
        raise ValueError("band must be 8, 16, 32 or 64, got %r" % (band,))
    threshold = 0 if threshold is None else int(threshold)
    if not 0 <= threshold <= 255:
        raise ValueError("threshold must be None (Otsu) or 1..255, got %r" % (threshold,))
    shear, n_steps = skew_shears(max_angle, step)
    n, K = len(src), len(shear)
    if n > 65535:
        raise ValueError("at most 65535 pages a call")
    if n == 0:
        return ([], []) if return_scores else []
    hs, wd, ch = i32([p.shape[0] for p in src]), i32([p.shape[1] for p in src]), i32([3 if p.dim() == 3 else 1 for p in src])
    be = _pages.Device(src[0].device)
    # one result block: scores (uint64 [n][K]), ink (int64 [n]), thresholds and best (int32 [n] each), read back in one copy
    res = torch.empty(n * K + n + n, dtype=torch.int64, device=be.dev)
    scores_ptr = res.data_ptr()
    ink_ptr = scores_ptr + 8 * n * K
    thr_ptr = ink_ptr + 8 * n
    best_ptr = thr_ptr + 4 * n
    be.call("rtn_skew_estimate", [n, pointers(be, src), hs.ctypes.data, wd.ctypes.data, ch.ctypes.data, threshold, band, K, shear.ctypes.data,
                                  thr_ptr, ink_ptr, best_ptr, scores_ptr],
            lambda: L.lib.rtn_skew_workspace_bytes(n, hs.ctypes.data, wd.ctypes.data, band, K))
    host = res.cpu().numpy()                                      # the single read-back
    scores = host[:n * K].view(np.uint64).reshape(n, K)
    ink = host[n * K:n * K + n]
    small = host[n * K + n:].view(np.int32)
    thr, best = small[:n], small[n:2 * n]
    angles = [float((int(b) - n_steps) * float(step)) for b in best]
    if return_scores:
        return angles, [dict(threshold=int(t), ink=int(i), best=int(b), scores=s.copy()) for t, i, b, s in zip(thr, ink, best, scores)]
    return angles


def estimate_skew(pages, max_angle=5.0, step=0.1, threshold=None, band=32, return_scores=False):
    """The skew angle of every page in degrees: a list of uint8 (H,W,3) B,G,R or (H,W) gray pages (NumPy arrays or CUDA tensors, sizes
    may differ, sides 1..32767), swept over the angles (k - n_steps) * step, k = 0 .. 2 n_steps, n_steps = floor(max_angle / step +
    1e-9), by rtn_skew_estimate on the current stream: one call for the batch, one read-back of the small result block.  Ink is
    gray < threshold; threshold=None takes Otsu's of each page.  band: the width of a column band, 8, 16, 32 or 64.  Ink of a text
    line of a page of angle a lies along y = y0 + (x - W/2) tan(a), y down.  With return_scores, (angles, details): per page a dict of
    threshold, ink, best and the uint64 scores of all angles.  ValueError for max_angle > 15, more than 401 angles, a bad band or
    bad pages."""
    return _estimate_skew(_pages.check_pages(pages, 1, SKEW_MAX_SIDE)[0], max_angle, step, threshold, band, return_scores)


def deskew_map(angle, height, width):
    """The destination->source map of deskew_images, 2 x 3 float64: the rotation by `angle` degrees about ((W-1)/2, (H-1)/2)."""
    t = np.radians(float(angle))
    c, s = np.cos(t), np.sin(t)
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy]], np.float64)


def deskew_images(pages, max_angle=5.0, step=0.1, threshold=None, band=32, fill=255, min_angle=None):
    """estimate_skew, then every page whose angle is at least min_angle (default: step) in magnitude rotated upright into a canvas of its
    own size by rtn_warp_affine_u8 (INTER_LINEAR, constant border `fill` in every channel) with deskew_map as the destination->source
    map.  Returns (pages, angles): CUDA uint8 tensors and degrees.  A page below min_angle is returned as the tensor it came in as (a
    NumPy page: as its upload).  No pixel comes to the host."""
    import ctypes as C
    src = _pages.check_pages(pages, 1, SKEW_MAX_SIDE)[0]
    angles = _estimate_skew(src, max_angle, step, threshold, band, False)
    min_angle = float(step) if min_angle is None else float(min_angle)
    fill = int(fill)
    if not 0 <= fill <= 255:
        raise ValueError("fill must be 0..255, got %r" % (fill,))
    cval = np.full(4, fill, np.uint8)
    h = _rt.handle()
    out = []
    for p, a in zip(src, angles):
        if abs(a) < min_angle:
            out.append(p)
            continue
        H, W = int(p.shape[0]), int(p.shape[1])
        inv = np.ascontiguousarray(deskew_map(a, H, W))
        dst = torch.empty_like(p)
        h.check(L.lib.rtn_warp_affine_u8(h.raw, p.data_ptr(), H, W, 3 if p.dim() == 3 else 1, inv.ctypes.data_as(C.c_void_p), 1, 0,
                                         cval.ctypes.data_as(C.c_void_p), dst.data_ptr()))
        out.append(dst)
    return out, angles


def deskew_files(src_paths, dst_paths, max_angle=5.0, step=0.1, threshold=None, band=32, fill=255, min_angle=None, quality=95, png="host",
                 tiff="host"):
    """Read every page (page_io.read_images_bgr), deskew all of them (deskew_images) and write them (page_io.write_images_bgr: .jpg
    names encoded on the device at `quality`, 4:2:0; png="device" encodes the .png names on the device too; tiff="g4" writes the
    .tif / .tiff names as bilevel Group 4 TIFFs on the device).  Returns the angles."""
    src_paths, dst_paths = list(src_paths), list(dst_paths)
    if png not in ("host", "device"):
        raise ValueError("png must be 'host' or 'device', got %r" % (png,))
    if tiff not in ("host", "g4"):
        raise ValueError("tiff must be 'host' or 'g4', got %r" % (tiff,))
    if len(src_paths) != len(dst_paths):
        raise ValueError("%d source paths for %d destination paths" % (len(src_paths), len(dst_paths)))
    if not src_paths:
        return []
    out, angles = deskew_images(read_images_bgr(src_paths), max_angle, step, threshold, band, fill, min_angle)
    write_images_bgr(dst_paths, out, quality=quality, png=png, tiff=tiff)
    return angles


def boxes_to_scan(boxes, angle, height, width):
    """Boxes (x1, y1, x2, y2) found on a page that deskew_images rotated by `angle` degrees, mapped back to the scan of height x width:
    the axis-aligned hull of the four corners under deskew_map (transform.transform_aabb).  Host arithmetic; returns float64 (n, 4)."""
    from .transform import transform_aabb
    m = np.vstack([deskew_map(angle, height, width), [0.0, 0.0, 1.0]])
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    return np.array([transform_aabb(m, row) for row in b], np.float64).reshape(-1, 4)


def resize_cubic(img, scale):
    """cv2.resize(img, None, fx=scale, fy=scale, interpolation=cv2.INTER_CUBIC) of a float32 (H,W,C) image."""
    img = np.asarray(img, np.float32)
    if img.ndim == 2:
        return resize_cubic(img[..., None], scale)[..., 0]
    H, W, Cc = img.shape
    Ho, Wo = int(np.rint(H * scale)), int(np.rint(W * scale))
    h = _rt.handle()
    s = _rt.dev(img, torch.float32)
    out = torch.empty(Ho, Wo, Cc, dtype=torch.float32, device="cuda")
    h.check(L.lib.rtn_resize_cubic(h.raw, s.data_ptr(), L.RTN_F32, H, W, Cc, float(scale), out.data_ptr(), L.RTN_F32, Ho, Wo, Wo * Cc))
    return _rt.host(out)


def compute_inputs_device(processed_u8_pages, min_side=800, max_side=1333, dtype=torch.bfloat16):
    """csv_generator.Generator: preprocess_group + compute_inputs on the device.  processed_u8_pages: list of uint8 (H,W,3)
    distance-map pages (any sizes).  Normalises (x/127.5-1), resizes each page by its own scale (INTER_CUBIC) and writes it
    into the top-left of a zero canvas of the largest resized shape.  Returns (device tensor (B,Hmax,Wmax,3), scales)."""
    from .utils import compute_resize_scale
    h = _rt.handle()
    scales = [compute_resize_scale(p.shape, min_side, max_side) for p in processed_u8_pages]
    shapes = [(int(np.rint(p.shape[0] * s)), int(np.rint(p.shape[1] * s))) for p, s in zip(processed_u8_pages, scales)]
    Hm, Wm = max(s[0] for s in shapes), max(s[1] for s in shapes)
    canvas = torch.zeros(len(shapes), Hm, Wm, 3, dtype=dtype, device="cuda")
    code = L.RTN_BF16 if dtype == torch.bfloat16 else L.RTN_F32
    keep = []
    for i, (p, s, (ho, wo)) in enumerate(zip(processed_u8_pages, scales, shapes)):
        src = _rt.dev(p, torch.uint8)
        keep.append(src)
        h.check(L.lib.rtn_resize_cubic(h.raw, src.data_ptr(), 2, p.shape[0], p.shape[1], 3, float(s), canvas[i].data_ptr(), code, ho, wo, Wm * 3))
    torch.cuda.synchronize()
    return canvas, scales
