"""NumPy oracle of header detection, stages 1-5, written from the stage definitions and HeaderDetect.py: the box
resample, OpenCV's 8-bit BGR2HSV / HSV2BGR (restated from its published source: recalled, not verifiable offline), the k-means
chain for k = 1 .. 9, analyse() on the raw pixel lists, and extractPatch.  No code is shared with the package."""
import colorsys

import numpy as np

W = 500
MAX_K = 9
F = np.float32

_SDIV = np.array([0] + [int(np.rint((255 << 12) / (1.0 * i))) for i in range(1, 256)], np.int64)
_HDIV = np.array([0] + [int(np.rint((180 << 12) / (6.0 * i))) for i in range(1, 256)], np.int64)


def bgr2hsv(bgr):
    """cv2.cvtColor(BGR2HSV) of uint8 (..., 3): RGB2HSV_b with hrange 180 and the 12-bit sdiv / hdiv tables."""
    a = np.asarray(bgr).astype(np.int64)
    b, g, r = a[..., 0], a[..., 1], a[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = (diff * _SDIV[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * _HDIV[diff] + 2048) >> 12
    h = h + np.where(h < 0, 180, 0)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def hsv2bgr(hsv):
    """cv2.cvtColor(HSV2BGR) of uint8 (..., 3): HSV2RGB_b over HSV2RGB_native, float32, one operation at a time."""
    a = np.asarray(hsv)
    h = a[..., 0].astype(F)
    s = a[..., 1].astype(F) * F(1.0 / 255.0)
    v = a[..., 2].astype(F) * F(1.0 / 255.0)
    h = h * (F(6.0) / F(180.0))
    h = np.where(h >= F(6.0), h - F(6.0), h)
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(F)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, F(0), h)
    one = F(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1)
    sector_data = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    pick = sector_data[sector]
    out = np.take_along_axis(tab, pick, axis=-1)
    out = np.where((a[..., 1] == 0)[..., None], v[..., None], out)
    assert out.dtype == F
    return np.clip(np.rint(out * F(255.0)), 0, 255).astype(np.uint8)


def _overlaps(src_n, dst_n):
    """(dst_n, src_n) int64: the overlap of destination cell [src_n * X, src_n * (X + 1)) with source cell [dst_n * i, dst_n * (i + 1))."""
    X = np.arange(dst_n, dtype=np.int64)[:, None] * src_n
    i = np.arange(src_n, dtype=np.int64)[None, :] * dst_n
    return np.clip(np.minimum(X + src_n, i + dst_n) - np.maximum(X, i), 0, None)


def sampled_height(h, w):
    return int(h * (W / float(w)))


def box_resample(img, dh):
    """The dh x 500 box filter of a uint8 (h, w, 3) image in 64-bit integers: (2 * sum(src * wx * wy) + w * h) // (2 * w * h)."""
    h, w = img.shape[:2]
    wy, wx = _overlaps(h, dh), _overlaps(w, W)
    acc = np.einsum("Yj,jic,Xi->YXc", wy, img.astype(np.int64), wx, optimize=True)
    return ((2 * acc + w * h) // (2 * w * h)).astype(np.uint8)


def sample(img):
    """Stage 1: the (dh, 500, 3) H,S,V image of a crop, or None where dh = 0."""
    dh = sampled_height(*img.shape[:2])
    return bgr2hsv(box_resample(img, dh)) if dh >= 1 else None


def _dist(p, c):
    """((H - c0)^2 + (S - c1)^2) + (V - c2)^2 in float32; p: (N, 3) float32, c: (3,) float32."""
    a, b, e = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
    return (a * a + b * b) + e * e


def _assign(p, cen):
    d = np.stack([_dist(p, c) for c in cen], axis=1)
    lab = np.argmin(d, axis=1)                          # the first of equal minima
    return lab, d[np.arange(len(p)), lab]


def _sums(pts, lab, k):
    n = np.bincount(lab, minlength=k).astype(np.int64)
    s = np.stack([np.bincount(lab, weights=None if False else pts[:, c], minlength=k) for c in range(3)], axis=1)
    q = np.stack([np.bincount(lab, weights=pts[:, c] * pts[:, c], minlength=k) for c in range(3)], axis=1)
    return n, s.astype(np.int64), q.astype(np.int64)    # float64 weights hold these integers exactly (< 2^53)


def _split(cen, n, s, q):
    k = len(cen)
    sse = np.zeros(k)
    for j in range(k):
        if n[j]:
            t = float(s[j, 0]) * float(s[j, 0]) + float(s[j, 1]) * float(s[j, 1])
            t = t + float(s[j, 2]) * float(s[j, 2])
            sse[j] = float(int(q[j].sum())) - t / float(n[j])
    js = int(np.argmax(sse))
    var = np.zeros(3)
    if n[js]:
        for c in range(3):
            m = float(s[js, c]) / float(n[js])
            var[c] = float(q[js, c]) / float(n[js]) - m * m
    cs = int(np.argmax(var))
    e = F(np.sqrt(max(var[cs], 0.0)))
    new = cen[js].copy()
    cen = np.concatenate([cen, new[None]], axis=0)
    cen[k, cs] = cen[js, cs] + e
    cen[js, cs] = cen[js, cs] - e
    return cen


def kmeans_chain(hsv_points, max_iter=300):
    """Stage 2 for one crop's (N, 3) uint8 points -> per k (list of 9): centres (k, 3) float32, counts (k,), passes, labels (N,)
    uint8, distortion_fx (Python int)."""
    pts = hsv_points.astype(np.int64)
    p = hsv_points.astype(F)
    out = []
    cen = np.zeros((1, 3), F)
    n = s = q = None
    for k in range(1, MAX_K + 1):
        if k > 1:
            cen = _split(cen, n, s, q)
        prev, passes = None, 0
        for it in range(1, max_iter + 1):
            lab, _ = _assign(p, cen)
            changed = prev is None or bool(np.any(lab != prev))
            prev = lab
            n, s, q = _sums(pts, lab, k)
            for j in range(k):
                if n[j]:
                    cen[j] = (s[j].astype(np.float64) / np.float64(n[j])).astype(F)
            passes = it
            if not changed:
                break
        _, d = _assign(p, cen)
        assert d.dtype == F
        fx = int(np.rint(np.sqrt(d) * F(65536.0)).astype(np.int64).sum())
        out.append({"centres": cen.copy(), "counts": n.copy(), "passes": passes, "labels": prev.astype(np.uint8), "distortion_fx": fx})
    return out


def opt_k(distortions):
    """optK of the reference, restated."""
    d = [x / 100. for x in distortions]
    d1 = [d[i] - d[i + 1] for i in range(len(d) - 1)]
    d2 = [d1[i] - d1[i + 1] for i in range(len(d1) - 1)]
    strength = [0] + [round(d2[i - 1] - d1[i], 3) for i in range(1, len(d) - 1)] + [0]
    return strength.index(max(strength)) + 1 if max(strength) > 0 else None


def histograms(hsv_points, labels):
    """(9, 3, 256) uint32: the histogram of every channel of every cluster."""
    hist = np.zeros((MAX_K, 3, 256), np.uint32)
    for j in range(MAX_K):
        for c in range(3):
            hist[j, c] = np.bincount(hsv_points[labels == j, c], minlength=256)
    return hist


def analyse(color_list):
    """analyse() of the reference for one cluster's raw (n, 3) uint8 list."""
    return {"min_value": np.min(color_list, axis=0), "max_value": np.max(color_list, axis=0),
            "Mean": np.mean(color_list, axis=0).astype(int), "Std": np.std(color_list, axis=0).astype(int),
            "Q1": np.quantile(color_list, 0.25, axis=0), "Q3": np.quantile(color_list, 0.75, axis=0),
            "Median": np.median(color_list, axis=0)}


def in_range_mask(hsv_img, lo, hi):
    return np.all((hsv_img >= lo) & (hsv_img <= hi), axis=-1)


def dilate3(mask):
    """Any pixel of the 3x3 neighbourhood, clipped to the image."""
    h, w = mask.shape
    p = np.zeros((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = mask
    out = np.zeros_like(mask)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def patch(hsv_img, lo, hi):
    """extractPatch on the sampled H,S,V image: H,S,V kept where the blurred inRange mask is non-zero, 0,0,0 elsewhere, HSV2BGR."""
    keep = dilate3(in_range_mask(hsv_img, np.asarray(lo, np.uint8), np.asarray(hi, np.uint8)))
    return hsv2bgr(np.where(keep[..., None], hsv_img, 0).astype(np.uint8))


def detect(crop, k=None, max_iter=300, chain=None):
    """Stages 1-5 for one crop -> what detect_headers returns for it (patches as arrays).  chain: a kmeans_chain result to reuse."""
    hsv = sample(crop)
    if hsv is None:
        return None
    pts = hsv.reshape(-1, 3)
    fits = chain if chain is not None else kmeans_chain(pts, max_iter)
    distortions = [f["distortion_fx"] / 65536 / len(pts) for f in fits]
    kk = int(k) if k is not None else (opt_k(distortions) or 5)
    fit = fits[kk - 1]
    total = int(fit["counts"].sum())
    order = sorted((j for j in range(kk) if fit["counts"][j] > 0), key=lambda j: (-int(fit["counts"][j]), j))
    dominant = []
    for j in order:
        c = [float(x) for x in fit["centres"][j]]
        dominant.append({"cluster_index": j, "HSV_color": c,
                         "RGB_color": np.array([int(round(x * 255)) for x in colorsys.hsv_to_rgb(c[0] / 255., c[1] / 255., c[2] / 255.)]),
                         "color_percentage": int(fit["counts"][j]) / total})
    clusters, patches = [], []
    for j in range(kk):
        if fit["counts"][j] == 0:
            continue
        info = {"cluster_index": j}
        info.update(analyse(pts[fit["labels"] == j]))
        info["selected"] = bool(info["Q3"][0] - info["Q1"][0] < 20)
        clusters.append(info)
        lo = np.array(np.clip(info["Q1"], 0, 255), dtype=np.uint8)
        hi = np.array(np.clip(info["Q3"], 0, 255), dtype=np.uint8)
        patches.append(patch(hsv, lo, hi))
    return {"distortions": distortions, "k": kk, "passes": [f["passes"] for f in fits], "dominant": dominant, "clusters": clusters,
            "patches": patches, "hsv": hsv, "fits": fits}
