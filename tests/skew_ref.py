"""NumPy oracle of the skew estimator, written from its definition: gray by the scan analysis' rule, Otsu's threshold
in int64 sums and four float64 operations per candidate, ink = gray < t, ink counts per (row, band), a profile per shear factor from
bands shifted by floor(((b band + band/2 - W/2) T + 32768) / 65536), the sum of squared differences of neighbouring profile
entries, and the pick with its tie rule.  Also the rotation that deskews a page, through oracle/ref_generator.warp_affine_u8."""
from unittest import mock

import numpy as np

from oracle import ref_generator as G


def shears(max_angle=5.0, step=0.1):
    """(int32 shear factors, n_steps)."""
    n_steps = int(np.floor(max_angle / step + 1e-9))
    k = np.arange(-n_steps, n_steps + 1, dtype=np.float64)
    return np.rint(np.tan(np.radians(k * step)) * 65536.0).astype(np.int32), n_steps


def gray(page):
    page = np.asarray(page)
    if page.ndim == 2:
        return page.astype(np.int64)
    p = page.astype(np.int64)
    return (1868 * p[..., 0] + 9617 * p[..., 1] + 4899 * p[..., 2] + 8192) >> 14


def otsu(g):
    """The smallest t in 1..255 of the largest w0 w1 (m0/w0 - m1/w1)^2; 0 where no t splits the page."""
    h = np.bincount(g.reshape(-1), minlength=256).astype(np.int64)
    N, M = int(h.sum()), int((np.arange(256, dtype=np.int64) * h).sum())
    best_v, best_t = None, 0
    for t in range(1, 256):
        w0 = int(h[:t].sum())
        m0 = int((np.arange(t, dtype=np.int64) * h[:t]).sum())
        w1, m1 = N - w0, M - m0
        if w0 == 0 or w1 == 0:
            continue
        d = np.float64(m0) / np.float64(w0) - np.float64(m1) / np.float64(w1)
        v = ((np.float64(w0) * np.float64(w1)) * d) * d
        if best_v is None or v > best_v:
            best_v, best_t = v, t
    return best_t


def band_counts(ink, band):
    """(H, NB) int64: ink pixels of each row per band of `band` columns."""
    H, W = ink.shape
    nb = -(-W // band)
    padded = np.zeros((H, nb * band), np.int64)
    padded[:, :W] = ink
    return padded.reshape(H, nb, band).sum(axis=2)


def estimate(page, shear, threshold=0, band=32):
    """dict(threshold, ink, best, scores (uint64), counts) of one page."""
    g = gray(page)
    H, W = g.shape
    t = int(threshold) if threshold else otsu(g)
    ink = g < t
    C = band_counts(ink, band)
    nb = C.shape[1]
    K = len(shear)
    n_steps = K // 2
    cx = W // 2
    scores = np.zeros(K, np.uint64)
    for k in range(K):
        T = int(shear[k])
        P = np.zeros(H, np.int64)
        for b in range(nb):
            s = ((b * band + band // 2 - cx) * T + 32768) // 65536          # Python's floor division
            lo, hi = max(0, -s), min(H, H - s)                               # rows r with 0 <= r + s < H
            if lo < hi:
                P[lo:hi] += C[lo + s:hi + s, b]
        d = np.diff(P)
        scores[k] = np.uint64(int((d * d).sum()))
    order = sorted(range(K), key=lambda k: (-int(scores[k]), abs(k - n_steps), k))
    return dict(threshold=t, ink=int(ink.sum()), best=order[0], scores=scores, counts=C)


def angle(page, max_angle=5.0, step=0.1, threshold=0, band=32):
    """The skew in degrees."""
    sh, n_steps = shears(max_angle, step)
    return (estimate(page, sh, threshold, band)["best"] - n_steps) * step


def rotation_map(theta, height, width):
    """The destination->source map of the deskewing rotation by theta degrees about the page's centre, 2 x 3 float64."""
    t = np.radians(np.float64(theta))
    c, s = np.cos(t), np.sin(t)
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy]], np.float64)


def warp_with_map(page, inv_map, fill=255):
    """oracle/ref_generator.warp_affine_u8 (linear, constant border) with inv_map taken as the destination->source map it would derive
    from a forward matrix; a B,G,R page channel by channel, so that `fill` reaches every channel (the oracle's scalar border value
    fills the first channel only, as cv2's Scalar(cval) does)."""
    page = np.asarray(page)
    with mock.patch.object(G, "invert_affine", lambda m: np.array(m, np.float64)[:2].copy()):
        if page.ndim == 2:
            return G.warp_affine_u8(page, inv_map, interpolation=1, border_mode=0, cval=fill)
        return np.stack([G.warp_affine_u8(np.ascontiguousarray(page[..., c]), inv_map, interpolation=1, border_mode=0, cval=fill)
                         for c in range(page.shape[2])], axis=-1)


def deskew(page, theta, fill=255):
    """The page rotated upright, given its skew theta in degrees."""
    return warp_with_map(page, rotation_map(theta, page.shape[0], page.shape[1]), fill)


def skewed(page, theta, fill=255):
    """A page whose text lines run at theta degrees (the estimator's sign): the upright page under the inverse rotation."""
    return warp_with_map(page, rotation_map(-theta, page.shape[0], page.shape[1]), fill)
