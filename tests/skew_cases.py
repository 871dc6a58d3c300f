"""The pages and sweeps the tests of the skew estimator share (tests/test_skew_host.py, test_gpu_skew.py), and the oracle's result
for each (tests/skew_ref.py), computed once per process.  One mixed batch of pages, gray and B,G,R, holds the smallest shapes at
which the kernels can go wrong; it runs under every sweep of SWEEPS (band width, angles, threshold)."""
import ctypes as C
import functools
import importlib
import os

import numpy as np

import skew_ref as R

L = importlib.import_module("retinanet-for-table-detection_amd")._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (max_angle, step, threshold (0 = Otsu), band)
SWEEPS = {
    "band32_otsu": (5.0, 0.1, 0, 32),
    "band8_otsu": (5.0, 0.1, 0, 8),
    "band16_otsu": (5.0, 0.1, 0, 16),
    "band64_otsu": (5.0, 0.1, 0, 64),
    "band32_15deg_otsu": (15.0, 0.1, 0, 32),                    # K = 301: shifts larger than the height of the low pages
    "band32_401_fixed128": (10.0, 0.05, 128, 32),               # K = 401, the most
    "band16_fixed200": (5.0, 0.1, 200, 16),
}


def text_lines(h, w, seed, pitch=None, channels=1):
    """Synthetic text: dark bars 6 rows high in word-length pieces on light paper with a little noise, the line pitch 14..22 rows."""
    rng = np.random.default_rng(seed)
    img = (236 + rng.integers(-6, 7, (h, w))).astype(np.int64)
    pitch = int(rng.integers(14, 23)) if pitch is None else pitch
    margin = max(2, w // 12)
    for y in range(int(rng.integers(4, 12)), h - 8, pitch):
        x = margin + int(rng.integers(0, 6))
        end = w - margin - (int(rng.integers(0, w // 3)) if rng.random() < 0.3 else 0)
        while x < end:
            word = int(rng.integers(12, 60))
            img[y:y + 6, x:min(x + word, end)] = rng.integers(15, 60, img[y:y + 6, x:min(x + word, end)].shape)
            x += word + int(rng.integers(5, 12))
    img = np.clip(img, 0, 255).astype(np.uint8)
    if channels == 3:
        tint = np.stack([img, np.clip(img.astype(np.int64) - 3, 0, 255).astype(np.uint8), np.clip(img.astype(np.int64) + 4, 0, 255).astype(np.uint8)], axis=-1)
        return np.ascontiguousarray(tint)
    return img


def random_page(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3) if c == 3 else (h, w), dtype=np.uint8)


def v_page():
    """384 wide and symmetric about its centre column: the lines of the left half run at +3 degrees, those of the right half mirror
    them.  The scores at +k and -k are equal and the largest lie off the centre: the pick's last rule decides."""
    left = R.skewed(text_lines(90, 384, 31, pitch=15), 3.0)[:, :192]
    return np.ascontiguousarray(np.concatenate([left, left[:, ::-1]], axis=1))


@functools.lru_cache(maxsize=None)
def pages():
    """name -> page, in the order of the mixed batch."""
    out = {
        "one_pixel": np.array([[17]], np.uint8),
        "one_pixel_bgr": np.array([[[17, 200, 90]]], np.uint8),
        "one_row_1x77": random_page(1, 77, 1, 1),
        "one_column_53x1": random_page(53, 1, 1, 2),
        "one_column_bgr_21x1": random_page(21, 1, 3, 3),
    }
    for w in (8, 9, 16, 17, 32, 33, 64, 65):                    # W = band and band + 1 for every band
        out["width_%d" % w] = random_page(19, w, 1 if w % 2 else 3, 10 + w)
    out["chunk_20x256"] = text_lines(20, 256, 4)                # one chunk of a wave exactly, and one pixel more
    out["chunk_20x257_bgr"] = text_lines(20, 257, 5, channels=3)
    out["odd_131x203"] = R.skewed(text_lines(131, 203, 6), 1.3)
    out["odd_240x333_bgr"] = R.skewed(text_lines(240, 333, 7, channels=3), -2.6)
    out["low_5x333"] = random_page(5, 333, 1, 8)
    out["white"] = np.full((40, 50), 255, np.uint8)
    out["black"] = np.zeros((40, 50), np.uint8)
    out["white_bgr"] = np.full((23, 70, 3), 255, np.uint8)
    out["black_bgr"] = np.zeros((23, 70, 3), np.uint8)
    out["two_levels"] = np.where(np.random.default_rng(9).random((33, 45)) < 0.2, 7, 7 + 1).astype(np.uint8)
    out["symmetric_v"] = v_page()
    return out


def sweep(name):
    """(shear_q16, n_steps, step, threshold, band)."""
    max_angle, step, threshold, band = SWEEPS[name]
    shear, n_steps = R.shears(max_angle, step)
    return np.ascontiguousarray(shear, np.int32), n_steps, step, threshold, band


@functools.lru_cache(maxsize=None)
def oracle(sweep_name):
    """The oracle's result of every page of the mixed batch under one sweep: a list of dicts in the batch's order."""
    shear, _n, _s, threshold, band = sweep(sweep_name)
    return [R.estimate(p, shear, threshold, band) for p in pages().values()]


def batch_arrays(ps):
    """(heights, widths, channels) int32 arrays of a list of pages."""
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    return i32([p.shape[0] for p in ps]), i32([p.shape[1] for p in ps]), i32([3 if p.ndim == 3 else 1 for p in ps])


def ptrs(addresses):
    return (C.c_void_p * max(len(addresses), 1))(*addresses)


def run_twin(ps, shear, threshold, band):
    """rtn_skew_estimate_host over the pages -> (rc, thresholds, ink, best, scores)."""
    n, K = len(ps), len(shear)
    hs, ws, ch = batch_arrays(ps)
    thr, ink, best, scores = np.full(n, -7, np.int32), np.full(n, -7, np.int64), np.full(n, -7, np.int32), np.full((n, K), 7, np.uint64)
    rc = L.lib.rtn_skew_estimate_host(n, ptrs([p.ctypes.data for p in ps]), hs.ctypes.data, ws.ctypes.data, ch.ctypes.data, threshold, band, K,
                                      shear.ctypes.data, thr.ctypes.data, ink.ctypes.data, best.ctypes.data, scores.ctypes.data)
    return rc, thr, ink, best, scores


def assert_equal_oracle(sweep_name, thr, ink, best, scores, where):
    for i, (name, want) in enumerate(zip(pages(), oracle(sweep_name))):
        tag = "%s, %s, %s" % (where, sweep_name, name)
        assert int(thr[i]) == want["threshold"], (tag, "threshold", int(thr[i]), want["threshold"])
        assert int(ink[i]) == want["ink"], (tag, "ink", int(ink[i]), want["ink"])
        assert np.array_equal(np.asarray(scores[i], np.uint64), want["scores"]), (tag, "scores differ at", np.nonzero(np.asarray(scores[i], np.uint64) != want["scores"])[0][:5])
        assert int(best[i]) == want["best"], (tag, "best", int(best[i]), want["best"])


def golden_page():
    from PIL import Image
    with Image.open(os.path.join(ROOT, "tests", "golden", "sample_0717_023_orig.jpg")) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])
