"""Crafted binary pages for the distance-transform tests, shared by the CPU oracle test (tests/test_preprocess_oracle.py) and
the device test (tests/test_gpu_preprocess.py).  Every builder returns two DIFFERENT uint8 pages (2, H, W) with values 0 / 255.

The device sweeps a page row by row; `T` threads hold `E` adjacent columns each (csrc/rtn_preprocess.hip: dt3_launch), so the
places where a scan can go wrong are the seams between threads (columns k*E - 1 | k*E) and between 64-lane waves
(k*64*E - 1 | k*64*E), the out-of-range columns of the last thread, and the first / last rows of a sweep."""
import numpy as np

CONTENTS = ("sparse", "corner0", "corner1", "corner2", "corner3", "seams", "all255", "all0", "dense")


def launch_shape(W):
    """(threads, columns per thread) that dt3_launch picks for a page W wide when RTN_DT_CFG is not set."""
    T = 256 if W <= 256 else (512 if W <= 512 else 1024)
    return T, -(-W // T)


def corner_pages(H, W, k):
    """A single zero pixel per page: corner k (clockwise from the top left) on page 0, the opposite corner on page 1."""
    corners = [(0, 0), (0, W - 1), (H - 1, W - 1), (H - 1, 0)]
    b = np.full((2, H, W), 255, np.uint8)
    for i in range(2):
        y, x = corners[(k + 2 * i) % 4]
        b[i, y, x] = 0
    return b


def seam_columns(W, T, E):
    """(left, right): the last column of a thread / wave and the first column of the next one.  Every wave seam, and the thread
    seam of every 37th thread (37 is odd and no divisor of 64, so the chosen lanes differ from wave to wave)."""
    ks = sorted(set(range(64, T, 64)) | set(range(1, T, 37)))
    left = np.array([k * E - 1 for k in ks if k * E - 1 < W], np.int64)
    right = np.array([k * E for k in ks if k * E < W], np.int64)
    return left, right


def seam_pages(H, W, T, E):
    """Zeros only at seam columns, on alternating rows: every second row carries zeros, in turn at the left and at the right
    columns (page 1 starts with the right ones); the rows between carry none.  A pixel next to a zero across a seam then has no
    zero straight above or below it, so its distance of 1 has to come through the seam, in both sweep directions."""
    left, right = seam_columns(W, T, E)
    b = np.full((2, H, W), 255, np.uint8)
    for i in range(2):
        for y in range(0, H, 2):
            b[i, y, left if (y + 2 * i) % 4 == 0 else right] = 0
    return b


def dt_pages(content, H, W, T=None, E=None, seed=0):
    if T is None:
        T, E = launch_shape(W)
    rng = np.random.RandomState(seed + 7919 * H + W)
    if content == "sparse":
        return (rng.uniform(size=(2, H, W)) > 0.002).astype(np.uint8) * 255
    if content == "dense":
        return (rng.uniform(size=(2, H, W)) > 0.5).astype(np.uint8) * 255
    if content.startswith("corner"):
        return corner_pages(H, W, int(content[6:]))
    if content == "seams":
        return seam_pages(H, W, T, E)
    if content in ("all255", "all0"):                       # the named page first, the other uniform page second
        b = np.empty((2, H, W), np.uint8)
        b[0], b[1] = (255, 0) if content == "all255" else (0, 255)
        return b
    raise ValueError(content)
