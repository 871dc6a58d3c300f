"""The header-detection oracle (tests/header_ref.py) and the host arithmetic of model/header.py against independent
implementations: colorsys, NumPy's own statistics on the raw pixel lists, a float64 block average, the explicit [1 2 1]/4 blur, the
reference's optK (recorded by tools/gen_header_golden.py) and, where sklearn is installed, the reference's estimator."""
import colorsys
import json
import os

import numpy as np
import pytest

import header_cases as K
import header_ref as R

HDR = K.HDR

# measured over all 2^24 colours (this file asserts them; DESIGN §3.4h quotes them)
HSV_VS_COLORSYS = (1, 1, 0)        # |cv2 8-bit rule - round(colorsys * (180, 255, 255))|, H on the circle of 180
ROUND_TRIP_BGR = (5, 5, 5)         # |HSV2BGR(BGR2HSV(x)) - x| per channel: H has 180 steps


def colorsys_hsv(rgb):
    """colorsys.rgb_to_hsv, vectorised in float64 with its operations in its order."""
    r, g, b = (rgb[..., i].astype(np.float64) / 255. for i in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    rangec = maxc - minc
    with np.errstate(all="ignore"):
        s = np.where(maxc == minc, 0.0, rangec / maxc)
        rc, gc, bc = (maxc - r) / rangec, (maxc - g) / rangec, (maxc - b) / rangec
        h = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc))
        h = (h / 6.0) % 1.0
    return np.where(maxc == minc, 0.0, h), s, maxc


def test_vectorised_colorsys_is_colorsys():
    c = np.random.default_rng(0).integers(0, 256, (3000, 3))
    h, s, v = colorsys_hsv(c)
    for i in range(len(c)):
        assert colorsys.rgb_to_hsv(c[i, 0] / 255., c[i, 1] / 255., c[i, 2] / 255.) == (h[i], s[i], v[i])


def test_bgr2hsv_and_the_round_trip_over_all_colours():
    worst, trip = np.zeros(3), np.zeros(3, np.int64)
    g, r = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for b in range(256):
        bgr = np.stack([np.full_like(g, b), g, r], axis=-1).astype(np.uint8)
        hsv = R.bgr2hsv(bgr)
        assert hsv[..., 0].max() < 180
        h, s, v = colorsys_hsv(bgr[..., ::-1])
        ref = np.rint(np.stack([h * 180, s * 255, v * 255], axis=-1))
        ref[..., 0] %= 180
        d = np.abs(hsv.astype(np.float64) - ref)
        d[..., 0] = np.minimum(d[..., 0], 180 - d[..., 0])
        worst = np.maximum(worst, d.reshape(-1, 3).max(axis=0))
        back = R.hsv2bgr(hsv)
        trip = np.maximum(trip, np.abs(back.astype(np.int64) - bgr.astype(np.int64)).reshape(-1, 3).max(axis=0))
    print("BGR2HSV against colorsys: H,S,V within", worst, "; HSV2BGR(BGR2HSV(x)) against x: B,G,R within", trip)
    assert tuple(worst) == HSV_VS_COLORSYS and tuple(trip) == ROUND_TRIP_BGR


def test_hsv2bgr_against_colorsys_on_the_whole_hsv_cube_slice():
    """Every H < 180 and S, V on a grid: the float32 sector rule against colorsys.hsv_to_rgb in float64, within one level."""
    hh, ss, vv = np.meshgrid(np.arange(180), np.arange(0, 256, 5), np.arange(0, 256, 5), indexing="ij")
    hsv = np.stack([hh, ss, vv], axis=-1).astype(np.uint8).reshape(-1, 3)
    got = R.hsv2bgr(hsv).astype(np.int64)
    step = 997
    for i in range(0, len(hsv), step):
        want = colorsys.hsv_to_rgb(hsv[i, 0] / 180., hsv[i, 1] / 255., hsv[i, 2] / 255.)
        assert np.abs(got[i, ::-1] - np.array(want) * 255).max() <= 0.5 + 1e-3, hsv[i]


def test_histogram_statistics_equal_numpys_on_the_raw_lists():
    rng = np.random.default_rng(3)
    lists = [rng.integers(0, 256, (n, 3)).astype(np.uint8) for n in (1, 2, 3, 4, 5, 7, 8, 101, 1000)]
    lists += [np.repeat(np.array([[0, 255, 7]], np.uint8), 9, axis=0), rng.integers(100, 104, (4001, 3)).astype(np.uint8),
              np.array([[0, 0, 0], [2, 255, 1], [0, 0, 0], [2, 255, 1]], np.uint8)]
    for nm in ("table_sigma6", "page_window", "enlarge_123x45"):
        o = K.oracle(nm)
        pts, fit = o["hsv"].reshape(-1, 3), o["fits"][o["k"] - 1]
        lists += [pts[fit["labels"] == j] for j in range(o["k"]) if fit["counts"][j]]
    for lst in lists:
        hist = np.stack([np.bincount(lst[:, c], minlength=256) for c in range(3)])
        got, want = HDR.histogram_stats(hist), R.analyse(lst)
        for key, w in want.items():
            assert np.array_equal(np.asarray(got[key], np.float64), np.asarray(w, np.float64)), (len(lst), key, got[key], w)


def test_box_resample_equals_a_float64_block_average_on_integer_ratios():
    for (h, w), (fy, fx) in (((36, 1000), (2, 2)), ((30, 1500), (3, 3)), ((8, 2000), (4, 4)), ((7, 500), (1, 1))):
        img = K.blocks(h, w, h + w, cell=5, noise=20)
        dh = R.sampled_height(h, w)
        assert (dh * fy, 500 * fx) == (h, w)
        sums = np.add.reduceat(np.add.reduceat(img.astype(np.float64), np.arange(0, h, fy), axis=0), np.arange(0, w, fx), axis=1)
        want = np.floor(sums / (fy * fx) + 0.5).astype(np.uint8)
        assert np.array_equal(R.box_resample(img, dh), want), (h, w)


def test_box_resample_keeps_flat_images_and_the_mean():
    for h, w in ((45, 123), (211, 1333), (37, 1000), (1, 1)):
        dh = R.sampled_height(h, w)
        flat = np.full((h, w, 3), (3, 250, 77), np.uint8)
        assert np.all(R.box_resample(flat, dh) == (3, 250, 77))
        img = K.blocks(h, w, 11, cell=7)
        got = R.box_resample(img, dh).astype(np.float64)
        assert np.abs(got.mean(axis=(0, 1)) - img.mean(axis=(0, 1))).max() <= 0.5      # every output is within 1/2 of an exact weighted mean


def blur_121(mask):
    """cv2.GaussianBlur(mask, (3, 3), 0) of a uint8 image: the fixed-point [1 2 1]/4 kernel both ways, reflect-101 border
    (a side of one pixel has nothing to reflect: its neighbours are the pixel itself), rounded once."""
    m = mask.astype(np.int64)
    modes = ["reflect" if n > 1 else "edge" for n in m.shape]
    p = np.pad(m, ((1, 1), (0, 0)), mode=modes[0])
    p = np.pad(p, ((0, 0), (1, 1)), mode=modes[1])
    h, w = m.shape
    acc = np.zeros((h, w), np.int64)
    k = (1, 2, 1)
    for dy in range(3):
        for dx in range(3):
            acc += k[dy] * k[dx] * p[dy:dy + h, dx:dx + w]
    return ((acc + 8) >> 4).astype(np.uint8)


def test_the_3x3_mask_rule_equals_the_explicit_blur():
    rng = np.random.default_rng(5)
    for h, w, density in ((1, 1, 0.5), (1, 9, 0.3), (9, 1, 0.3), (2, 2, 0.4), (12, 17, 0.02), (12, 17, 0.5), (30, 500, 0.005), (3, 500, 0.9)):
        for _ in range(4):
            mask = rng.random((h, w)) < density
            assert np.array_equal(blur_121(np.where(mask, 255, 0).astype(np.uint8)) != 0, R.dilate3(mask)), (h, w)
    corner = np.zeros((5, 6), bool)
    corner[0, 0] = corner[4, 5] = True
    assert R.dilate3(corner).sum() == 8


def test_opt_k_equals_the_reference_on_the_recorded_vectors():
    with open(os.path.join(K.ROOT, "tests", "golden", "header_optk.json")) as f:
        rows = json.load(f)
    assert len(rows) >= 40 and any(r["k"] is None for r in rows) and {r["k"] for r in rows} >= set(range(2, 9))
    for r in rows:
        assert HDR.opt_k(r["distortions"]) == r["k"] == R.opt_k(r["distortions"]), r


QUALITY_CASES = ["table_sigma%d" % s for s in K.TABLE_SIGMAS] + ["page_window"]


def inertia(pts, labels, centres):
    d = pts.astype(np.float64) - centres.astype(np.float64)[labels]
    return float((d * d).sum())


def sklearn_inertias(pts, k, seeds=range(20)):
    from sklearn.cluster import KMeans
    from threadpoolctl import threadpool_limits             # sklearn's own dependency; 80,000 points run fastest on a few threads
    with threadpool_limits(limits=4):
        return [float(KMeans(n_clusters=k, random_state=s, n_init=1).fit(pts).inertia_) for s in seeds]


@pytest.mark.parametrize("name", QUALITY_CASES)
def test_clustering_is_never_worse_than_a_single_kmeanspp_start(name):
    """For k = 2 .. 9 the inertia of the chain's final labels and centres, recomputed in float64, is at most (1 + 1e-6) x the worst of
    twenty KMeans(n_clusters=k, random_state=s, n_init=1) fits, s = 0 .. 19 (the reference's estimator with one start).
    Measured (tools/header_kmeans_quality.py, profiles/header_kmeans_quality.txt): see DESIGN §3.4h."""
    pytest.importorskip("sklearn")
    o = K.oracle(name)
    pts = o["hsv"].reshape(-1, 3)
    for k in range(2, 10):
        fit = o["fits"][k - 1]
        ours = inertia(pts, fit["labels"], fit["centres"])
        theirs = sklearn_inertias(pts, k)
        print("%s k=%d ours %.6g worst %.6g best %.6g ratio to worst %.4f to best %.4f" % (
            name, k, ours, max(theirs), min(theirs), ours / max(theirs), ours / min(theirs)))
        assert ours <= (1 + 1e-6) * max(theirs), (name, k, ours, max(theirs))
