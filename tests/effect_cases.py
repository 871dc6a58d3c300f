"""The pages and parameters the colour-effect tests share (tests/test_effect_ref.py, test_effect_host.py, test_gpu_effect.py), and the
oracle's result for each, computed once per process.  A case is (name, page, params, flags): params = contrast factor, brightness
delta, hue delta, saturation factor; flags as rtn_visual_effect_u8 takes them."""
import functools
import itertools

import numpy as np

import effect_ref as R

RAW_HSV, FORCE = 1, (16, 32, 64, 128)
# H = 1; the summation order (1 x 4097, 3 x 3000, 700 x 513); many row strips (1030 x 7, 700 x 513); a width below one vector (1 x 1,
# 1030 x 7, 5 x 17); rows that are dword aligned (9 x 64, 6 x 196, 211 x 172) and rows that are not
SHAPES = ((1, 1), (1, 4097), (3, 3000), (700, 513), (1030, 7), (5, 17), (9, 64), (6, 196), (211, 172))
# a fused (x - m) * f + m and float32 change entries of the contrast table at these factors, float32 those of S and H at these
FUSED_AT_MEAN_100 = (0.8, 0.9, 1.1, 1.3, 1.6)
F32_AT_MEAN_100 = (0.6, 1.1, 1.2)
F32_AT_MEAN_0 = (0.7, 1.3, 1.4, 2.1)
F32_SATURATION = (0.29, 0.35, 0.7)
F32_HUE = (-127 / 180, -121 / 180, -116 / 180, -112 / 180)
PLAIN_HUE = 116 / 180                                                        # float32 gives the same table here; kept as a plain case
TINY_HUE = -1e-22                                                            # mod gives 180.0: the byte 180 reaches HSV2BGR


def random_page(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def exact_means_page():
    """4 x 512: B holds every byte and every column of it adds up to 400 (mean exactly 100.0), G is 0 (mean exactly 0.0), R random."""
    v = np.arange(512) % 256
    b = np.where(v <= 200, [v, 200 - v, 100 + 0 * v, 100 + 0 * v], [v, 400 - v, 0 * v, 0 * v])
    page = random_page(4, 512, 77)
    page[..., 0] = b
    page[..., 1] = 0
    return page


def ramp_page():
    """3 x 256, taken as H,S,V: channel 0 and channel 1 hold every byte, so every entry of the H and S tables reaches the output."""
    page = random_page(3, 256, 78)
    page[..., 0] = np.arange(256)
    page[..., 1] = 255 - np.arange(256)
    return page


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    rng = np.random.default_rng(5)
    for h, w in SHAPES:
        p = (rng.uniform(0.5, 1.5), rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.5), rng.uniform(0.5, 1.5))
        out.append(("random_%dx%d" % (h, w), random_page(h, w, 1000 * h + w), p, 0))
    exact, ramp, colours, small = exact_means_page(), ramp_page(), random_page(211, 172, 3), random_page(9, 64, 4)
    for f in sorted(set(FUSED_AT_MEAN_100 + F32_AT_MEAN_100 + F32_AT_MEAN_0)):
        out.append(("exact_means_contrast_%g" % f, exact, (f, 0.0, 0.0, 0.0), 0))
    for f in F32_SATURATION:
        out.append(("saturation_%g" % f, colours, (0.0, 0.0, 0.0, f), 0))
        out.append(("raw_saturation_%g" % f, ramp, (0.0, 0.0, 0.0, f), RAW_HSV))
    for d in F32_HUE + (PLAIN_HUE, TINY_HUE):
        out.append(("hue_%g" % d, colours, (0.0, 0.0, d, 0.0), 0))
        out.append(("raw_hue_%g" % d, ramp, (0.0, 0.0, d, 0.0), RAW_HSV))
    for d in (1.0, -1.0):
        out.append(("both_clips_%g" % d, small, (3.0, d, 0.0, 0.0), 0))
    for on in itertools.product((0, 1), repeat=4):                           # all 16 combinations; at 0000 the page is copied
        out.append(("steps_%d%d%d%d" % on, small, tuple(v * k for v, k in zip((1.3, 0.2, 0.1, 0.7), on)), 0))
    # adjust_* on their own run whatever the parameter: a zero factor leaves the truncated mean, a zero hue delta is mod 180
    out.append(("forced_contrast_0", small, (0.0, 0.0, 0.0, 0.0), FORCE[0]))
    out.append(("forced_brightness_0", small, (0.0, 0.0, 0.0, 0.0), FORCE[1]))
    out.append(("forced_raw_hue_0", ramp, (0.0, 0.0, 0.0, 0.0), FORCE[2] | RAW_HSV))
    out.append(("forced_raw_saturation_0", ramp, (0.0, 0.0, 0.0, 0.0), FORCE[3] | RAW_HSV))
    out.append(("forced_round_trip", small, (0.0, 0.0, 0.0, 0.0), FORCE[2]))
    assert len(set(c[0] for c in out)) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def oracle(i):
    """effect_ref.effect of case i."""
    _name, page, params, flags = cases()[i]
    return R.effect(page, params, raw_hsv=bool(flags & RAW_HSV), force=[bool(flags & f) for f in FORCE])


def batch_arrays(pages, params, flags):
    """The host arrays of one call: heights, widths, params (n, 4) float64, flags uint32."""
    heights = np.array([p.shape[0] for p in pages], np.int32)
    widths = np.array([p.shape[1] for p in pages], np.int32)
    return heights, widths, np.ascontiguousarray(params, np.float64).reshape(len(pages), 4), np.asarray(flags, np.uint32)
