"""NumPy oracle of the colour effects (VisualEffect of model/transform.py): the four steps as direct array text, written
from their definitions, around header_ref's restatement of OpenCV's 8-bit BGR2HSV / HSV2BGR (recalled, not verifiable offline).  No
code is shared with the package.  The variants (float32, fused, exactly rounded mean) are what the tests show the rules are not."""
import math

import numpy as np

from header_ref import bgr2hsv, hsv2bgr


def clip_u8(a):
    return np.clip(a, 0, 255).astype(np.uint8)


def channel_means(image):
    return image.mean(axis=0).mean(axis=0)


def contrast(image, factor, mean=None):
    mean = channel_means(image) if mean is None else mean
    return clip_u8((image - mean) * factor + mean)


def brightness(image, delta):
    return clip_u8(image + delta * 255)


def hue(hsv, delta):
    out = hsv.copy()
    out[..., 0] = np.mod(hsv[..., 0] + delta * 180, 180)
    return out


def saturation(hsv, factor):
    out = hsv.copy()
    out[..., 1] = np.clip(hsv[..., 1] * factor, 0, 255)
    return out


def effect(image, params, raw_hsv=False, force=(False, False, False, False)):
    """VisualEffect(*params)(image) for a uint8 (H, W, 3) B,G,R page; a falsy parameter skips its step unless `force` names it (the
    adjust_* functions called on their own run whatever the parameter).  raw_hsv: the page holds H,S,V already and neither conversion
    runs."""
    c, b, h, s = (float(v) for v in params)
    on = [bool(v) or bool(f) for v, f in zip((c, b, h, s), force)]
    image = np.asarray(image)
    if on[0]:
        image = contrast(image, c)
    if on[1]:
        image = brightness(image, b)
    if on[2] or on[3]:
        if not raw_hsv:
            image = bgr2hsv(image)
        if on[2]:
            image = hue(image, h)
        if on[3]:
            image = saturation(image, s)
        if not raw_hsv:
            image = hsv2bgr(image)
    return np.array(image, np.uint8)


# ---- what the rules are not -----------------------------------------------------------------------------------------------------------
def sequential_means(image):
    """The column means added from x = 0 upwards, one float64 add at a time."""
    col = image.sum(axis=0, dtype=np.int64)
    out = []
    for c in range(3):
        acc = 0.0
        for x in range(image.shape[1]):
            acc = acc + float(col[x, c]) / float(image.shape[0])
        out.append(acc / float(image.shape[1]))
    return np.array(out)


def fsum_means(image):
    """The same column means, summed with one rounding."""
    col = image.sum(axis=0, dtype=np.int64)
    return np.array([math.fsum(float(col[x, c]) / float(image.shape[0]) for x in range(image.shape[1])) / float(image.shape[1])
                     for c in range(3)])


def _trunc_u8(a):
    return np.clip(a.astype(np.float64), 0, 255).astype(np.uint8)


def contrast_table(mean, factor, variant="f64"):
    """The 256 results of the contrast step for one channel mean: 'f64' (the rule), 'f32' (every operation in float32) or 'fused'
    ((x - m) * f + m with the product unrounded, as a fused multiply-add gives it)."""
    x = np.arange(256)
    if variant == "f64":
        return clip_u8((x - np.float64(mean)) * factor + np.float64(mean))
    if variant == "f32":
        m, f = np.float32(mean), np.float32(factor)
        return _trunc_u8((x.astype(np.float32) - m) * f + m)
    from fractions import Fraction
    out = []
    for v in x:
        d = float(v) - float(mean)                                           # rounded, as before a fused multiply-add
        exact = Fraction(d) * Fraction(float(factor)) + Fraction(float(mean))
        out.append(float(exact))                                             # one rounding of the exact sum
    return clip_u8(np.array(out))


def saturation_table(factor, variant="f64"):
    x = np.arange(256)
    if variant == "f64":
        return clip_u8(x * float(factor))
    return _trunc_u8(x.astype(np.float32) * np.float32(factor))


def hue_table(delta, variant="f64"):
    x = np.arange(256)
    if variant == "f64":
        return np.mod(x + float(delta) * 180, 180).astype(np.uint8)
    return np.mod(x.astype(np.float32) + np.float32(delta) * np.float32(180), np.float32(180)).astype(np.uint8)
