"""The augmentation of the reference's model/transform.py behind the same names: geometry and colour effects.

The 3x3 homogeneous matrices are host NumPy (float64, a handful of flops per image); the draws come from the caller's PRNG in the
reference's order (rotation, translation x/y, shear, scaling x/y, flip x, flip y - model/transform.py:190-234), so a seeded
RandomState yields the reference's matrices bit for bit (tests/golden/ref_generator_golden.npz holds matrices produced by the
reference module itself).  apply_transform - cv2.warpAffine in the reference (model/transform.py:343-362) - runs on the device
through rtn_warp_affine_u8.

The colour effects (VisualEffect, random_visual_effect_generator, adjust_*: model/transform.py:365-512) run on the device through
rtn_visual_effect_u8: the four parameters are np.random.uniform draws from the global NumPy state in the
reference's order (contrast, brightness, hue, saturation), the pixels are the reference's NumPy text bit for bit around a
restatement of cv2's 8-bit BGR2HSV / HSV2BGR (recalled, not verifiable offline).  visual_effect_batch is the batched form the
generator uses: every page of a group in one call.
"""
import numpy as np

DEFAULT_PRNG = np.random

_BORDER_CV = {'constant': 0, 'nearest': 1, 'reflect': 4, 'wrap': 3}            # cv2.BORDER_* values
_INTER_CV = {'nearest': 0, 'linear': 1, 'cubic': 2, 'area': 3, 'lanczos4': 4}  # cv2.INTER_* values
_BORDER_RTN = {0: 0, 1: 1, 4: 2, 3: 3}                                          # cv2 code -> rtn_warp_affine_u8 border_mode


def colvec(*args):
    return np.array([args]).T


def _homogeneous(top, bottom):
    return np.array([list(top), list(bottom), [0, 0, 1]])


def rotation(angle):
    c, s = np.cos(angle), np.sin(angle)
    return _homogeneous((c, -s, 0), (s, c, 0))


def translation(translation):
    return _homogeneous((1, 0, translation[0]), (0, 1, translation[1]))


def shear(angle):
    return _homogeneous((1, -np.sin(angle), 0), (0, np.cos(angle), 0))


def scaling(factor):
    return _homogeneous((factor[0], 0, 0), (0, factor[1], 0))


def _random_vector(min, max, prng=DEFAULT_PRNG):
    lo, hi = np.array(min), np.array(max)
    assert lo.shape == hi.shape
    assert len(lo.shape) == 1
    return prng.uniform(lo, hi)


def random_rotation(min, max, prng=DEFAULT_PRNG):
    return rotation(prng.uniform(min, max))


def random_translation(min, max, prng=DEFAULT_PRNG):
    return translation(_random_vector(min, max, prng))


def random_shear(min, max, prng=DEFAULT_PRNG):
    return shear(prng.uniform(min, max))


def random_scaling(min, max, prng=DEFAULT_PRNG):
    return scaling(_random_vector(min, max, prng))


def random_flip(flip_x_chance, flip_y_chance, prng=DEFAULT_PRNG):
    fx = prng.uniform(0, 1) < flip_x_chance
    fy = prng.uniform(0, 1) < flip_y_chance
    return scaling((1 - 2 * fx, 1 - 2 * fy))


def change_transform_origin(transform, center):
    """translate(center) . transform . translate(-center) (model/transform.py:177-187)."""
    center = np.array(center)
    return np.linalg.multi_dot([translation(center), transform, translation(-center)])


def random_transform(min_rotation=0, max_rotation=0, min_translation=(0, 0), max_translation=(0, 0), min_shear=0, max_shear=0,
                     min_scaling=(1, 1), max_scaling=(1, 1), flip_x_chance=0, flip_y_chance=0, prng=DEFAULT_PRNG):
    """rotation . translation . shear . scaling . flip, each drawn from `prng` in that order (model/transform.py:190-234)."""
    parts = [random_rotation(min_rotation, max_rotation, prng),
             random_translation(min_translation, max_translation, prng),
             random_shear(min_shear, max_shear, prng),
             random_scaling(min_scaling, max_scaling, prng),
             random_flip(flip_x_chance, flip_y_chance, prng)]
    return np.linalg.multi_dot(parts)


def random_transform_generator(prng=None, **kwargs):
    """Endless stream of random_transform(**kwargs) from one dedicated PRNG (model/transform.py:237-272)."""
    prng = np.random.RandomState() if prng is None else prng
    while True:
        yield random_transform(prng=prng, **kwargs)


def transform_aabb(transform, aabb):
    """Axis-aligned box around the four transformed corners (model/transform.py:17-42)."""
    x1, y1, x2, y2 = aabb
    pts = transform.dot([[x1, x2, x1, x2],
                         [y1, y2, y2, y1],
                         [1, 1, 1, 1]])
    lo, hi = pts.min(axis=1), pts.max(axis=1)
    return [lo[0], lo[1], hi[0], hi[1]]


class TransformParameters:
    """How apply_transform samples (model/transform.py:280-321): fill_mode 'constant' | 'nearest' | 'reflect' | 'wrap',
    interpolation 'nearest' | 'linear' (the device kernel implements these two; 'cubic', 'area', 'lanczos4' raise),
    cval for 'constant', relative_translation."""

    def __init__(self, fill_mode='nearest', interpolation='linear', cval=0, relative_translation=True):
        self.fill_mode = fill_mode
        self.cval = cval
        self.interpolation = interpolation
        self.relative_translation = relative_translation

    def cvBorderMode(self):
        return _BORDER_CV.get(self.fill_mode)

    def cvInterpolation(self):
        return _INTER_CV.get(self.interpolation)


def adjust_transform_for_image(transform, image, relative_translation):
    """Scale the translation by the image size (in place, as the reference does) and move the origin to the image centre
    (model/transform.py:324-340)."""
    height, width = image.shape[0], image.shape[1]
    if relative_translation:
        transform[0:2, 2] *= [width, height]
    return change_transform_origin(transform, (0.5 * width, 0.5 * height))


def invert_affine(matrix):
    """The destination->source map cv2.warpAffine derives from a forward 2x3 matrix (its own double-precision formula, recalled
    from OpenCV's imgwarp.cpp - not the general matrix inverse, so the roundings match)."""
    M = np.array(matrix, np.float64)[:2, :].copy()
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[1, 1] * D, M[0, 0] * D
    M[0, 0] = A11
    M[0, 1] *= -D
    M[1, 0] *= -D
    M[1, 1] = A22
    b1 = -M[0, 0] * M[0, 2] - M[0, 1] * M[1, 2]
    b2 = -M[1, 0] * M[0, 2] - M[1, 1] * M[1, 2]
    M[0, 2], M[1, 2] = b1, b2
    return M


def warp_codes(params):
    """(interpolation, border_mode, cval4) of rtn_warp_affine_u8 for a TransformParameters."""
    inter, border = params.cvInterpolation(), params.cvBorderMode()
    if inter not in (0, 1):
        raise NotImplementedError("apply_transform: interpolation %r is not implemented on the device (nearest, linear are)" % (params.interpolation,))
    if border not in _BORDER_RTN:
        raise ValueError("apply_transform: unknown fill_mode %r" % (params.fill_mode,))
    # cv2 receives borderValue = params.cval as Scalar(cval): the first channel gets cval, the others 0
    cval = np.zeros(4, np.uint8)
    cval[0] = int(np.clip(np.rint(params.cval), 0, 255))
    return inter, _BORDER_RTN[border], cval


def apply_transform(matrix, image, params):
    """cv2.warpAffine(image, matrix[:2], dsize = image size, flags, borderMode, borderValue) on the device.  `image`: uint8 (H,W,C)
    NumPy array (returns NumPy) or CUDA tensor (returns a CUDA tensor, no host round trip)."""
    import ctypes
    import torch
    from . import _rt
    L = _rt.L
    inter, border, cval = warp_codes(params)
    on_device = isinstance(image, torch.Tensor)
    if (image.dtype != torch.uint8) if on_device else (np.asarray(image).dtype != np.uint8):
        raise ValueError("apply_transform: the device path takes uint8 pages (what cv2.imread hands the generator)")
    src = image.contiguous() if on_device else _rt.dev(image, torch.uint8)
    if src.dim() == 2:
        src = src[..., None]
    H, W, C = src.shape
    inv = np.ascontiguousarray(invert_affine(matrix))
    dst = torch.empty_like(src)
    h = _rt.handle()
    h.check(L.lib.rtn_warp_affine_u8(h.raw, src.data_ptr(), H, W, C, inv.ctypes.data_as(ctypes.c_void_p), inter, border,
                                     cval.ctypes.data_as(ctypes.c_void_p), dst.data_ptr()))
    if image.ndim == 2:
        dst = dst[..., 0]
    return dst if on_device else _rt.host(dst)


# ---- colour effects (model/transform.py:365-512) on the device: rtn_visual_effect_u8, DESIGN §3.4j -----------------------------------
_CONTRAST, _BRIGHTNESS, _HUE, _SATURATION = 0, 1, 2, 3                          # the order of a page's four parameters


def _uniform(val_range):
    """One draw from the global NumPy state (model/transform.py:365-370)."""
    return np.random.uniform(val_range[0], val_range[1])


def _check_range(val_range, min_val=None, max_val=None):
    """model/transform.py:373-385."""
    if val_range[0] > val_range[1]:
        raise ValueError('interval lower bound > upper bound')
    if min_val is not None and val_range[0] < min_val:
        raise ValueError('invalid interval lower bound')
    if max_val is not None and val_range[1] > max_val:
        raise ValueError('invalid interval upper bound')


def _clip(image):
    """model/transform.py:388-394, host NumPy (the device steps clip inside their tables)."""
    return np.clip(image, 0, 255).astype(np.uint8)


def visual_effect_batch(pages, params, flags=None, handle=None, in_place=False):
    """Every page of a group through rtn_visual_effect_u8 in one call.  pages: contiguous uint8 (H,W,3) CUDA tensors of any sizes;
    params: one (contrast_factor, brightness_delta, hue_delta, saturation_factor) per page; flags: None or one RTN_EFFECT_* word per
    page.  Runs on `handle` and its stream (default: the package's handle on the current stream) and returns the new pages, or the
    pages themselves with in_place."""
    import torch
    from . import _pages
    L = _pages.L
    n = len(pages)
    if n == 0:
        return []
    for p in pages:
        if not isinstance(p, torch.Tensor) or not p.is_cuda or p.dtype != torch.uint8 or p.dim() != 3 or p.shape[2] != 3 or not p.is_contiguous():
            raise ValueError("visual_effect_batch: contiguous uint8 (H,W,3) CUDA tensors expected")
    be = _pages.Device(pages[0].device, handle)
    par = np.ascontiguousarray(np.asarray(params, np.float64).reshape(n, 4))
    fl = np.zeros(n, np.uint32) if flags is None else np.ascontiguousarray(np.asarray(flags, np.uint32).reshape(n))
    heights = np.array([p.shape[0] for p in pages], np.int32)
    widths = np.array([p.shape[1] for p in pages], np.int32)
    outs = list(pages) if in_place else [torch.empty_like(p) for p in pages]

    def room():
        wsb = L.lib.rtn_visual_effect_workspace_bytes(n, heights.ctypes.data, widths.ctypes.data)
        if wsb == 0:
            raise ValueError("visual_effect_batch: at most 65535 pages with sides 1 .. 65500")
        return wsb
    be.call("rtn_visual_effect_u8", [n, _pages.pointers(be, pages), heights.ctypes.data, widths.ctypes.data, par.ctypes.data, fl.ctypes.data,
                                     _pages.pointers(be, outs)], room)
    return outs


def _effect_one(image, params, flags, in_place=False):
    """One page through the device entry: a uint8 (H,W,3) NumPy array (returns NumPy) or CUDA tensor (returns a CUDA tensor, no host
    round trip), as apply_transform."""
    import torch
    from . import _rt
    on_device = isinstance(image, torch.Tensor)
    if (image.dtype != torch.uint8) if on_device else (np.asarray(image).dtype != np.uint8):
        raise ValueError("the colour effects take uint8 pages (what cv2.imread hands the generator)")
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("the colour effects take (H,W,3) pages")
    if on_device:
        if in_place and image.is_contiguous():
            return visual_effect_batch([image], [params], [flags], in_place=True)[0]
        out = visual_effect_batch([image.contiguous()], [params], [flags])[0]
        return image.copy_(out) if in_place else out
    out = _rt.host(visual_effect_batch([_rt.dev(image, torch.uint8)], [params], [flags])[0])
    if in_place:
        image[...] = out
        return image
    return out


class VisualEffect:
    """model/transform.py:397-440: the four parameters, and __call__ applying them to a page.  A parameter that is 0 skips its step;
    the HSV round trip runs when hue or saturation does."""

    def __init__(self, contrast_factor, brightness_delta, hue_delta, saturation_factor):
        self.contrast_factor = contrast_factor
        self.brightness_delta = brightness_delta
        self.hue_delta = hue_delta
        self.saturation_factor = saturation_factor

    def params(self):
        return (float(self.contrast_factor), float(self.brightness_delta), float(self.hue_delta), float(self.saturation_factor))

    def __call__(self, image):
        return _effect_one(image, self.params(), 0)


def random_visual_effect_generator(contrast_range=(0.9, 1.1), brightness_range=(-.1, .1), hue_range=(-0.05, 0.05),
                                   saturation_range=(0.95, 1.05)):
    """Endless stream of VisualEffect with parameters drawn uniformly from the given intervals (model/transform.py:443-472); the
    intervals are checked by the call itself."""
    _check_range(contrast_range, 0)
    _check_range(brightness_range, -1, 1)
    _check_range(hue_range, -1, 1)
    _check_range(saturation_range, 0)

    def _generate():
        while True:
            yield VisualEffect(contrast_factor=_uniform(contrast_range), brightness_delta=_uniform(brightness_range),
                               hue_delta=_uniform(hue_range), saturation_factor=_uniform(saturation_range))

    return _generate()


def _one_step(image, step, value, raw_hsv, in_place=False):
    from . import _rt
    params = [0.0, 0.0, 0.0, 0.0]
    params[step] = float(value)
    flags = (_rt.L.RTN_EFFECT_FORCE_CONTRAST << step) | (_rt.L.RTN_EFFECT_RAW_HSV if raw_hsv else 0)
    return _effect_one(image, params, flags, in_place)


def adjust_contrast(image, factor):
    """clip((image - mean) * factor + mean) with the per-channel mean (model/transform.py:475-482)."""
    return _one_step(image, _CONTRAST, factor, False)


def adjust_brightness(image, delta):
    """clip(image + delta * 255) (model/transform.py:485-491)."""
    return _one_step(image, _BRIGHTNESS, delta, False)


def adjust_hue(image, delta):
    """H = mod(H + delta * 180, 180) of an H,S,V image, in place as in the reference (model/transform.py:494-502)."""
    return _one_step(image, _HUE, delta, True, in_place=True)


def adjust_saturation(image, factor):
    """S = clip(S * factor, 0, 255) of an H,S,V image, in place as in the reference (model/transform.py:505-512)."""
    return _one_step(image, _SATURATION, factor, True, in_place=True)
