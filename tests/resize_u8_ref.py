"""NumPy oracle of the 8-bit bicubic resize (csrc/rtn_resize_u8.h): cv2.resize(INTER_CUBIC) of a uint8 page in
OpenCV's portable C form, as recalled (OpenCV is not available to check it against).  Written on its own, in int64 NumPy, from
the rules of the header's comment; it asserts that the sums the kernels keep in int32 fit.

Per axis: f = (d + 0.5) * inv - 0.5 (float64), s = floor(f), x = float32(f - s); the float32 coefficients of x with A = -0.75,
one rounding per operation, c3 = 1 - c0 - c1 - c2; each coefficient becomes rint(c * 2048) (half to even) saturated to a short;
the taps read clip(s - 1 + k, 0, n - 1).  Horizontal sums, vertical sums, then clip((v + 2^21) >> 22, 0, 255)."""
import numpy as np

F32 = np.float32
ONE = 2048
LIMIT = 1 << 31


def out_size(h, w, fx, fy=None):
    """cv2's factor form: (Ho, Wo) = saturate_cast<int>(H * fy), saturate_cast<int>(W * fx), half to even."""
    fy = fx if fy is None else fy
    return int(np.rint(h * float(fy))), int(np.rint(w * float(fx)))


def coefficients(x):
    """The four fixed-point coefficients (int64 arrays) of the float32 fractions x."""
    x = np.asarray(x, F32)
    a = F32(-0.75)
    one, two, three = F32(1), F32(2), F32(3)
    x1 = x + one
    c0 = ((a * x1 - F32(5) * a) * x1 + F32(8) * a) * x1 - F32(4) * a
    c1 = ((a + two) * x - (a + three)) * x * x + one
    y = one - x
    c2 = ((a + two) * y - (a + three)) * y * y + one
    c3 = one - c0 - c1 - c2
    out = []
    for c in (c0, c1, c2, c3):
        assert c.dtype == F32
        fixed = np.rint(c * F32(ONE))                           # the product is exact; rint rounds half to even
        out.append(np.clip(fixed, -32768, 32767).astype(np.int64))
    return out


def axis(n_out, n_in, inv):
    """(indices (4, n_out) of the clipped taps, coefficients (4, n_out)) of one axis."""
    f = (np.arange(n_out, dtype=np.float64) + 0.5) * np.float64(inv) - 0.5
    s = np.floor(f)
    coef = coefficients((f - s).astype(F32))
    s = np.clip(s, -4, n_in + 4).astype(np.int64)                # far outside every tap clips to the same border
    idx = [np.clip(s - 1 + k, 0, n_in - 1) for k in range(4)]
    return np.stack(idx), np.stack(coef)


def resize(page, ho, wo, inv_x, inv_y):
    """The (ho, wo[, 3]) uint8 resize of a uint8 (H, W[, 3]) page with the inverse scales inv_x, inv_y."""
    page = np.asarray(page)
    assert page.dtype == np.uint8 and page.ndim in (2, 3)
    src = page.astype(np.int64).reshape(page.shape[0], page.shape[1], -1)
    H, W, _ = src.shape
    ix, cx = axis(wo, W, inv_x)
    iy, cy = axis(ho, H, inv_y)
    h = np.zeros((H, wo, src.shape[2]), np.int64)
    for k in range(4):
        h += src[:, ix[k]] * cx[k][None, :, None]
    assert np.abs(h).max() < LIMIT
    v = np.zeros((ho, wo, src.shape[2]), np.int64)
    for k in range(4):
        v += h[iy[k]] * cy[k][:, None, None]
    assert np.abs(v).max() + (1 << 21) < LIMIT
    out = np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
    return out.reshape((ho, wo) + page.shape[2:])


def resize_factor(page, fx, fy=None):
    """cv2.resize(page, None, fx=fx, fy=fy, interpolation=INTER_CUBIC)."""
    fy = fx if fy is None else fy
    ho, wo = out_size(page.shape[0], page.shape[1], fx, fy)
    return resize(page, ho, wo, 1.0 / float(fx), 1.0 / float(fy))


def resize_dsize(page, dsize):
    """cv2.resize(page, (width, height), interpolation=INTER_CUBIC)."""
    wo, ho = dsize
    return resize(page, ho, wo, page.shape[1] / float(wo), page.shape[0] / float(ho))
