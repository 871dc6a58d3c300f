"""CPU: tests/jpeg_encode_ref.py, the NumPy restatement of the encoder's rules used to locate a device mismatch to a stage, gives
Pillow's entropy-coded segment byte for byte on small pages of every mode (edge blocks, dummy blocks, stuffing included)."""
import io

import numpy as np
import pytest
from PIL import Image, features

import jpeg_encode_ref as R

if not features.check_feature("libjpeg_turbo"):
    pytest.skip("Pillow is not linked against libjpeg-turbo: the restatement is libjpeg-turbo's encoder",
                allow_module_level=True)


def pillow_scan(page, q, ss):
    b = io.BytesIO()
    Image.fromarray(page[:, :, ::-1] if page.ndim == 3 else page).save(b, "JPEG", quality=q, subsampling=ss)
    d = b.getvalue()
    p = 2
    while d[p + 1] != 0xDA:
        p += 2 + ((d[p + 2] << 8) | d[p + 3])
    p += 2 + ((d[p + 2] << 8) | d[p + 3])
    return d[p:-2]


@pytest.mark.parametrize("hw", [(1, 1), (8, 8), (9, 17), (17, 9), (24, 40), (37, 53)])
def test_restatement_equals_pillow(hw):
    rng = np.random.RandomState(hw[0] * 100 + hw[1])
    h, w = hw
    noise = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    smooth = np.kron(np.clip(rng.exponential(12.0, (h // 8 + 2, w // 8 + 2, 3)) * 6, 0, 255), np.ones((8, 8, 1)))[:h, :w]
    for img in (noise, smooth.astype(np.uint8)):
        for q in (10, 50, 95, 100):
            for ss in (0, 1, 2):
                want = pillow_scan(img, q, ss)
                assert R.scan(R.coefficients(img, q, ss), 3, ss) == want, (hw, q, ss)
            gray = np.ascontiguousarray(img[..., 1])
            assert R.scan(R.coefficients(gray, q, 2), 1, 2) == pillow_scan(gray, q, 2), (hw, q, "gray")
