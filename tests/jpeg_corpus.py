"""The JPEG files that tests/test_gpu_jpeg.py (device) and tests/test_jpeg_decode_host.py (CPU twin) decode: everything Pillow writes
here, every sampling, quality, optimize and restart setting, sizes from 1x1 to a 2200x1712 page, smooth / page / noise / constant
content, and the two sample pages of tests/golden."""
import io
import os

import numpy as np
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def encode(img, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


_crop = None


def content(kind, h, w, rng):
    global _crop
    if kind == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "const":
        return np.full((h, w, 3), (23, 200, 141), np.uint8)
    if kind in ("crop", "crop_gray"):
        if _crop is None:
            _crop = np.load(os.path.join(GOLDEN, "sample_page_crop.npz"))
        c = _crop["processed_rgb"] if kind == "crop" else np.repeat(_crop["orig_gray"][..., None], 3, -1)
        return np.ascontiguousarray(np.tile(c, (h // c.shape[0] + 1, w // c.shape[1] + 1, 1))[:h, :w])
    # DT-like smooth pages (the generator tests' recipe)
    base = np.clip(rng.exponential(12.0, (h // 8 + 2, w // 8 + 2, 3)) * 6, 0, 255)
    return np.kron(base, np.ones((8, 8, 1)))[:h, :w].astype(np.uint8)


RESTARTS = [{}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 7}, {"restart_marker_rows": 1}]


def try_encode(img, gray, **kw):
    try:
        return encode(img[..., 0] if gray else img, **kw)
    except OSError:                     # Pillow cannot write some restart settings for tiny images
        return None


def build_corpus(d):
    """Paths of every file the bit-exactness tests decode, written into directory d (a pathlib.Path)."""
    rng = np.random.RandomState(0)
    files = []
    # every encoder setting on two contents
    for kind in ("smooth", "noise"):
        img = content(kind, 33, 47, rng)
        for ss in (0, 1, 2, None):
            for q in (50, 75, 95, 100):
                for opt in (False, True):
                    for rs in RESTARTS:
                        kw = dict(quality=q, optimize=opt, **rs)
                        if ss is not None:
                            kw["subsampling"] = ss
                        data = try_encode(img, ss is None, **kw)
                        if data is not None:
                            files.append(data)
    # every size and content, the settings rotating
    k = 0
    for (h, w) in ((1, 1), (1, 17), (17, 1), (8, 8), (15, 17), (16, 16), (33, 47), (250, 333)):
        for kind in ("smooth", "crop", "crop_gray", "noise", "const"):
            img = content(kind, h, w, rng)
            for ss in (0, 1, 2):
                k += 1
                kw = dict(quality=(50, 75, 95, 100)[k % 4], optimize=bool(k % 2), subsampling=ss, **RESTARTS[k % 4])
                data = try_encode(img, False, **kw)
                if data is not None:
                    files.append(data)
            data = try_encode(img, True, quality=(50, 75, 95, 100)[k % 4], **RESTARTS[(k + 1) % 4])
            if data is not None:
                files.append(data)
    files.append(encode(content("crop", 1712, 2200, rng), quality=95, subsampling=2))
    paths = []
    for i, data in enumerate(files):
        p = d / ("f%03d.jpg" % i)
        p.write_bytes(data)
        paths.append(str(p))
    paths += [os.path.join(GOLDEN, "sample_0717_023.jpg"), os.path.join(GOLDEN, "sample_0717_023_orig.jpg")]
    return paths
