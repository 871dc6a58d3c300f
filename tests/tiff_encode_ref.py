"""Reference helper of the Group 4 TIFF encoder tests (no test here): the corpus of pages and settings that
tests/test_tiff_encode_host.py and tests/test_gpu_tiff_encode.py share, the gray rule and the mask restated in NumPy, Pillow's file of
a mask, and the parity checks (strip payloads by tags 273 / 279, tag dictionaries apart from 273).  The yardstick is Pillow / libtiff:
Image.fromarray(mask).save(f, "TIFF", compression="group4", tiffinfo={262: photometric, 278: rows_per_strip})."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np
from PIL import Image

import tiff_ref as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDTHS = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)          # word and byte edges of the bitmap
HEIGHTS = (1, 2, 3, 63, 64, 65, 130)                                            # strip edges, the last short strip, the single strip
DENSITIES = (0.02, 0.5, 0.98)
THRESHOLDS = (1, 128, 255)

Case = namedtuple("Case", "label page threshold rows_per_strip photometric")


def rows_per_strip_values(h):
    return (1, 2, 3, 64, h, h + 7)


def gray_of(page):
    """The project's gray rule (skw_gray3 of csrc/rtn_skew.h) of a (H,W,3) B,G,R page; a gray page as it is."""
    if page.ndim == 2:
        return page.astype(np.int64)
    p = page.astype(np.int64)
    return (1868 * p[:, :, 0] + 9617 * p[:, :, 1] + 4899 * p[:, :, 2] + 8192) >> 14


def mask_of(case):
    """True where gray is at least the threshold (not ink)."""
    return gray_of(case.page) >= case.threshold


def pillow_file(case):
    return T.pillow_tiff(Image.fromarray(mask_of(case)), "group4", {262: case.photometric, 278: case.rows_per_strip})


def strips_of(data):
    f = T.read_fields(data)
    return [data[o:o + c] for o, c in zip(f[273][1], f[279][1])]


def fields_but_offsets(data):
    f = T.read_fields(data)
    del f[273]
    return f


def random_page(rng, w, h, density, threshold, bgr):
    """A page whose share of ink (gray < threshold) is about `density`: gray values on either side of the threshold, as B,G,R with
    the channels spread around the gray value."""
    ink = rng.random_sample((h, w)) < density
    v = np.where(ink, rng.randint(0, threshold, (h, w)), rng.randint(threshold, 256, (h, w))).astype(np.int64)
    if not bgr:
        return v.astype(np.uint8)
    return np.clip(v[:, :, None] + rng.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


def bilevel(mask_white):
    """A gray page of 0 (ink) and 255 from a boolean array that is True where the page is white."""
    return np.where(mask_white, 255, 0).astype(np.uint8)


def structured_pages():
    """[(name, gray page)]: each names a place where the coder can go wrong."""
    pages = []
    pages.append(("all white", bilevel(np.ones((5, 70), bool))))
    pages.append(("all black", bilevel(np.zeros((5, 70), bool))))
    w = np.ones((9, 70), bool)                                                  # rows that start black: 1 .. 70 pixels, a whole row
    for y, k in enumerate((1, 2, 3, 8, 63, 64, 65, 69, 70)):
        w[y, :k] = False
    pages.append(("rows start black", bilevel(w)))
    # a bar whose two edges shift by -4 .. +4 from row to row: each of the seven vertical codes and both sides of the switch to
    # horizontal mode, for an edge to black and an edge to white
    deltas = [0, 1, 2, 3, 4, -1, -2, -3, -4, 4, 3, -3, -4, 2, -2, 1, -1, 0]
    w = np.ones((len(deltas), 90), bool)
    e = 30
    for y, d in enumerate(deltas):
        e += d
        w[y, e:e + 12 + (y % 3)] = False
    pages.append(("staircase", bilevel(w)))
    w = np.ones((4, 40), bool)                                                  # pass mode: ink in the reference row, none below it
    w[0, 10:20] = False
    w[2, 5:8] = False
    w[2, 30:33] = False
    w[3, 32:36] = False
    pages.append(("pass", bilevel(w)))
    # long runs: full-width runs, a run of exactly 2560, runs of 2623 and 2624 (the repeated make-up code and its boundary)
    w = np.ones((4, 2700), bool)
    w[1, :] = False
    w[2, 2560:] = False
    w[3, :2623] = False
    pages.append(("2700 x 4", bilevel(w)))
    w = np.ones((4, 5300), bool)
    w[0, :] = False
    w[1, 2624:] = False
    w[2, :2623] = False
    w[2, 2623 + 2624:] = False
    pages.append(("5300 x 4", bilevel(w)))
    pages.append(("sample crop", np.ascontiguousarray(np.load(os.path.join(GOLDEN, "sample_page_crop.npz"))["orig_gray"])))
    return pages


_corpus = None


def corpus():
    """[Case]: WIDTHS x HEIGHTS x rows per strip 1, 2, 3, 64, H, H + 7 on random pages, with ink density, photometric, gray / B,G,R
    input and threshold taking turns so that every value meets every width, height and strip height; then the structured pages with
    both photometrics at rows per strip 1, 3, 64 and H.  Built once and shared (nobody changes it)."""
    global _corpus
    if _corpus is not None:
        return _corpus
    rng = np.random.RandomState(0)
    cases, k = [], 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for rps in rows_per_strip_values(h):
                k += 1
                density, t = DENSITIES[k % 3], THRESHOLDS[(k // 3) % 3]
                photometric, bgr = (k // 2) & 1, bool((k // 5) & 1)
                page = random_page(rng, w, h, density, t, bgr)
                cases.append(Case("%dx%d rps %d density %.2f t %d photometric %d %s" % (w, h, rps, density, t, photometric, "bgr" if bgr else "gray"),
                                  page, t, rps, photometric))
    for name, page in structured_pages():
        h = page.shape[0]
        for rps in sorted({1, 3, 64, h}):
            if name == "sample crop" and rps < 64:
                continue                                                        # 640 rows: the strip edges are covered above
            for photometric in (0, 1):
                cases.append(Case("%s rps %d photometric %d" % (name, rps, photometric), page, 128, rps, photometric))
    _corpus = cases
    return cases


def mixed_batch():
    """Cases of at least four sizes for one call: the per-page tables and scans."""
    cs = corpus()
    pick = [c for c in cs if c.label.startswith(("1x1 ", "33x65 ", "129x130 ", "200x64 ", "2700 x 4 rps 3 ", "5300 x 4 rps 1 ", "staircase rps 3 "))]
    assert len({c.page.shape[:2] for c in pick}) >= 4
    return pick


def twin_file(pkg, case, guard=64):
    """The CPU twin's file of a case (rtn_tiff_encode_host into exactly rtn_tiff_encode_bound bytes; the guard bytes must stay)."""
    L = pkg._lib.lib
    page = np.ascontiguousarray(case.page)
    h, w = page.shape[:2]
    bound = int(L.rtn_tiff_encode_bound(w, h, case.rows_per_strip))
    assert bound > 0, case.label
    out = np.full(bound + 2 * guard, 0xa5, np.uint8)
    n = C.c_size_t(0)
    rc = L.rtn_tiff_encode_host(w, h, 1 if page.ndim == 2 else 3, page.ctypes.data, case.threshold, case.rows_per_strip, case.photometric,
                                out.ctypes.data + guard, bound, C.byref(n))
    assert rc == 0, (case.label, L.rtn_last_error(None))
    assert 0 < n.value <= bound, (case.label, n.value, bound)
    assert (out[:guard] == 0xa5).all() and (out[guard + bound:] == 0xa5).all(), case.label
    return out[guard:guard + n.value].tobytes()


def check_parity(data, case):
    """Payload parity (strip for strip, byte for byte) and field parity (every tag but 273) with Pillow's file of the case's mask."""
    want = pillow_file(case)
    assert strips_of(data) == strips_of(want), case.label
    assert fields_but_offsets(data) == fields_but_offsets(want), case.label
