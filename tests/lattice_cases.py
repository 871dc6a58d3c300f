"""The inputs the table-structure tests share (tests/test_lattice_ref.py, test_lattice_host.py, test_gpu_lattice.py) and the
oracle's result for each, computed once per process.  Every synthetic page is built from known rule positions on near-white
paper whose noise (+-1) stays below the threshold, so that the expected grid follows from the construction: a horizontal rule
is longer than w // line_scale and thinner than h // line_scale (and the other way round), a text blob is smaller than both."""
import functools
import importlib
import os

import numpy as np

import lattice_ref as R

S = importlib.import_module("retinanet-for-table-detection_amd.model.structure")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def paper(h, w, gray, seed):
    rng = np.random.default_rng(seed)
    shape = (h, w) if gray else (h, w, 3)
    return (245 + rng.integers(-1, 2, shape)).astype(np.uint8), rng


def inked(img, rng, ys, xs):
    img[ys, xs] = rng.integers(10, 41, img[ys, xs].shape)


def ruled(h, w, ys, xs, thick=2, thick_of=None, blob=(4, 5), gray=False, seed=1):
    """A page with horizontal rules whose top rows are ys and vertical rules whose left columns are xs, all `thick` thick (thick_of:
    {y: thickness} for single horizontal rules), the horizontal ones from the first to the last vertical one and the other way
    round, and in every cell four blobs of blob = (width, height) pixels, 2 apart, 3 pixels inside the cell's corner."""
    img, rng = paper(h, w, gray, seed)
    t = lambda y: (thick_of or {}).get(y, thick)
    for y in ys:
        inked(img, rng, slice(y, y + t(y)), slice(xs[0], xs[-1] + thick))
    for x in xs:
        inked(img, rng, slice(ys[0], ys[-1] + t(ys[-1])), slice(x, x + thick))
    bw, bh = blob
    for ya, yb in zip(ys[:-1], ys[1:]):
        for xa, xb in zip(xs[:-1], xs[1:]):
            y0, x0 = ya + t(ya) + 3, xa + thick + 3
            for k in range(4):
                if x0 + (bw + 2) * k + bw + 3 <= xb and y0 + bh + 3 <= yb:
                    inked(img, rng, slice(y0, y0 + bh), slice(x0 + (bw + 2) * k, x0 + (bw + 2) * k + bw))
    return img


TABLE_YS, TABLE_XS = (20, 45, 70, 95, 120), (15, 70, 130, 184)
TABLE_BOX = (18, 23, 183, 119)                       # 3 px inside the frame: only the margin brings the frame into the crop


def table(erase=()):
    """The ruled 4 x 3 table on a 150 x 200 B,G,R page; erase: rectangles (y0, y1, x0, x1) painted back to paper."""
    img = ruled(150, 200, TABLE_YS, TABLE_XS)
    rng = np.random.default_rng(9)
    for y0, y1, x0, x1 in erase:
        img[y0:y1, x0:x1] = 245 + rng.integers(-1, 2, img[y0:y1, x0:x1].shape)
    return img


SPAN_ERASE = ((47, 70, 70, 72),)                                     # the vertical rule x = 70 between the rules y = 45 and y = 70
ELL_ERASE = SPAN_ERASE + ((70, 72, 72, 130),)                        # and the horizontal rule y = 70 between x = 70 and x = 130


def borderless():
    """Ink blobs in three columns [20, 60), [71, 111), [123, 163): gaps of 11 and 12; four text lines 5 tall, 15 apart."""
    img, rng = paper(120, 200, False, 2)
    for y in (20, 40, 60, 80):
        for x0 in (20, 71, 123):
            for k in range(7):
                inked(img, rng, slice(y, y + 5), slice(x0 + 6 * k, x0 + 6 * k + 4))
    return img


def long_page():
    """Gray 30 x 16384: L = 1092 along x and 2 along y, so horizontal rules are 1 thick and blobs 1 tall."""
    img, rng = paper(30, 16384, True, 3)
    for y in (4, 25):
        inked(img, rng, slice(y, y + 1), slice(100, 16002))
    for x in (100, 8000, 16000):
        inked(img, rng, slice(4, 26), slice(x, x + 2))
    for x in (300, 5000, 9000, 15000):
        inked(img, rng, slice(12, 13), slice(x, x + 5))
    return img


def golden_page():
    from PIL import Image
    with Image.open(os.path.join(ROOT, "tests", "golden", "sample_0717_023_orig.jpg")) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def case(page, boxes, ys=None, xs=None, thick=2, thick_of=None, R_=None, C_=None, **kw):
    """expect: for a lattice case the rules' rows and columns (top, thickness) in page coordinates and the numbers of separators."""
    expect = None
    if ys is not None:
        expect = dict(rows=[(y, (thick_of or {}).get(y, thick)) for y in ys], cols=[(x, thick) for x in xs],
                      R=len(ys) if R_ is None else R_, C=len(xs) if C_ is None else C_)
    return dict(page=page, boxes=np.asarray(boxes, np.float64).reshape(-1, 4), expect=expect, kw=kw)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(page, boxes (n, 4), expect, kw: table_cells' keywords), in the order of the mixed batch."""
    out = {}
    out["table"] = case(table(), [TABLE_BOX], TABLE_YS, TABLE_XS)
    out["table_span"] = case(table(SPAN_ERASE), [TABLE_BOX], TABLE_YS, TABLE_XS)
    out["table_ell"] = case(table(ELL_ERASE), [TABLE_BOX], TABLE_YS, TABLE_XS)
    # 30 x 30, the smallest crop: L = 2, rules 1 thick, one single-pixel dot
    small = ruled(30, 30, (5, 24), (3, 26), thick=1, blob=(1, 1), seed=4)
    out["crop_30x30"] = case(small, [(10, 10, 20, 20)], (5, 24), (3, 26), thick=1)
    for w in (64, 65, 257):                                                     # the crop is the page: 64 is one mask word, 65 and 257 one bit more
        out["width_%d" % w] = case(ruled(61, w, (4, 30, 55), (3, w // 2, w - 6), blob=(3, 3), seed=w), [(0, 0, w, 61)], (4, 30, 55), (3, w // 2, w - 6))
    # the frame on the crop's first and last row and column: every band is cut.  Rules 1 thick: a window cut by the border is
    # shorter, so a thicker rule on the border would pass the opening across it
    out["frame_on_border"] = case(ruled(60, 90, (0, 30, 59), (0, 44, 89), thick=1, blob=(3, 3), seed=6), [(0, 0, 90, 60)], (0, 30, 59),
                                  (0, 44, 89), thick=1)
    out["thick_rule"] = case(ruled(180, 200, (20, 60, 110, 150), (15, 100, 184), thick_of={60: 7}, seed=7), [(18, 23, 183, 149)],
                             (20, 60, 110, 150), (15, 100, 184), thick_of={60: 7})
    # rules 2 zero rows apart (40 / 44: one separator at line_tol = 2) and 3 apart (80 / 85: two)
    out["near_rules"] = case(ruled(150, 200, (20, 40, 44, 80, 85, 120), (15, 100, 184), seed=8), [(18, 23, 183, 119)],
                             (20, 40, 44, 80, 85, 120), (15, 100, 184), R_=5)
    out["box_outside"] = case(table(), [(-20.5, -5, 250, 135.2)], TABLE_YS, TABLE_XS)
    # a gray page without a box, then a B,G,R page with two overlapping boxes
    out["gray_no_box"] = case(ruled(131, 173, (10, 60, 110), (12, 90, 160), gray=True, seed=10), [])
    out["overlapping"] = case(table(), [TABLE_BOX, (60, 40, 183, 119)])
    out["borderless"] = case(borderless(), [(0, 0, 200, 120)])
    out["blank"] = case(paper(80, 90, False, 11)[0], [(5, 5, 80, 70)])
    out["gray_table"] = case(R.gray(table()).astype(np.uint8), [TABLE_BOX], TABLE_YS, TABLE_XS)
    return out


@functools.lru_cache(maxsize=None)
def long_case():
    return case(long_page(), [(0, 0, 16384, 30)], (4, 25), (100, 8000, 16000), thick=2, thick_of={4: 1, 25: 1})


GOLDEN_BOXES = ((300, 600, 1300, 900), (150.5, 200, 1550, 1000.25), (100, 1200, 900, 2000))


@functools.lru_cache(maxsize=None)
def golden_case():
    return case(golden_page(), GOLDEN_BOXES)


@functools.lru_cache(maxsize=None)
def oracle(name, flavor="auto"):
    """lattice_ref.grid for every box of a case -> list of dicts."""
    c = {"long": long_case, "golden": golden_case}[name]() if name in ("long", "golden") else cases()[name]
    bw = R.page_bw(c["page"])
    return [R.grid(c["page"], b, flavor=flavor, bw=bw, **c["kw"]) for b in c["boxes"]]


def same_grid(got, want):
    """Is a TableGrid the oracle's dict, field for field (dtypes included)?  Returns the name of the first field that differs."""
    if got.flavor != want["flavor"]:
        return "flavor"
    for key, kind in (("rows", np.int32), ("cols", np.int32), ("h_edges", bool), ("v_edges", bool), ("cell_ink", np.int32), ("cell_ink_box", np.int32)):
        a = getattr(got, key)
        if a.dtype != kind or a.shape != want[key].shape or not np.array_equal(a, want[key]):
            return key
    if [tuple(c[:9]) + (tuple(c.ink_box), bool(c.rect)) for c in got.cells] != [tuple(c[:9]) + (tuple(c[9]), bool(c[10])) for c in want["cells"]]:
        return "cells"
    return None
