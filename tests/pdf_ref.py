"""A NumPy oracle of model/pdf.py's page geometry and of the compose step (csrc/rtn_compose.hip): np.rot90, flips and slicing, and
the two box mappings restated from the reference's PDFCSVtoImageCSV.  Nothing here looks at orientation codes to place an image on a
page: render() goes from the CTM's corners."""
import math

import numpy as np


def half_up(v):
    return int(math.floor(v + 0.5))


def oriented(S, code):
    """The oriented image of a (h, w, 3) array under TIFF / EXIF orientation `code`."""
    return {1: S, 2: S[:, ::-1], 3: S[::-1, ::-1], 4: S[::-1], 5: S.transpose(1, 0, 2), 6: np.rot90(S, -1), 7: np.rot90(S, -1)[::-1],
            8: np.rot90(S, 1)}[code]


def compose(pages_hw, items):
    """rtn_page_compose: pages_hw [(H, W)], items [(S, code, invert, page, x, y, crop_x, crop_y, crop_w, crop_h)] -> the pages."""
    out = [np.full((h, w, 3), 255, np.uint8) for h, w in pages_hw]
    for S, code, invert, page, x, y, cx, cy, cw, ch in items:
        O = oriented(S, code)[cy:cy + ch, cx:cx + cw]
        out[page][y:y + ch, x:x + cw] = 255 - O if invert else O
    return out


def apply(m, x, y):
    a, b, c, d, e, f = m
    return a * x + c * y + e, b * x + d * y + f


def turned(S, ctm):
    """The image as the CTM shows it on a page whose y runs upwards, from where its corners go: image space is the unit square with
    the first row at y = 1."""
    tl, tr, bl = apply(ctm, 0, 1), apply(ctm, 1, 1), apply(ctm, 0, 0)
    dcol, drow = (tr[0] - tl[0], tr[1] - tl[1]), (bl[0] - tl[0], bl[1] - tl[1])
    if abs(dcol[0]) > abs(dcol[1]):                    # columns run along the page's x
        O = S
        if dcol[0] < 0:
            O = O[:, ::-1]
        if drow[1] > 0:                                # rows run up the page
            O = O[::-1]
    else:
        O = S.transpose(1, 0, 2)
        if dcol[1] > 0:                                # columns run up the page
            O = O[::-1]
        if drow[0] < 0:                                # rows run to the left
            O = O[:, ::-1]
    return O


def render(media_box, rotate, draws):
    """The page model/pdf.py must give: draws [(S (h, w, 3) B,G,R as the page shows it, CTM)], the first one setting the scale."""
    x0, y0, x1, y1 = media_box
    canvas = None
    for S, ctm in draws:
        O = turned(S, ctm)
        xs, ys = zip(*[apply(ctm, u, v) for u in (0, 1) for v in (0, 1)])
        if canvas is None:
            sx, sy = O.shape[1] / (max(xs) - min(xs)), O.shape[0] / (max(ys) - min(ys))
            W, H = half_up((x1 - x0) * sx), half_up((y1 - y0) * sy)
            canvas = np.full((H, W, 3), 255, np.uint8)
        left, top = half_up((min(xs) - x0) * sx), half_up((y1 - max(ys)) * sy)
        oh, ow = O.shape[:2]
        cy0, cx0, cy1, cx1 = max(0, -top), max(0, -left), min(oh, H - top), min(ow, W - left)
        if cy0 < cy1 and cx0 < cx1:
            canvas[top + cy0:top + cy1, left + cx0:left + cx1] = O[cy0:cy1, cx0:cx1]
    return np.ascontiguousarray(np.rot90(canvas, -((rotate % 360) // 90)))


def reference_pixels(box_pt, scale, h):
    """PDFCSVtoImageCSV's two formulas on one box (xmin, ymin, xmax, ymax) in points: x = int(scale x), y = h - int(scale y), the
    upper edge (ymax) becoming ymin."""
    xmin, ymin, xmax, ymax = box_pt
    return (int(scale * int(xmin)), h - int(scale * int(ymax)), int(scale * int(xmax)), h - int(scale * int(ymin)))


def pixels_to_points(box_px, media_box, sx, sy, rotate, size_as_read):
    """A pixel box (x1, y1, x2, y2) on the page as read (W x H after /Rotate) -> (x1, y1, x2, y2) in points of the unrotated user
    space, y upwards: the corners are turned back one quarter at a time, then scaled."""
    W, H = size_as_read
    pts = [(box_px[0], box_px[1]), (box_px[2], box_px[3])]
    for _ in range((rotate % 360) // 90):              # the page as read is the earlier one turned clockwise: (x, y) <- (H0 - y0, x0)
        pts = [(y, W - x) for x, y in pts]
        W, H = H, W
    xs = [media_box[0] + x / sx for x, _ in pts]
    ys = [media_box[1] + (H - y) / sy for _, y in pts]
    return (min(xs), min(ys), max(xs), max(ys))
