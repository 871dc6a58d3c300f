"""NumPy / scipy oracle of scan analysis (connectedComponentAnalysis.py), written from the definitions in the
docstring of model/components.py and independent of the twins' code: whole-array shifts instead of prefix counts, scipy.ndimage
labelling (3x3 structure for the foreground, the cross for the background) instead of flood fill or union-find."""
import numpy as np
from scipy import ndimage

CROSS = ndimage.generate_binary_structure(2, 1)
FULL = np.ones((3, 3), bool)
BINS, RANGE = 25, (0, 100)


def gray(page):
    page = np.asarray(page)
    if page.ndim == 2:
        return page.copy()
    p = page.astype(np.int64)
    return ((1868 * p[..., 0] + 9617 * p[..., 1] + 4899 * p[..., 2] + 8192) >> 14).astype(np.uint8)


def win(a, L, anchor, axis, op):
    """op over a[x - anchor .. x - anchor + L - 1] along `axis`; positions outside the image are ignored."""
    a = np.moveaxis(np.asarray(a).astype(np.int64), axis, -1)
    n = a.shape[-1]
    neutral = 1 << 40 if op is np.minimum else -(1 << 40)
    padded = np.full(a.shape[:-1] + (n + 2 * L,), neutral, np.int64)
    padded[..., L:L + n] = a
    out = np.full(a.shape, neutral, np.int64)
    for d in range(L):
        s = L + d - anchor
        out = op(out, padded[..., s:s + n])
    return np.moveaxis(out, -1, axis).astype(np.uint8)


def erode(a, L, anchor, axis):
    return win(a, L, anchor, axis, np.minimum)


def dilate(a, L, anchor, axis):
    return win(a, L, anchor, axis, np.maximum)


def line_masks(page):
    """-> (bw, horizontal, vertical) of process_graphical_lines."""
    g = 255 - gray(page).astype(np.int64)
    H, W = g.shape
    e = np.pad(g, 7, mode="edge")
    S = sum(e[dy:dy + H, dx:dx + W] for dy in range(15) for dx in range(15))
    mean = (2 * S + 225) // 450
    bw = np.where(g - mean > 2, 255, 0).astype(np.uint8)
    Lh, Lv = W // 30, H // 30
    horizontal = dilate(erode(bw, Lh, Lh // 2, 1), Lh, Lh // 2, 1)
    vertical = dilate(erode(bw, Lv, Lv // 2, 0), Lv, Lv // 2, 0)
    return bw, horizontal, vertical


def components(mask, external_only=True):
    """findContours + boundingRect: int32 (n, 4) boxes x, y, w, h of the 8-connected components of mask != 0, ordered by the raster
    index of their first pixel; with external_only those with a pixel 4-adjacent to the background region of the frame."""
    fg = np.pad(np.asarray(mask) != 0, 1)
    lab, n = ndimage.label(fg, structure=FULL)
    if n == 0:
        return np.zeros((0, 4), np.int32)
    keep = np.ones(n + 1, bool)
    if external_only:
        bg, _nb = ndimage.label(~fg, structure=CROSS)
        frame = bg == bg[0, 0]
        near = ndimage.binary_dilation(frame, structure=CROSS) & fg
        keep[:] = False
        keep[np.unique(lab[near])] = True
    keep[0] = False
    ids, first = np.unique(lab.ravel(), return_index=True)
    order = [int(i) for i in ids[np.argsort(first, kind="stable")] if keep[i]]
    slices = ndimage.find_objects(lab)
    out = [(slices[i - 1][1].start - 1, slices[i - 1][0].start - 1, slices[i - 1][1].stop - slices[i - 1][1].start,
            slices[i - 1][0].stop - slices[i - 1][0].start) for i in order]
    return np.asarray(out, np.int32).reshape(-1, 4)


def components_by_hole_filling(mask):
    """The alternative definition of external: a component is not external iff it lies inside binary_fill_holes of another one."""
    fg = np.asarray(mask) != 0
    lab, n = ndimage.label(fg, structure=FULL)
    inside = np.zeros(n + 1, bool)
    for i in range(1, n + 1):
        comp = lab == i
        holes = ndimage.binary_fill_holes(comp) & ~comp
        inside[np.unique(lab[holes])] = True
    inside[0] = True
    ids, first = np.unique(lab.ravel(), return_index=True)
    order = [int(i) for i in ids[np.argsort(first, kind="stable")] if not inside[i]]
    slices = ndimage.find_objects(lab)
    out = [(slices[i - 1][1].start, slices[i - 1][0].start, slices[i - 1][1].stop - slices[i - 1][1].start,
            slices[i - 1][0].stop - slices[i - 1][0].start) for i in order]
    return np.asarray(out, np.int32).reshape(-1, 4)


def remove_lines(page):
    """process_graphical_lines -> (cleaned page, boxes: horizontal components first, then vertical)."""
    _bw, horizontal, vertical = line_masks(page)
    boxes = np.concatenate([components(horizontal), components(vertical)])
    out = np.array(page, copy=True)
    for x, y, w, h in boxes:
        out[y:y + h, x:x + w] = 255
    return out, boxes


def blur_taps():
    """GaussianBlur((5, 5), 0.5) in 8-bit fixed point: exp(-x^2 / 0.5) normalised, times 256, rounded, centre takes the remainder."""
    k = np.exp(-np.arange(-2, 3) ** 2 / 0.5)
    t = np.rint(k / k.sum() * 256).astype(np.int64)
    t[2] += 256 - t.sum()
    return t


def text_stages(page):
    """-> (blurred, blackhat, thresholded, dilated, closed) of process_image."""
    g = gray(page).astype(np.int64)
    H, W = g.shape
    t = blur_taps()
    e = np.pad(g, ((0, 0), (2, 2)), mode="reflect")
    rows = sum(t[i] * e[:, i:i + W] for i in range(5))
    e = np.pad(rows, ((2, 2), (0, 0)), mode="reflect")
    blurred = ((sum(t[i] * e[i:i + H] for i in range(5)) + 32768) >> 16).astype(np.uint8)
    closed4 = erode(dilate(blurred, 4, 2, 1), 4, 2, 1)
    blackhat = np.maximum(closed4.astype(np.int64) - blurred, 0).astype(np.uint8)
    th = np.where(blackhat > 10, 255, 0).astype(np.uint8)
    dil = th
    for _ in range(9):                                   # the iterated form: 9 times the 1x4 element anchored at 2
        dil = dilate(dil, 4, 2, 1)
    closed = dil
    for _ in range(2):
        closed = erode(dilate(closed, 10, 5, 1), 10, 5, 1)
    return blurred, blackhat, th, dil, closed


def text_boxes(page):
    return components(text_stages(page)[4])


def kept(boxes):
    return np.asarray([b for b in boxes if b[2] > b[3] and b[3] > 0 and int(b[2]) * int(b[3]) > 500], np.int32).reshape(-1, 4)


def outline(page, boxes):
    """cv2.rectangle(page, (x, y), (x + w, y + h), (0, 255, 0), 2) by the band rule: bands of 2 centred on the four edges."""
    out = np.array(page, copy=True)
    H, W = out.shape[:2]
    colour = (0, 255, 0) if out.ndim == 3 else 255
    for x, y, w, h in boxes:
        x1, y1, x2, y2 = int(x), int(y), int(x + w), int(y + h)
        for ya, yb, xa, xb in ((y1 - 1, y1 + 1, x1 - 1, x2 + 1), (y2 - 1, y2 + 1, x1 - 1, x2 + 1), (y1 - 1, y2 + 1, x1 - 1, x1 + 1),
                               (y1 - 1, y2 + 1, x2 - 1, x2 + 1)):
            ya, yb, xa, xb = max(ya, 0), min(yb, H), max(xa, 0), min(xb, W)
            if ya < yb and xa < xb:
                out[ya:yb, xa:xb] = colour
    return out


def histogram(heights):
    counts, edges = np.histogram(np.asarray(heights, np.float64), BINS, RANGE)
    k = int(np.argmax(counts))
    return counts, int(edges[k]), int(edges[k]) + (RANGE[1] - RANGE[0]) // BINS


def analyse(page):
    """main()'s chain for one page."""
    cleaned, line_boxes = remove_lines(page)
    boxes = text_boxes(cleaned)
    k = kept(boxes)
    counts, lo, hi = histogram(k[:, 3])
    return {"line_boxes": line_boxes, "cleaned": cleaned, "text_boxes": boxes, "heights": k[:, 3].copy(), "histogram": counts,
            "mode_bin": (lo, hi), "annotated": outline(cleaned, k)}
