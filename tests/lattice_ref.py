"""NumPy oracle of table structure, written from the rules in the docstring of model/structure.py and independent
of the twins' code: an integral image for the box sum, whole-array shifts for the openings, array slices for the edges and the
cells, plain loops for the runs, a flood fill over the grid for the merged cells."""
import math

import numpy as np

MIN_SIDE = 30


def gray(page):
    page = np.asarray(page)
    if page.ndim == 2:
        return page.astype(np.int64)
    p = page.astype(np.int64)
    return (1868 * p[..., 0] + 9617 * p[..., 1] + 4899 * p[..., 2] + 8192) >> 14


def page_bw(page):
    """Rule 2: the thresholded image of the whole page, bool."""
    g = 255 - gray(page)
    H, W = g.shape
    e = np.pad(g, 7, mode="edge")
    I = np.zeros((H + 15, W + 15), np.int64)
    I[1:, 1:] = e.cumsum(0).cumsum(1)
    S = I[15:, 15:] - I[:-15, 15:] - I[15:, :-15] + I[:-15, :-15]
    return g - (2 * S + 225) // 450 > 2


def shifted(a, d, fill):
    """out[..., x] = a[..., x + d], `fill` outside."""
    out = np.full(a.shape, fill, bool)
    n = a.shape[-1]
    if d >= 0:
        out[..., :max(n - d, 0)] = a[..., d:]
    else:
        out[..., -d:] = a[..., :max(n + d, 0)]
    return out


def opened(a, L, axis):
    """Rule 3: erode then dilate along `axis` by the window [x - L // 2, x - L // 2 + L - 1]; positions outside are ignored."""
    a = np.moveaxis(a, axis, -1)
    lo = -(L // 2)
    er = np.ones(a.shape, bool)
    for d in range(lo, lo + L):
        er &= shifted(a, d, True)
    di = np.zeros(a.shape, bool)
    for d in range(lo, lo + L):
        di |= shifted(er, d, False)
    return np.moveaxis(di, -1, axis)


def crop_of(box, H, W, margin):
    x1, y1, x2, y2 = box
    xa, ya = max(0, math.floor(x1) - margin), max(0, math.floor(y1) - margin)
    xb, yb = min(W, math.ceil(x2) + margin), min(H, math.ceil(y2) + margin)
    return int(xa), int(ya), int(xb - xa), int(yb - ya)


def lattice_runs(profile, tol):
    """Rule 5."""
    runs = []
    for i, v in enumerate(profile):
        if v <= 0:
            continue
        if runs and i - runs[-1][1] - 1 <= tol:
            runs[-1][1] = i
        else:
            runs.append([i, i])
    return np.array(runs, np.int32).reshape(-1, 2)


def stream_runs(profile, gap):
    """Rule 9."""
    inked = [i for i, v in enumerate(profile) if v > 0]
    if not inked:
        return np.zeros((0, 2), np.int32)
    runs = [[0, inked[0] - 1]]
    for a, b in zip(inked[:-1], inked[1:]):
        if b - a - 1 >= gap:
            runs.append([a + 1, b - 1])
    runs.append([inked[-1] + 1, len(profile) - 1])
    return np.array(runs, np.int32).reshape(-1, 2)


def edges_of(hm, vm, rows, cols, tol, cover):
    """Rule 6 on the crop's masks; rows, cols in crop coordinates."""
    h, w = hm.shape
    R, C = len(rows), len(cols)
    h_edges, v_edges = np.zeros((R, C - 1), bool), np.zeros((R - 1, C), bool)
    for r in range(R):
        band = hm[max(rows[r][0] - tol, 0):min(rows[r][1] + tol, h - 1) + 1]
        for c in range(C - 1):
            span = band[:, cols[c][1] + 1:cols[c + 1][0]]
            h_edges[r, c] = 100 * int(span.any(axis=0).sum()) >= cover * span.shape[1]
    for c in range(C):
        band = vm[:, max(cols[c][0] - tol, 0):min(cols[c][1] + tol, w - 1) + 1]
        for r in range(R - 1):
            span = band[rows[r][1] + 1:rows[r + 1][0]]
            v_edges[r, c] = 100 * int(span.any(axis=1).sum()) >= cover * span.shape[0]
    return h_edges, v_edges


def cells_of(ink, rows, cols, x0, y0):
    """Rule 7."""
    R, C = len(rows), len(cols)
    count, box = np.zeros((R - 1, C - 1), np.int32), np.zeros((R - 1, C - 1, 4), np.int32)
    for r in range(R - 1):
        for c in range(C - 1):
            ya, xa = rows[r][1] + 1, cols[c][1] + 1
            cell = ink[ya:rows[r + 1][0], xa:cols[c + 1][0]]
            count[r, c] = cell.sum()
            if count[r, c]:
                ys, xs = np.nonzero(cell)
                box[r, c] = (x0 + xa + xs.min(), y0 + ya + ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1)
    return count, box


def merged(rows, cols, h_edges, v_edges, count, box, stream):
    """Rule 8 by flood fill; tuples (r0, c0, r1, c1, x1, y1, x2, y2, ink, ink_box, rect), rows and cols in page coordinates."""
    nr, nc = len(rows) - 1, len(cols) - 1
    seen = np.zeros((nr, nc), bool)
    out = []
    for r in range(nr):
        for c in range(nc):
            if seen[r, c]:
                continue
            group, stack = [], [(r, c)]
            seen[r, c] = True
            while stack:
                y, x = stack.pop()
                group.append((y, x))
                nbrs = [] if stream else [(y, x + 1, x + 1 < nc and not v_edges[y, x + 1]), (y, x - 1, x > 0 and not v_edges[y, x]),
                                          (y + 1, x, y + 1 < nr and not h_edges[y + 1, x]), (y - 1, x, y > 0 and not h_edges[y, x])]
                for ny, nx, joined in nbrs:
                    if joined and not seen[ny, nx]:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
            r0, r1 = min(g[0] for g in group), max(g[0] for g in group)
            c0, c1 = min(g[1] for g in group), max(g[1] for g in group)
            inked = [g for g in group if count[g]]
            ink = int(sum(count[g] for g in inked))
            if inked:
                xa, ya = min(box[g][0] for g in inked), min(box[g][1] for g in inked)
                xb, yb = max(box[g][0] + box[g][2] for g in inked), max(box[g][1] + box[g][3] for g in inked)
                ink_box = (int(xa), int(ya), int(xb - xa), int(yb - ya))
            else:
                ink_box = (0, 0, 0, 0)
            mid = lambda run: int((int(run[0]) + int(run[1])) // 2)
            out.append((r0, c0, r1, c1, mid(cols[c0]), mid(rows[r0]), mid(cols[c1 + 1]), mid(rows[r1 + 1]), ink, ink_box,
                        len(group) == (r1 - r0 + 1) * (c1 - c0 + 1)))
    return out


NONE = dict(flavor="none", rows=np.zeros((0, 2), np.int32), cols=np.zeros((0, 2), np.int32), h_edges=np.zeros((0, 0), bool),
            v_edges=np.zeros((0, 0), bool), cell_ink=np.zeros((0, 0), np.int32), cell_ink_box=np.zeros((0, 0, 4), np.int32), cells=[])


def grid(page, box, flavor="auto", line_scale=15, line_tol=2, cover=50, col_gap=12, row_gap=4, margin=10, bw=None):
    """Rules 1-10 for one box of one page -> a dict with TableGrid's fields, plus crop and, for a crop of 30 x 30 or more, the masks
    (uint8 0 / 255) and the four profiles.  bw: page_bw(page) when the caller has it."""
    H, W = np.asarray(page).shape[:2]
    x0, y0, w, h = crop_of(box, H, W, margin)
    if w < MIN_SIDE or h < MIN_SIDE:
        return dict(NONE, crop=(x0, y0, w, h))
    bw = (page_bw(page) if bw is None else bw)[y0:y0 + h, x0:x0 + w]
    hm, vm = opened(bw, w // line_scale, 1), opened(bw, h // line_scale, 0)
    ink = bw & ~hm & ~vm
    prof = dict(rowH=hm.sum(1).astype(np.int32), rowInk=ink.sum(1).astype(np.int32), colV=vm.sum(0).astype(np.int32),
                colInk=ink.sum(0).astype(np.int32))
    out = dict(NONE, crop=(x0, y0, w, h), masks={k: np.where(v, 255, 0).astype(np.uint8) for k, v in (("bw", bw), ("hm", hm), ("vm", vm), ("ink", ink))},
               profiles=prof)
    got, rows, cols = "none", None, None
    if flavor != "stream":
        rows, cols = lattice_runs(prof["rowH"], line_tol), lattice_runs(prof["colV"], line_tol)
        if len(rows) >= 2 and len(cols) >= 2:
            got = "lattice"
    if got == "none" and flavor != "lattice":
        rows, cols = stream_runs(prof["rowInk"], row_gap), stream_runs(prof["colInk"], col_gap)
        if len(rows):
            got = "stream"
    if got == "none":
        return out
    if got == "lattice":
        h_edges, v_edges = edges_of(hm, vm, rows, cols, line_tol, cover)
    else:
        h_edges, v_edges = np.zeros((len(rows), len(cols) - 1), bool), np.zeros((len(rows) - 1, len(cols)), bool)
    count, box4 = cells_of(ink, rows, cols, x0, y0)
    prow, pcol = (rows + np.int32(y0)).astype(np.int32), (cols + np.int32(x0)).astype(np.int32)
    out.update(flavor=got, rows=prow, cols=pcol, h_edges=h_edges, v_edges=v_edges, cell_ink=count, cell_ink_box=box4,
               cells=merged(prow, pcol, h_edges, v_edges, count, box4, got == "stream"))
    return out


def csv_text(g):
    lines = ["row,col,rowspan,colspan,x1,y1,x2,y2,ink,ink_x,ink_y,ink_w,ink_h"]
    for (r0, c0, r1, c1, x1, y1, x2, y2, ink, ink_box, _rect) in g["cells"]:
        lines.append(",".join(str(v) for v in (r0, c0, r1 - r0 + 1, c1 - c0 + 1, x1, y1, x2, y2, ink) + tuple(ink_box)))
    return "\n".join(lines) + "\n"


def outline(page, boxes):
    """draw_box's bands of thickness 2 from (x, y) to (x + w, y + h): rows / columns [e - 1, e + 1) around every edge, (0, 255, 0)."""
    out = np.array(page)
    H, W = out.shape[:2]
    colour = (0, 255, 0) if out.ndim == 3 else 255
    for x, y, w, h in boxes:
        x2, y2 = x + w, y + h
        for ya, yb, xa, xb in ((y - 1, y + 1, x - 1, x2 + 1), (y2 - 1, y2 + 1, x - 1, x2 + 1), (y - 1, y2 + 1, x - 1, x + 1), (y - 1, y2 + 1, x2 - 1, x2 + 1)):
            ya, xa, yb, xb = max(ya, 0), max(xa, 0), min(yb, H), min(xb, W)
            if ya < yb and xa < xb:
                out[ya:yb, xa:xb] = colour
    return out
