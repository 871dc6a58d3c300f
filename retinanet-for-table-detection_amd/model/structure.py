"""Table structure on the device: the rows, columns and cells of every detected table.  The reference hands the
document to camelot.read_pdf (exportPDFTableDataToCSV, DetectTablesUtils.py:263-275), whose "lattice" flavour finds the ruling
lines by two morphological openings and whose "stream" flavour falls back to the gaps of the text; table_cells does both on the
page's pixels, for the boxes detect_files reports.  Launches per batch (csrc/rtn_lattice.hip): the four masks of every crop (the
threshold at the crops, transpose, the two openings, transpose back with the ink), one profile launch, one edge launch, one
cell launch.  The profiles come to the host once per call; the separator runs are host arithmetic through the C function the CPU
twins use too (rtn_lattice_separators_host), the merged cells are host arithmetic on the R x C flags.

The rules, for one box on one page of H x W (all arithmetic is integer):
  1. Crop.  x1' = max(0, x1 - margin), x2' = min(W, x2 + margin), the same for y; floats are floored for x1, y1 and ceiled for
     x2, y2.  w = x2' - x1', h = y2' - y1'.  A crop with w < 30 or h < 30 gives flavor "none" and empty arrays; it is no error.
  2. bw is the thresholded image of rtn_cca_lines_mask (the same gray, 15x15 box sum, replicated borders, > 2; see
     model/components.py) of the whole page, taken at the crop: a box border never acts as an image border.
  3. hm = bw eroded then dilated along x by the window [x - L // 2, x - L // 2 + L - 1] cut to the crop, L = w // line_scale;
     vm the same along y with L = h // line_scale; line_scale within 1 .. 30.  ink = bw & ~hm & ~vm.
  4. Profiles (int32): rowH[y] = sum_x hm, colV[x] = sum_y vm, rowInk[y], colInk[x].
  5. Lattice separators: the maximal runs of rows with rowH > 0, two runs with at most line_tol zero rows between them being one;
     rows are the runs (lo, hi), inclusive; cols the same from colV.  Lattice holds iff R >= 2 and C >= 2.
  6. Edges (lattice).  Horizontal edge (r, c), c < C - 1: the span is the columns strictly between cols[c].hi and cols[c+1].lo,
     the band the rows rows[r].lo - line_tol .. rows[r].hi + line_tol cut to the crop, covered the number of span columns with
     an hm pixel in the band; present iff 100 covered >= cover len; an empty span is present.  Vertical edges the same on vm
     with rows and columns exchanged.
  7. Cell (r, c) is the rows strictly between rows[r].hi and rows[r+1].lo and the columns strictly between cols[c].hi and
     cols[c+1].lo; cell_ink its count of ink, cell_ink_box the bounding box (x, y, w, h) of that ink in page coordinates, or
     0,0,0,0 when the count is 0.
  8. Merged cells: neighbouring cells whose shared interior edge is absent are united; the groups are ordered by the raster
     index of their first cell; r0, c0, r1, c1 is the bounding range, rect is true iff the group fills it; the outer box runs
     from the midpoints (lo + hi) // 2 of the bounding separators; ink is the sum over the group, ink_box the union.
  9. Stream separators: on colInk the leading zero run (possibly empty: hi = lo - 1), every inner zero run of at least col_gap,
     the trailing zero run (possibly empty); rows the same on rowInk with row_gap.  No ink at all gives flavor "none".  Every
     edge is reported absent and every grid cell is a merged cell of its own.  Rule 7 is unchanged.
 10. flavor "auto" is lattice where rule 5 holds and stream otherwise; "lattice" gives "none" where rule 5 fails; "stream" never
     looks at the rules.
 11. Separator and cell tables are sized here so that they cannot overflow: a run needs a position and so does a gap, so an axis
     of n holds at most (n + 1) // 2 + 1 runs (the two possibly empty ones of rule 9 included).  A C entry given less room
     returns RTN_EINVAL with the true count.

Differences from camelot: the window lengths come from the box, not from the page; the separators come from projections, not
from the joints of contours; and nothing can confirm the grids against camelot offline: PARITY UNPINNED."""
import collections
import math
import os

import numpy as np
import torch

from . import _pages, _rt
from . import components
from ._pages import Device as _Device, Twins as _Twins, i32 as _i32, pointers as _pointers, ptr as _ptr, starts as _starts

L = _rt.L

MIN_SIDE, MAX_SIDE = components.MIN_SIDE, components.MAX_SIDE
FLAVORS = ("auto", "lattice", "stream")
CSV_HEADER = "row,col,rowspan,colspan,x1,y1,x2,y2,ink,ink_x,ink_y,ink_w,ink_h"

Cell = collections.namedtuple("Cell", "r0 c0 r1 c1 x1 y1 x2 y2 ink ink_box rect")
TableGrid = collections.namedtuple("TableGrid", "flavor rows cols h_edges v_edges cell_ink cell_ink_box cells")


def max_runs(n):
    """The most separator runs an axis of n positions can hold (rule 11)."""
    return (int(n) + 1) // 2 + 1


def crop_of(box, H, W, margin):
    """Rule 1: (x0, y0, w, h) of a box on an H x W page; w or h may come out below 30, even negative."""
    x1, y1, x2, y2 = (float(v) for v in box)
    xa, ya = max(0, int(math.floor(x1)) - margin), max(0, int(math.floor(y1)) - margin)
    xb, yb = min(W, int(math.ceil(x2)) + margin), min(H, int(math.ceil(y2)) + margin)
    return xa, ya, xb - xa, yb - ya


def _check_pages(pages, device):
    """-> (the pages as contiguous CUDA tensors / NumPy arrays, [(h, w, channels)]); ValueError naming the page before any launch."""
    return _pages.check_pages(pages, MIN_SIDE, MAX_SIDE, device)


def _workspace(crops, n_items=0):
    return lambda: L.lib.rtn_lattice_workspace_bytes(len(crops), _ptr(crops), int(n_items))


def _check_boxes(boxes, n_pages):
    boxes = list(boxes)
    if len(boxes) != n_pages:
        raise ValueError("%d box arrays for %d pages" % (len(boxes), n_pages))
    out = []
    for i, b in enumerate(boxes):
        b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
        b = b.reshape(-1, 4) if b.size == 0 else b
        if b.ndim != 2 or b.shape[1] != 4 or not np.all(np.isfinite(b.astype(np.float64))):
            raise ValueError("page %d: an (n, 4) array of finite x1, y1, x2, y2 expected, got %s" % (i, tuple(b.shape)))
        out.append(b.astype(np.float64))
    return out


def _check_params(flavor, line_scale, line_tol, cover, col_gap, row_gap, margin):
    if flavor not in FLAVORS:
        raise ValueError("flavor: one of %s expected, got %r" % (", ".join(FLAVORS), flavor))
    if not 1 <= int(line_scale) <= 30:
        raise ValueError("line_scale within 1 .. 30 expected, got %r" % (line_scale,))
    if not 0 <= int(cover) <= 100:
        raise ValueError("cover within 0 .. 100 expected, got %r" % (cover,))
    for name, v, lo in (("line_tol", line_tol, 0), ("col_gap", col_gap, 1), ("row_gap", row_gap, 1), ("margin", margin, 0)):
        if not lo <= int(v) <= MAX_SIDE:
            raise ValueError("%s within %d .. %d expected, got %r" % (name, lo, MAX_SIDE, v))


def _buffer(be, bufs, name, n, dtype):
    """A zeroed buffer of n elements; with bufs (a dict) the buffer of an earlier call is taken as it is, whatever it holds."""
    n = max(int(n), 1)
    if bufs is not None and name in bufs and len(bufs[name]) == n:
        return bufs[name]
    buf = be.empty(n, dtype)
    if bufs is not None:
        bufs[name] = buf
    return buf


def separators(profile, mode, param, capacity=None):
    """A profile to its (count, 2) int32 runs through rtn_lattice_separators_host: mode 0 lattice (param = line_tol), mode 1 stream
    (param = the gap).  capacity None gives max_runs(n), which cannot overflow; RtnError (RTN_EINVAL) with the true count where
    the capacity is too small."""
    profile = _i32(profile)
    cap = max_runs(len(profile)) if capacity is None else int(capacity)
    runs, count = np.zeros((max(cap, 1), 2), np.int32), np.zeros(1, np.int32)
    rc = L.lib.rtn_lattice_separators_host(_ptr(profile), len(profile), int(mode), int(param), cap, runs.ctypes.data, count.ctypes.data)
    if rc != 0:
        raise L.RtnError(rc, L.lib.rtn_last_error(None).decode("utf-8", "replace"))
    return runs[:int(count[0])].copy()


def _masks(be, pages, shapes, box_page, crops, line_scale, bufs=None):
    """-> (bw, hm, vm, ink, offsets, total): the packed masks of every crop."""
    hs, ws, ch = _i32([s[0] for s in shapes]), _i32([s[1] for s in shapes]), _i32([s[2] for s in shapes])
    offsets, total = _starts(crops[:, 2].astype(np.int64) * crops[:, 3])
    m = [_buffer(be, bufs, k, total, np.uint8) for k in ("bw", "hm", "vm", "ink")]
    be.call("rtn_lattice_masks", [len(pages), _pointers(be, pages), _ptr(hs), _ptr(ws), _ptr(ch), len(crops), _ptr(box_page), _ptr(crops),
                                  int(line_scale), _ptr(offsets)] + [be.ptr(a) for a in m] + [total], _workspace(crops))
    return m[0], m[1], m[2], m[3], offsets, total


def _profiles(be, crops, offsets, total, hm, vm, ink, bufs=None):
    """-> (profiles, prof_offsets): box j's rowH[h], rowInk[h], colV[w], colInk[w] from prof_offsets[j]."""
    prof_offsets, count = _starts(2 * (crops[:, 2].astype(np.int64) + crops[:, 3]))
    profiles = _buffer(be, bufs, "profiles", count, np.int32)
    be.call("rtn_lattice_profiles", [len(crops), _ptr(crops), _ptr(offsets), be.ptr(hm), be.ptr(vm), be.ptr(ink), total, _ptr(prof_offsets),
                                     be.ptr(profiles), count], _workspace(crops))
    return profiles, prof_offsets


def _runs_table(rows, cols):
    """Per-box run lists -> (R, C, sep_offsets, runs (n, 2))."""
    R, Cn = _i32([len(r) for r in rows]), _i32([len(c) for c in cols])
    sep_offsets, _total = _starts(R.astype(np.int64) + Cn)
    parts = [np.reshape(a, (-1, 2)) for pair in zip(rows, cols) for a in pair]
    runs = _i32(np.concatenate(parts) if parts else np.zeros((0, 2)))
    return R, Cn, sep_offsets, runs.reshape(-1, 2)


def _edges(be, crops, offsets, total, R, Cn, sep_offsets, runs, line_tol, cover, hm, vm, bufs=None, capacity=None):
    """-> (edges, edge_offsets): box j's R (C - 1) horizontal then (R - 1) C vertical flags (uint8) from edge_offsets[j]."""
    per = np.where((R >= 1) & (Cn >= 1), R.astype(np.int64) * (Cn - 1) + (R.astype(np.int64) - 1) * Cn, 0)
    edge_offsets, n_items = _starts(per)
    count = n_items if capacity is None else int(capacity)
    edges = _buffer(be, bufs, "edges", count, np.uint8)
    be.call("rtn_lattice_edges", [len(crops), _ptr(crops), _ptr(offsets), _ptr(R), _ptr(Cn), _ptr(sep_offsets), _ptr(runs), len(runs),
                                  int(line_tol), int(cover), _ptr(edge_offsets), be.ptr(hm), be.ptr(vm), total, be.ptr(edges), count],
            _workspace(crops, n_items))
    return edges, edge_offsets


def _cells(be, crops, offsets, total, R, Cn, sep_offsets, runs, ink, bufs=None, capacity=None):
    """-> (cell_ink, cell_box, cell_offsets): box j's (R - 1) (C - 1) counts and boxes (x, y, w, h in the page) from cell_offsets[j]."""
    per = np.where((R >= 1) & (Cn >= 1), (R.astype(np.int64) - 1) * (Cn - 1), 0)
    cell_offsets, n_items = _starts(per)
    count = n_items if capacity is None else int(capacity)
    cell_ink, cell_box = _buffer(be, bufs, "cell_ink", count, np.int32), _buffer(be, bufs, "cell_box", 4 * count, np.int32)
    be.call("rtn_lattice_cells", [len(crops), _ptr(crops), _ptr(offsets), _ptr(R), _ptr(Cn), _ptr(sep_offsets), _ptr(runs), len(runs),
                                  _ptr(cell_offsets), be.ptr(ink), total, be.ptr(cell_ink), be.ptr(cell_box), count],
            _workspace(crops, n_items))
    return cell_ink, cell_box, cell_offsets


def merge_cells(rows, cols, h_edges, v_edges, cell_ink, cell_ink_box, stream=False):
    """Rule 8 (rule 9 with stream=True: every cell on its own): the list of merged cells.  rows, cols in page coordinates."""
    nr, nc = len(rows) - 1, len(cols) - 1
    if nr < 1 or nc < 1:
        return []
    parent = list(range(nr * nc))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    if not stream:
        for r in range(nr):
            for c in range(nc):
                if c + 1 < nc and not v_edges[r, c + 1]:
                    unite(r * nc + c, r * nc + c + 1)
                if r + 1 < nr and not h_edges[r + 1, c]:
                    unite(r * nc + c, (r + 1) * nc + c)
    groups = collections.OrderedDict()
    for i in range(nr * nc):
        groups.setdefault(find(i), []).append(i)              # roots are the smallest indices: first cells in raster order
    mid_r = [(int(lo) + int(hi)) // 2 for lo, hi in rows]
    mid_c = [(int(lo) + int(hi)) // 2 for lo, hi in cols]
    out = []
    for root in sorted(groups):
        rs, cs = [i // nc for i in groups[root]], [i % nc for i in groups[root]]
        r0, r1, c0, c1 = min(rs), max(rs), min(cs), max(cs)
        ink, xa, ya, xb, yb = 0, None, None, None, None
        for r, c in zip(rs, cs):
            n = int(cell_ink[r, c])
            if n == 0:
                continue
            x, y, w, h = (int(v) for v in cell_ink_box[r, c])
            ink += n
            xa, ya = (x, y) if xa is None else (min(xa, x), min(ya, y))
            xb, yb = (x + w, y + h) if xb is None else (max(xb, x + w), max(yb, y + h))
        ink_box = (0, 0, 0, 0) if ink == 0 else (xa, ya, xb - xa, yb - ya)
        out.append(Cell(r0, c0, r1, c1, mid_c[c0], mid_r[r0], mid_c[c1 + 1], mid_r[r1 + 1], ink, ink_box,
                        len(rs) == (r1 - r0 + 1) * (c1 - c0 + 1)))
    return out


def _none_grid():
    z = np.zeros((0, 2), np.int32)
    return TableGrid("none", z, z.copy(), np.zeros((0, 0), bool), np.zeros((0, 0), bool), np.zeros((0, 0), np.int32),
                     np.zeros((0, 0, 4), np.int32), [])


def _grids(be, pages, shapes, boxes, flavor, line_scale, line_tol, cover, col_gap, row_gap, margin, bufs=None, raw=None):
    """table_cells after the checks.  raw (a dict) receives the host copy of every stage's output, for tests."""
    flat = [(i, crop_of(b, shapes[i][0], shapes[i][1], margin)) for i, bs in enumerate(boxes) for b in bs]
    live = [k for k, (_i, c) in enumerate(flat) if c[2] >= MIN_SIDE and c[3] >= MIN_SIDE]
    grids = [_none_grid() for _ in flat]
    if raw is not None:
        raw.update(crops=[c for _i, c in flat], live=live)
    if live:
        box_page, crops = _i32([flat[k][0] for k in live]), _i32([flat[k][1] for k in live]).reshape(-1, 4)
        bw, hm, vm, ink, offsets, total = _masks(be, pages, shapes, box_page, crops, line_scale, bufs)
        profiles, prof_offsets = _profiles(be, crops, offsets, total, hm, vm, ink, bufs)
        prof = be.host(profiles)                                   # the one round trip before the grids are known
        flavors, rows, cols = [], [], []
        for j, (_x0, _y0, w, h) in enumerate(crops):
            o = int(prof_offsets[j])
            rowH, rowInk, colV, colInk = prof[o:o + h], prof[o + h:o + 2 * h], prof[o + 2 * h:o + 2 * h + w], prof[o + 2 * h + w:o + 2 * h + 2 * w]
            f, r, c = "none", np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32)
            if flavor != "stream":
                lr, lc = separators(rowH, 0, line_tol), separators(colV, 0, line_tol)
                if len(lr) >= 2 and len(lc) >= 2:
                    f, r, c = "lattice", lr, lc
            if f == "none" and flavor != "lattice":
                sr, sc = separators(rowInk, 1, row_gap), separators(colInk, 1, col_gap)
                if len(sr) and len(sc):
                    f, r, c = "stream", sr, sc
            flavors.append(f)
            rows.append(r)
            cols.append(c)
        R, Cn, sep_offsets, runs = _runs_table(rows, cols)
        lattice = np.array([f == "lattice" for f in flavors])
        edges, edge_offsets = _edges(be, crops, offsets, total, _i32(np.where(lattice, R, 0)), _i32(np.where(lattice, Cn, 0)), sep_offsets,
                                     runs, line_tol, cover, hm, vm, bufs)
        cell_ink, cell_box, cell_offsets = _cells(be, crops, offsets, total, R, Cn, sep_offsets, runs, ink, bufs)
        edges_h, ink_h, box_h = be.host(edges), be.host(cell_ink), be.host(cell_box)
        if raw is not None:
            raw.update(offsets=offsets, masks={k: be.host(v) for k, v in (("bw", bw), ("hm", hm), ("vm", vm), ("ink", ink))},
                       profiles=prof, prof_offsets=prof_offsets, flavors=flavors, rows=rows, cols=cols, edges=edges_h,
                       edge_offsets=edge_offsets, cell_ink=ink_h, cell_box=box_h, cell_offsets=cell_offsets)
        for j, k in enumerate(live):
            if flavors[j] == "none":
                continue
            x0, y0 = int(crops[j, 0]), int(crops[j, 1])
            nr, nc = len(rows[j]), len(cols[j])
            if flavors[j] == "lattice":
                e = edges_h[int(edge_offsets[j]):int(edge_offsets[j]) + nr * (nc - 1) + (nr - 1) * nc].astype(bool)
                h_edges, v_edges = e[:nr * (nc - 1)].reshape(nr, nc - 1).copy(), e[nr * (nc - 1):].reshape(nr - 1, nc).copy()
            else:
                h_edges, v_edges = np.zeros((nr, nc - 1), bool), np.zeros((nr - 1, nc), bool)
            o, n = int(cell_offsets[j]), (nr - 1) * (nc - 1)
            ci = np.array(ink_h[o:o + n], np.int32).reshape(nr - 1, nc - 1)
            cb = np.array(box_h[4 * o:4 * (o + n)], np.int32).reshape(nr - 1, nc - 1, 4)
            prow, pcol = _i32(rows[j] + np.int32(y0)), _i32(cols[j] + np.int32(x0))
            grids[k] = TableGrid(flavors[j], prow, pcol, h_edges, v_edges, ci, cb,
                                 merge_cells(prow, pcol, h_edges, v_edges, ci, cb, stream=flavors[j] == "stream"))
    out, k = [], 0
    for bs in boxes:
        out.append(grids[k:k + len(bs)])
        k += len(bs)
    return out


def table_cells(pages, boxes, flavor="auto", line_scale=15, line_tol=2, cover=50, col_gap=12, row_gap=4, margin=10, device=True):
    """The grid of every box of every page, by the rules of this module's docstring.  pages: uint8 (H,W,3) B,G,R or (H,W) gray
    pages of mixed sizes with sides 30 .. 16384, as NumPy arrays or CUDA tensors (never written); boxes: per page an (n, 4) array
    x1, y1, x2, y2 in page pixels, as detect_files reports them; n may be 0, boxes may overlap or reach outside the page.
    Returns, per page, the list of one TableGrid per box: flavor ("lattice", "stream" or "none"), rows (R, 2) and cols (C, 2)
    (int32 separator runs lo, hi in page coordinates), h_edges (R, C - 1) and v_edges (R - 1, C) (bool), cell_ink (R - 1, C - 1)
    (int32), cell_ink_box (R - 1, C - 1, 4) (int32 x, y, w, h) and cells, the list of merged Cell(r0, c0, r1, c1, x1, y1, x2, y2,
    ink, ink_box, rect).  device=False runs the CPU twins (no GPU needed), which give the same bytes.  ValueError naming the page,
    before anything is launched, for a page that is not uint8 (H,W,3) / (H,W) or has a side outside 30 .. 16384."""
    _check_params(flavor, line_scale, line_tol, cover, col_gap, row_gap, margin)
    pages, shapes = _check_pages(pages, device)
    boxes = _check_boxes(boxes, len(pages))
    be = _Device(pages[0].device) if device and pages else _Twins()
    return _grids(be, pages, shapes, boxes, flavor, int(line_scale), int(line_tol), int(cover), int(col_gap), int(row_gap), int(margin))


def csv_text(grid):
    """The CSV of one TableGrid: CSV_HEADER, then one line per merged cell."""
    lines = [CSV_HEADER]
    for c in grid.cells:
        lines.append(",".join(str(int(v)) for v in (c.r0, c.c0, c.r1 - c.r0 + 1, c.c1 - c.c0 + 1, c.x1, c.y1, c.x2, c.y2, c.ink) + tuple(c.ink_box)))
    return "\n".join(lines) + "\n"


def write_csvs(grids, names, out_dir):
    """<stem>_table<k>_cells.csv under out_dir (created) for box k of every page; names: one file name per page, whose extension is
    dropped.  Returns the paths written."""
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for name, page_grids in zip(names, grids):
        stem = os.path.splitext(os.path.basename(str(name)))[0]
        for k, g in enumerate(page_grids):
            paths.append(os.path.join(out_dir, "{}_table{}_cells.csv".format(stem, k)))
            with open(paths[-1], "w", newline="") as f:
                f.write(csv_text(g))
    return paths


def outline_cells(pages, grids):
    """New pages (CUDA tensors) with the outer box of every merged cell outlined by rtn_cca_paint mode 1 (draw_box's bands, (0, 255, 0),
    255 on a gray page); coordinates left of or above the page are drawn from 0."""
    pages, shapes = _check_pages(pages, True)
    drawn = [p.clone() for p in pages]
    boxes = [np.array([[max(c.x1, 0), max(c.y1, 0), c.x2 - max(c.x1, 0), c.y2 - max(c.y1, 0)] for g in page_grids for c in g.cells],
                      np.int32).reshape(-1, 4) for page_grids in grids]
    if drawn:
        components._paint(_Device(drawn[0].device), drawn, shapes, boxes, components.OUTLINE)
    return drawn


def cells_files(paths, boxes, result_dir, outline=False, png="host", **kw):
    """table_cells over image files read by read_images_bgr: writes <stem>_table<k>_cells.csv under result_dir for box k of every
    file (the header row,col,rowspan,colspan,x1,y1,x2,y2,ink,ink_x,ink_y,ink_w,ink_h, one line per merged cell) and, with
    outline=True, <stem>_cells.<ext> with the cells' outer boxes drawn, through write_images_bgr(..., png=png).  kw: table_cells'
    keywords.  Returns table_cells' grids."""
    from .page_io import read_images_bgr, write_images_bgr
    paths = [str(p) for p in paths]
    pages = read_images_bgr(paths)
    grids = table_cells(pages, boxes, **kw)
    write_csvs(grids, paths, result_dir)
    if outline:
        names = [os.path.splitext(os.path.basename(p)) for p in paths]
        write_images_bgr([os.path.join(result_dir, "{}_cells{}".format(stem, ext)) for stem, ext in names], outline_cells(pages, grids), png=png)
    return grids
