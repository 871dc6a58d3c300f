"""The workspace contract of the 16 page-analysis device entries (csrc/rtn_cca.hip, rtn_lattice.hip, rtn_header.hip, rtn_effect.hip,
rtn_resize_u8.hip, rtn_skew.hip, rtn_render.hip), each on the smallest batch it accepts.  No case launches a kernel:
  (a) a valid workspace pointer plus 16 bytes: RTN_EINVAL, "aligned" in rtn_last_error;
  (b) an aligned pointer with workspace_bytes = 0: RTN_ENOMEM, "workspace" in the message;
  (c) after (a) and after (b) every output still holds the pattern it was filled with;
  (d) n = 0 with a null workspace: RTN_OK;
  (e) a plan error (a null table) together with a misaligned workspace reports the plan error: RTN_EINVAL without "aligned".
The file was written against the entries as they stood before the table stager of csrc/rtn_page_launch.h existed and passed there
unchanged: it pins that behaviour."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
EINVAL, ENOMEM = -1, -3


class Case:
    """name: the entry; args: its arguments between the handle and the workspace; outs: the output buffers; wsb: the workspace
    bytes its size function asks for; zero: the arguments of the empty batch; bad: the index in args of a table to withhold."""

    def __init__(self, name, args, outs, wsb, zero, bad, keep):
        self.name, self.args, self.outs, self.wsb, self.zero, self.bad, self.keep = name, args, outs, wsb, zero, bad, keep


class Alloc:
    """Device buffers of PATTERN; NumPy arrays are kept alive by the case that holds them."""

    def buf(self, nbytes):
        return torch.full((int(nbytes),), PATTERN, dtype=torch.uint8, device="cuda")

    def upload(self, a):
        return torch.as_tensor(np.array(a)).cuda()

    def ptr(self, t):
        return t.data_ptr()


def i32(*v):
    return np.ascontiguousarray(v, np.int32).reshape(-1)


def i64(*v):
    return np.ascontiguousarray(v, np.int64).reshape(-1)


def one(p):
    return (C.c_void_p * 1)(p)


def build_cases(lib, A):
    """-> {entry name: Case}"""
    cases = {}

    def add(name, args, outs, wsb, zero, bad, *keep):
        assert wsb > 0 and wsb % 256 == 0, (name, wsb)
        cases[name] = Case(name, args, outs, int(wsb), zero, bad, keep)

    p = lambda a: a.ctypes.data
    # ---- scan analysis and table structure: one 30 x 30 gray page, one 30 x 30 box ---------------------------------------------------
    rng = np.random.RandomState(5)
    page = A.upload(rng.randint(0, 256, (30, 30)).astype(np.uint8))
    hs, ws, ch, off = i32(30), i32(30), i32(1), i64(0)
    px = 900
    cca_ws = lambda n_boxes: lib.rtn_cca_workspace_bytes(1, p(hs), p(ws), n_boxes)
    hor, ver = A.buf(px), A.buf(px)
    add("rtn_cca_lines_mask", [1, one(A.ptr(page)), p(hs), p(ws), p(ch), p(off), A.ptr(hor), A.ptr(ver), px], [hor, ver], cca_ws(0),
        [0, None, None, None, None, None, None, None, 0], 2, page)
    closed = A.buf(px)
    add("rtn_cca_text_mask", [1, one(A.ptr(page)), p(hs), p(ws), p(ch), p(off), A.ptr(closed), px], [closed], cca_ws(0),
        [0, None, None, None, None, None, None, 0], 2, page)
    cap, first = i32(225), i64(0)
    counts, boxes = A.buf(4), A.buf(16 * 225)
    add("rtn_cca_label", [1, one(A.ptr(page)), p(hs), p(ws), 1, p(cap), p(first), A.ptr(counts), A.ptr(boxes), 16 * 225], [counts, boxes],
        cca_ws(0), [0, None, None, None, 1, None, None, None, None, 0], 2, page)
    painted = A.buf(px)
    box_page, rect = i32(0), i32(0, 0, 30, 30)
    add("rtn_cca_paint", [1, one(A.ptr(painted)), p(hs), p(ws), p(ch), 1, p(box_page), p(rect), 0], [painted], cca_ws(1),
        [0, None, None, None, None, 0, None, None, 0], 2)
    crops = i32(0, 0, 30, 30)
    lat_ws = lambda items: lib.rtn_lattice_workspace_bytes(1, p(crops), items)
    masks = [A.buf(px) for _ in range(4)]
    add("rtn_lattice_masks", [1, one(A.ptr(page)), p(hs), p(ws), p(ch), 1, p(box_page), p(crops), 15, p(off)] + [A.ptr(m) for m in masks] + [px],
        masks, lat_ws(0), [0, None, None, None, None, 0, None, None, 15, None, None, None, None, None, 0], 2, page)
    hm, vm, ink = (A.upload(np.zeros(px, np.uint8)) for _ in range(3))
    prof_off, profiles = i64(0), A.buf(4 * 120)
    add("rtn_lattice_profiles", [1, p(crops), p(off), A.ptr(hm), A.ptr(vm), A.ptr(ink), px, p(prof_off), A.ptr(profiles), 120], [profiles],
        lat_ws(0), [0, None, None, None, None, None, 0, None, None, 0], 1, hm, vm, ink)
    R, Cn, sep_off, runs = i32(2), i32(2), i64(0), i32(0, 0, 29, 29, 0, 0, 29, 29)
    edge_off, edges = i64(0), A.buf(4)
    add("rtn_lattice_edges", [1, p(crops), p(off), p(R), p(Cn), p(sep_off), p(runs), 4, 2, 50, p(edge_off), A.ptr(hm), A.ptr(vm), px,
                              A.ptr(edges), 4], [edges], lat_ws(4),
        [0, None, None, None, None, None, None, 0, 2, 50, None, None, None, 0, None, 0], 1, hm, vm)
    cell_off, cell_ink, cell_box = i64(0), A.buf(4), A.buf(16)
    add("rtn_lattice_cells", [1, p(crops), p(off), p(R), p(Cn), p(sep_off), p(runs), 4, p(cell_off), A.ptr(ink), px, A.ptr(cell_ink),
                              A.ptr(cell_box), 1], [cell_ink, cell_box], lat_ws(1),
        [0, None, None, None, None, None, None, 0, None, None, 0, None, None, 0], 1, ink)
    # ---- header detection: one 2 x 500 crop, so dh = 2 ------------------------------------------------------------------------------
    crop = A.upload(rng.randint(0, 256, (2, 500, 3)).astype(np.uint8))
    ch_, cw_, dst = i32(2), i32(500), i32(2)
    pts = 1000
    hdr_ws = lambda n_patches: lib.rtn_header_workspace_bytes(1, n_patches)
    hsv = A.buf(3 * pts)
    add("rtn_header_sample", [1, one(A.ptr(crop)), p(ch_), p(cw_), p(dst), p(off), A.ptr(hsv), 3 * pts], [hsv], hdr_ws(0),
        [0, None, None, None, None, None, None, 0], 4, crop)
    hsv_in = A.upload(np.zeros(3 * pts, np.uint8))
    labels_in = A.upload(np.zeros(9 * pts, np.uint8))
    centres, kcounts, passes, dist, labels = A.buf(4 * 243), A.buf(4 * 81), A.buf(4 * 9), A.buf(8 * 9), A.buf(9 * pts)
    add("rtn_header_cluster", [1, p(dst), p(off), A.ptr(hsv_in), 3 * pts, 2, A.ptr(centres), A.ptr(kcounts), A.ptr(passes), A.ptr(dist),
                               A.ptr(labels), 9 * pts], [centres, kcounts, passes, dist, labels], hdr_ws(0),
        [0, None, None, None, 0, 2, None, None, None, None, None, 0], 1, hsv_in)
    ks, hist = i32(1), A.buf(4 * 9 * 3 * 256)
    add("rtn_header_stats", [1, p(dst), p(off), p(ks), A.ptr(hsv_in), 3 * pts, A.ptr(labels_in), 9 * pts, A.ptr(hist)], [hist], hdr_ws(0),
        [0, None, None, None, None, 0, None, 0, None], 1, hsv_in, labels_in)
    patch_crop, low, high = i32(0), np.zeros(3, np.uint8), np.full(3, 255, np.uint8)
    patch = A.buf(3 * pts)
    add("rtn_header_patches", [1, p(dst), p(off), A.ptr(hsv_in), 3 * pts, 1, p(patch_crop), p(low), p(high), p(off), A.ptr(patch), 3 * pts],
        [patch], hdr_ws(1), [0, None, None, None, 0, 0, None, None, None, None, None, 0], 1, hsv_in, low, high)
    # ---- effect, resize, skew: one 1 x 1 page ---------------------------------------------------------------------------------------
    h1, w1, c1 = i32(1), i32(1), i32(1)
    bgr = A.upload(np.array([[[10, 20, 30]]], np.uint8))
    par, fl = np.array([1.1, 0.0, 0.0, 0.0], np.float64), np.zeros(1, np.uint32)
    shaded = A.buf(3)
    add("rtn_visual_effect_u8", [1, one(A.ptr(bgr)), p(h1), p(w1), p(par), p(fl), one(A.ptr(shaded))], [shaded],
        lib.rtn_visual_effect_workspace_bytes(1, p(h1), p(w1)), [0, None, None, None, None, None, None], 2, bgr, par, fl)
    gray = A.upload(np.array([[77]], np.uint8))
    inv = np.ones(1, np.float64)
    resized = A.buf(1)
    add("rtn_resize_u8", [1, one(A.ptr(gray)), p(h1), p(w1), p(c1), p(h1), p(w1), p(inv), p(inv), one(A.ptr(resized))], [resized],
        lib.rtn_resize_u8_workspace_bytes(1), [0, None, None, None, None, None, None, None, None, None], 2, gray, inv)
    shear = i32(0)
    thr, sink, best, scores = A.buf(4), A.buf(8), A.buf(4), A.buf(8)
    add("rtn_skew_estimate", [1, one(A.ptr(gray)), p(h1), p(w1), p(c1), 0, 32, 1, p(shear), A.ptr(thr), A.ptr(sink), A.ptr(best), A.ptr(scores)],
        [thr, sink, best, scores], lib.rtn_skew_workspace_bytes(1, p(h1), p(w1), 32, 1),
        [0, None, None, None, None, 0, 32, 1, p(shear), None, None, None, None], 2, gray, shear)
    # ---- render: one 8 x 8 page, no detection kept on it would give no output: one detection with an empty rectangle gives the page alone
    U = importlib.import_module("retinanet-for-table-detection_amd.model.utils")
    plan = U._render_plan([(8, 8)], [[(np.array([2, 2, 2, 6]), 0.9, 0)]])
    assert len(plan["images"]) == 1
    rpage = A.upload(rng.randint(0, 256, (8, 8, 3)).astype(np.uint8))
    rmasks = A.upload(plan["masks"]) if plan["masks"].size else None
    rout = A.buf(plan["out_bytes"])
    empty = U._render_plan([], [])
    add("rtn_render_pages", U._render_args(plan, [A.ptr(rpage)], A.ptr(rmasks) if rmasks is not None else None, A.ptr(rout)), [rout],
        lib.rtn_render_workspace_bytes(1, len(plan["boxes"]), 1), U._render_args(empty, [], None, None), 2, rpage, rmasks, plan, empty)
    cases.update(_keep=(hs, ws, ch, off, cap, first, box_page, rect, crops, prof_off, R, Cn, sep_off, runs, edge_off, cell_off, ch_, cw_, dst,
                        ks, patch_crop, h1, w1, c1))
    return cases


ENTRIES = ["rtn_cca_lines_mask", "rtn_cca_text_mask", "rtn_cca_label", "rtn_cca_paint", "rtn_lattice_masks", "rtn_lattice_profiles",
           "rtn_lattice_edges", "rtn_lattice_cells", "rtn_header_sample", "rtn_header_cluster", "rtn_header_stats", "rtn_header_patches",
           "rtn_visual_effect_u8", "rtn_resize_u8", "rtn_skew_estimate", "rtn_render_pages"]


@pytest.fixture(scope="module")
def cases(pkg):
    return build_cases(pkg.lib, Alloc())


def untouched(case):
    torch.cuda.synchronize()
    return all(bool((o == PATTERN).all()) for o in case.outs)


@pytest.mark.parametrize("name", ENTRIES)
def test_workspace_contract(pkg, handle, cases, name):
    case = cases[name]
    f = getattr(pkg.lib, name)
    err = lambda: pkg.lib.rtn_last_error(handle.raw)
    ws = torch.empty(case.wsb + 256, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    assert f(handle.raw, *case.args, ws.data_ptr() + 16, case.wsb) == EINVAL and b"aligned" in err(), err()             # (a)
    assert untouched(case)                                                                                              # (c)
    assert f(handle.raw, *case.args, ws.data_ptr(), 0) == ENOMEM and b"workspace" in err(), err()                       # (b)
    assert untouched(case)                                                                                              # (c)
    assert f(handle.raw, *case.zero, None, 0) == 0, err()                                                               # (d)
    bad = list(case.args)
    bad[case.bad] = None
    assert f(handle.raw, *bad, ws.data_ptr() + 16, case.wsb) == EINVAL and b"aligned" not in err(), err()               # (e)
    assert untouched(case)
