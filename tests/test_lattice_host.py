"""The CPU twins of table structure (rtn_lattice_*_host, csrc/rtn_lattice.h) against the NumPy oracle (tests/lattice_ref.py), bit for
bit and without a GPU: the masks, the profiles, the separators, the edges, the cell tables and the merged cells of every case;
the capacity errors, the argument checks and the flavour forced to each value."""
import numpy as np
import pytest

import lattice_cases as K
import lattice_ref as R

S = K.S
L = S.L
TW = S._pages.Twins()
KW = dict(flavor="auto", line_scale=15, line_tol=2, cover=50, col_gap=12, row_gap=4, margin=10)


def run(case, **kw):
    """One case through the twins -> (grids of its page, raw stages)."""
    pages, shapes = S._pages.check_pages([case["page"]], S.MIN_SIDE, S.MAX_SIDE, False)
    raw = {}
    grids = S._grids(TW, pages, shapes, S._check_boxes([case["boxes"]], 1), raw=raw, **dict(KW, **kw))
    return grids[0], raw


def named(name):
    return K.long_case() if name == "long" else K.golden_case() if name == "golden" else K.cases()[name]


@pytest.mark.parametrize("name", list(K.cases()) + ["long", "golden"])
def test_every_stage_equals_the_oracle(name):
    case = named(name)
    grids, raw = run(case)
    want = K.oracle(name)
    assert len(grids) == len(want) and raw["crops"] == [w["crop"] for w in want]
    for k, (g, w) in enumerate(zip(grids, want)):
        assert K.same_grid(g, w) is None, (name, k, K.same_grid(g, w))
    for j, k in enumerate(raw["live"]):
        w = want[k]
        _x0, _y0, cw, ch = w["crop"]
        o = int(raw["offsets"][j])
        for key in ("bw", "hm", "vm", "ink"):
            assert np.array_equal(raw["masks"][key][o:o + cw * ch].reshape(ch, cw), w["masks"][key]), (name, k, key)
        p = int(raw["prof_offsets"][j])
        got = raw["profiles"][p:p + 2 * (cw + ch)]
        assert got.dtype == np.int32
        for key, a, b in (("rowH", 0, ch), ("rowInk", ch, 2 * ch), ("colV", 2 * ch, 2 * ch + cw), ("colInk", 2 * ch + cw, 2 * ch + 2 * cw)):
            assert np.array_equal(got[a:b], w["profiles"][key]), (name, k, key)
    assert np.array_equal(case["page"], named(name)["page"])


def test_the_mixed_batch_in_one_call_equals_the_cases_one_by_one():
    names = list(K.cases())
    pages = [K.cases()[nm]["page"] for nm in names]
    assert any(p.ndim == 2 for p in pages) and any(len(K.cases()[nm]["boxes"]) == 0 for nm in names)
    got = S.table_cells(pages, [K.cases()[nm]["boxes"] for nm in names], device=False)
    for nm, grids in zip(names, got):
        assert len(grids) == len(K.oracle(nm))
        for g, w in zip(grids, K.oracle(nm)):
            assert K.same_grid(g, w) is None, (nm, K.same_grid(g, w))


@pytest.mark.parametrize("flavor", ["lattice", "stream"])
def test_forced_flavours_equal_the_oracle(flavor):
    for nm in ("table", "table_ell", "borderless", "blank", "near_rules"):
        c = K.cases()[nm]
        got = S.table_cells([c["page"]], [c["boxes"]], flavor=flavor, device=False)[0]
        for g, w in zip(got, K.oracle(nm, flavor)):
            assert K.same_grid(g, w) is None, (nm, flavor, K.same_grid(g, w))


@pytest.mark.parametrize("kw", [dict(line_tol=0), dict(line_tol=3), dict(cover=100), dict(cover=0), dict(col_gap=11, flavor="stream"),
                                dict(row_gap=16, flavor="stream"), dict(margin=0), dict(line_scale=30), dict(line_scale=6)])
def test_other_parameters_equal_the_oracle(kw):
    for nm in ("table_ell", "near_rules", "borderless"):
        c = K.cases()[nm]
        got = S.table_cells([c["page"]], [c["boxes"]], device=False, **kw)[0]
        for g, b in zip(got, c["boxes"]):
            w = R.grid(c["page"], b, **kw)
            assert K.same_grid(g, w) is None, (nm, kw, K.same_grid(g, w))


def test_separators_report_the_true_count_when_the_room_is_short():
    prof = np.zeros(40, np.int32)
    prof[::2] = 1                                                               # 20 runs at line_tol = 0; stream: 21 gaps of 1 and two empty ends
    assert len(S.separators(prof, 0, 0)) == 20 and S.max_runs(40) == 21
    assert len(S.separators(prof[:39], 1, 1)) == 21 == S.max_runs(39)           # ink on both ends: the most an axis can hold
    runs, count = np.full((5, 2), -7, np.int32), np.zeros(1, np.int32)
    rc = L.lib.rtn_lattice_separators_host(prof.ctypes.data, 40, 0, 0, 5, runs.ctypes.data, count.ctypes.data)
    assert rc == -1 and int(count[0]) == 20 and runs.tolist() == [[0, 0], [2, 2], [4, 4], [6, 6], [8, 8]]
    assert "20 runs" in L.lib.rtn_last_error(None).decode()
    with pytest.raises(L.RtnError):
        S.separators(prof, 0, 0, capacity=19)
    for bad in ((prof.ctypes.data, 0, 0, 0), (prof.ctypes.data, 40, 2, 0), (prof.ctypes.data, 40, 0, -1), (None, 40, 0, 0)):
        assert L.lib.rtn_lattice_separators_host(bad[0], bad[1], bad[2], bad[3], 5, runs.ctypes.data, count.ctypes.data) == -1


def stage_args():
    c = K.cases()["table"]
    pages, shapes = S._pages.check_pages([c["page"]], S.MIN_SIDE, S.MAX_SIDE, False)
    crops, box_page = np.array([[8, 13, 185, 116]], np.int32), np.zeros(1, np.int32)
    bw, hm, vm, ink, offsets, total = S._masks(TW, pages, shapes, box_page, crops, 15)
    g = K.oracle("table")[0]
    rows, cols = g["rows"] - np.int32(13), g["cols"] - np.int32(8)
    return crops, offsets, total, hm, vm, ink, S._runs_table([rows], [cols])


def test_edge_and_cell_tables_report_the_true_count_when_the_room_is_short():
    crops, offsets, total, hm, vm, ink, (Rn, Cn, sep, runs) = stage_args()
    with pytest.raises(L.RtnError, match="31 edges, room for 30"):
        S._edges(TW, crops, offsets, total, Rn, Cn, sep, runs, 2, 50, hm, vm, capacity=30)
    with pytest.raises(L.RtnError, match="12 cells, room for 11"):
        S._cells(TW, crops, offsets, total, Rn, Cn, sep, runs, ink, capacity=11)
    edges, _off = S._edges(TW, crops, offsets, total, Rn, Cn, sep, runs, 2, 50, hm, vm, capacity=31)
    assert edges.tolist() == [1] * 31


def test_argument_checks():
    crops, offsets, total, hm, vm, ink, (Rn, Cn, sep, runs) = stage_args()
    c = K.cases()["table"]
    pages, shapes = S._pages.check_pages([c["page"]], S.MIN_SIDE, S.MAX_SIDE, False)
    page0 = np.zeros(1, np.int32)
    for bad_crop, why in (([8, 13, 29, 116], "side outside"), ([-1, 13, 185, 116], "negative origin"), ([8, 13, 193, 116], "outside its page")):
        with pytest.raises(L.RtnError, match=why):
            S._masks(TW, pages, shapes, page0, np.array([bad_crop], np.int32), 15)
    with pytest.raises(L.RtnError, match="line_scale"):
        S._masks(TW, pages, shapes, page0, crops, 31)
    with pytest.raises(L.RtnError, match="page outside the batch"):
        S._masks(TW, pages, shapes, np.ones(1, np.int32), crops, 15)
    for bad in ([[5, 4], [9, 9], [3, 3]], [[0, 3], [2, 9]], [[0, 3], [9, 116]], [[0, 3], [7, 6], [9, 9]]):      # unordered, touching the last, outside, empty inside
        r = np.array(bad, np.int32)
        with pytest.raises(L.RtnError, match="separator run"):
            S._cells(TW, crops, offsets, total, *S._runs_table([r], [r]), ink)
    with pytest.raises(L.RtnError, match="cover"):
        S._edges(TW, crops, offsets, total, Rn, Cn, sep, runs, 2, 101, hm, vm)
    with pytest.raises(L.RtnError, match="mask ends past"):
        S._profiles(TW, crops, offsets, total - 1, hm, vm, ink)


def test_table_cells_checks_its_arguments_before_anything_runs():
    page = K.cases()["table"]["page"]
    for bad, why in ((np.zeros((29, 40), np.uint8), "page 1: sides"), (np.zeros((40, 16385), np.uint8), "page 1: sides"),
                     (np.zeros((40, 40, 4), np.uint8), "page 1: a uint8"), (np.zeros((40, 40), np.float32), "page 1: a uint8")):
        with pytest.raises(ValueError, match=why):
            S.table_cells([page, bad], [np.zeros((0, 4)), np.zeros((0, 4))], device=False)
    for kw in (dict(flavor="hough"), dict(line_scale=0), dict(line_scale=31), dict(cover=101), dict(line_tol=-1), dict(col_gap=0), dict(margin=-1)):
        with pytest.raises(ValueError):
            S.table_cells([page], [K.TABLE_BOX], device=False, **kw)
    with pytest.raises(ValueError, match="1 box arrays for 2 pages"):
        S.table_cells([page, page], [np.zeros((0, 4))], device=False)
    with pytest.raises(ValueError, match="page 0: an"):
        S.table_cells([page], [np.zeros((2, 3))], device=False)
    assert S.table_cells([], [], device=False) == [] and S.table_cells([page], [np.zeros((0, 4))], device=False) == [[]]


def test_csv_text_equals_the_oracle():
    for nm in ("table_ell", "borderless", "blank"):
        c = K.cases()[nm]
        g = S.table_cells([c["page"]], [c["boxes"]], device=False)[0][0]
        assert S.csv_text(g) == R.csv_text(K.oracle(nm)[0])
    assert S.csv_text(S._none_grid()) == S.CSV_HEADER + "\n"
    text = R.csv_text(K.oracle("table_ell")[0]).splitlines()
    assert text[0] == "row,col,rowspan,colspan,x1,y1,x2,y2,ink,ink_x,ink_y,ink_w,ink_h" and text[4] == "1,0,2,2,15,45,130,95,240,20,50,77,30"
