"""The NumPy oracle of table structure (tests/lattice_ref.py) against what the construction of every synthetic case fixes, without a
GPU and without the library's results: this is what keeps the tests that compare the twins and the kernels with the oracle
honest."""
import numpy as np
import pytest

import lattice_cases as K
import lattice_ref as R

LATTICE = [nm for nm, c in K.cases().items() if c["expect"] is not None]


def first(name, **kw):
    return K.oracle(name, **kw)[0]


@pytest.mark.parametrize("name", LATTICE + ["long"])
def test_separators_are_the_drawn_rules(name):
    c = K.long_case() if name == "long" else K.cases()[name]
    g, e = first(name), c["expect"]
    assert g["flavor"] == "lattice"
    assert len(g["rows"]) == e["R"] and len(g["cols"]) == e["C"]
    for runs, rules in ((g["rows"], e["rows"]), (g["cols"], e["cols"])):
        for top, thick in rules:                                                # every rule's rows lie in one run
            assert any(lo <= top and top + thick - 1 <= hi for lo, hi in runs), (name, top)
        if len(runs) == len(rules):                                             # nothing merged: the runs are the rules, exactly
            assert [tuple(r) for r in runs] == [(top, top + thick - 1) for top, thick in rules], name
    assert g["h_edges"].shape == (e["R"], e["C"] - 1) and g["v_edges"].shape == (e["R"] - 1, e["C"])
    assert g["cell_ink"].shape == (e["R"] - 1, e["C"] - 1) and g["cell_ink_box"].shape == (e["R"] - 1, e["C"] - 1, 4)


@pytest.mark.parametrize("name", [nm for nm in LATTICE if nm not in ("table_span", "table_ell")] + ["long"])
def test_every_edge_of_a_full_grid_is_present(name):
    g = first(name)
    assert g["h_edges"].all() and g["v_edges"].all()
    assert len(g["cells"]) == g["cell_ink"].size and all(c[10] and (c[0], c[1]) == (c[2], c[3]) for c in g["cells"])


def test_the_table_cells_hold_their_blobs():
    g = first("table")
    assert np.array_equal(g["cell_ink"], np.full((4, 3), 80))                   # four blobs of 4 x 5
    for r, y in enumerate(K.TABLE_YS[:-1]):
        for c, x in enumerate(K.TABLE_XS[:-1]):
            assert tuple(g["cell_ink_box"][r, c]) == (x + 5, y + 5, 22, 5)


def test_the_margin_brings_the_frame_in():
    c = K.cases()["table"]
    assert first("table")["crop"] == (8, 13, 185, 116)
    g = R.grid(c["page"], c["boxes"][0], margin=0)
    assert g["flavor"] == "lattice" and len(g["rows"]) == 3 and len(g["cols"]) == 2        # the frame stays outside


MIDS_Y, MIDS_X = (20, 45, 70, 95, 120), (15, 70, 130, 184)


def single(r, c, ink=80):
    x, y = K.TABLE_XS[c] + 5, K.TABLE_YS[r] + 5
    return (r, c, r, c, MIDS_X[c], MIDS_Y[r], MIDS_X[c + 1], MIDS_Y[r + 1], ink, (x, y, 22, 5), True)


def test_the_erased_segment_gives_one_cell_of_colspan_two():
    g = first("table_span")
    v = np.ones((4, 4), bool)
    v[1, 1] = False
    assert g["h_edges"].all() and np.array_equal(g["v_edges"], v)               # the erased edge, and only it, is absent
    want = [single(0, 0), single(0, 1), single(0, 2),
            (1, 0, 1, 1, 15, 45, 130, 70, 160, (20, 50, 77, 5), True), single(1, 2),
            single(2, 0), single(2, 1), single(2, 2),
            single(3, 0), single(3, 1), single(3, 2)]
    assert g["cells"] == want


def test_the_ell_shaped_erasure_gives_a_cell_that_is_no_rectangle():
    g = first("table_ell")
    v, h = np.ones((4, 4), bool), np.ones((5, 3), bool)
    v[1, 1] = False
    h[2, 1] = False
    assert np.array_equal(g["h_edges"], h) and np.array_equal(g["v_edges"], v)
    want = [single(0, 0), single(0, 1), single(0, 2),
            (1, 0, 2, 1, 15, 45, 130, 95, 240, (20, 50, 77, 30), False), single(1, 2),
            single(2, 0), single(2, 2),
            single(3, 0), single(3, 1), single(3, 2)]
    assert g["cells"] == want


def test_the_smallest_crop():
    g = first("crop_30x30")
    assert g["crop"] == (0, 0, 30, 30) and g["cell_ink"].tolist() == [[4]] and tuple(g["cell_ink_box"][0, 0]) == (7, 9, 10, 1)


def test_near_rules_merge_at_two_zero_rows_and_not_at_three():
    g = first("near_rules")
    assert [tuple(r) for r in g["rows"]] == [(20, 21), (40, 45), (80, 81), (85, 86), (120, 121)]
    c = K.cases()["near_rules"]
    assert len(R.grid(c["page"], c["boxes"][0], line_tol=3)["rows"]) == 4 and len(R.grid(c["page"], c["boxes"][0], line_tol=1)["rows"]) == 6
    assert g["cell_ink"][2].tolist() == [0, 0] and g["cell_ink_box"][2].tolist() == [[0, 0, 0, 0]] * 2       # three rows, no ink


def test_a_box_outside_the_page_is_cut_to_it():
    assert first("box_outside")["crop"] == (0, 0, 200, 146)


def test_overlapping_boxes_and_a_page_without_one():
    assert K.oracle("gray_no_box") == []
    a, b = K.oracle("overlapping")
    assert a["flavor"] == b["flavor"] == "lattice" and b["crop"] == (50, 30, 143, 99)
    assert [tuple(r) for r in b["rows"]] == [(45, 46), (70, 71), (95, 96), (120, 121)]
    assert [tuple(r) for r in b["cols"]] == [(70, 71), (130, 131), (184, 185)]


def test_the_borderless_table_splits_at_a_gap_of_twelve_only():
    g = first("borderless")
    assert g["flavor"] == "stream"
    assert [tuple(r) for r in g["cols"]] == [(0, 19), (111, 122), (163, 199)]
    assert [tuple(r) for r in g["rows"]] == [(0, 19), (25, 39), (45, 59), (65, 79), (85, 119)]
    assert not g["h_edges"].any() and not g["v_edges"].any() and g["h_edges"].shape == (5, 2) and g["v_edges"].shape == (4, 3)
    assert g["cell_ink"].tolist() == [[14 * 20, 7 * 20]] * 4
    assert [c[:8] for c in g["cells"][:2]] == [(0, 0, 0, 0, 9, 9, 116, 32), (0, 1, 0, 1, 116, 9, 181, 32)] and len(g["cells"]) == 8
    c = K.cases()["borderless"]
    assert len(R.grid(c["page"], c["boxes"][0], col_gap=11)["cols"]) == 4 and len(R.grid(c["page"], c["boxes"][0], col_gap=13)["cols"]) == 2
    # ink from the crop's first column to its last: the leading and the trailing run are empty
    tight = R.grid(c["page"], (20, 0, 163, 120), margin=0)
    assert tuple(tight["cols"][0]) == (20, 19) and tuple(tight["cols"][-1]) == (163, 162) and len(tight["cols"]) == 3
    assert tight["cells"][0][4:6] == (19, 9) and tight["cells"][1][6] == 162 and tight["cell_ink"].tolist() == [[280, 140]] * 4


def test_a_blank_crop_and_a_small_one_have_no_grid():
    assert first("blank")["flavor"] == "none" and first("blank")["cells"] == []
    c = K.cases()["table"]
    small = R.grid(c["page"], (50, 50, 59, 90), margin=10)
    assert small["flavor"] == "none" and small["crop"] == (40, 40, 29, 60) and "masks" not in small


def test_forced_flavours():
    assert first("table", flavor="stream")["flavor"] == "stream"
    assert first("borderless", flavor="lattice")["flavor"] == "none"
    assert first("blank", flavor="stream")["flavor"] == "none"


def test_the_golden_page_gives_consistent_grids():
    for g in K.oracle("golden"):
        assert g["flavor"] in ("lattice", "stream")
        nr, nc = len(g["rows"]), len(g["cols"])
        assert g["h_edges"].shape == (nr, nc - 1) and g["v_edges"].shape == (nr - 1, nc) and g["cell_ink"].shape == (nr - 1, nc - 1)
        assert sum(c[8] for c in g["cells"]) == int(g["cell_ink"].sum())
