"""The CPU twins of scan analysis (rtn_cca_*_host, csrc/rtn_cca.h) against the NumPy / scipy oracle (tests/cca_ref.py), bit for bit
and without a GPU: every intermediate mask, every box list, every output page; the capacity overflow; the argument checks."""
import ctypes as C

import numpy as np
import pytest

import cca_cases as K
import cca_ref as R

CCA = K.CCA
L = CCA.L
TW = CCA._pages.Twins()


def batch():
    names = list(K.pages())
    pages, shapes = CCA._pages.check_pages([K.pages()[nm] for nm in names], CCA.MIN_SIDE, CCA.MAX_SIDE, False, upload=False)
    return names, pages, shapes


def test_line_masks_equal_the_oracle_on_the_mixed_batch():
    names, pages, shapes = batch()
    hor, ver, off, bw = CCA._lines_mask(TW, pages, shapes, bw=True)
    for i, nm in enumerate(names):
        hw = shapes[i][:2]
        for key, buf in (("bw", bw), ("horizontal", hor), ("vertical", ver)):
            assert np.array_equal(TW.view(buf, int(off[i]), hw), K.oracle(nm)[key]), (nm, key)
    assert all(np.array_equal(p, K.pages()[nm]) for p, nm in zip(pages, names))


@pytest.mark.parametrize("which", ["page", "cleaned"])
def test_text_stages_equal_the_oracle_on_the_mixed_batch(which):
    names, pages, shapes = batch()
    if which == "cleaned":
        pages = [K.oracle(nm)["cleaned"] for nm in names]
    closed, off, st = CCA._text_mask(TW, pages, shapes, stages=True)
    for i, nm in enumerate(names):
        h, w = shapes[i][:2]
        want = K.oracle(nm)["stages_" + which]
        planes = st[4 * int(off[i]):4 * (int(off[i]) + h * w)].reshape(4, h, w)
        for k, key in enumerate(("blurred", "blackhat", "thresholded", "dilated")):
            assert np.array_equal(planes[k], want[k]), (nm, key)
        assert np.array_equal(TW.view(closed, int(off[i]), (h, w)), want[4]), (nm, "closed")


@pytest.mark.parametrize("external", [True, False])
def test_labelling_equals_the_oracle_on_every_binary_image(external):
    names = list(K.binaries())
    imgs = [K.binaries()[nm] for nm in names]
    got = CCA._label(TW, imgs, [a.shape for a in imgs], external_only=external)                 # one call for all
    for nm, g in zip(names, got):
        assert g.dtype == np.int32 and np.array_equal(g, K.oracle_components(nm, external)), nm


def test_every_result_equals_the_oracle_on_the_mixed_batch():
    names, pages, _shapes = batch()
    cleaned, line_boxes = CCA.remove_graphical_lines(pages, device=False)
    text = CCA.text_components(cleaned, device=False)
    heights, drawn = CCA.component_heights(cleaned, annotate=True, device=False)
    res = CCA.analyse_scan(pages, annotate=True, device=False)
    for i, nm in enumerate(names):
        o = K.oracle(nm)
        assert np.array_equal(line_boxes[i], o["line_boxes"]) and line_boxes[i].dtype == np.int32, nm
        assert np.array_equal(cleaned[i], o["cleaned"]) and cleaned[i] is not pages[i], nm
        assert np.array_equal(text[i], o["text_boxes"]), nm
        assert np.array_equal(heights[i], o["heights"]) and heights[i].dtype == np.int32, nm
        assert np.array_equal(drawn[i], o["annotated"]), nm
        for key in ("line_boxes", "cleaned", "heights", "histogram", "annotated"):
            assert np.array_equal(res[i][key], o[key]), (nm, key)
        assert res[i]["mode_bin"] == o["mode_bin"], nm
        assert np.array_equal(pages[i], K.pages()[nm]), nm                                      # the inputs are only read
    assert sum(len(o) for o in heights) > 0 and sum(len(b) for b in line_boxes) > 0
    assert np.array_equal(CCA.component_heights(cleaned, device=False)[3], heights[3])


def test_outlines_are_clipped_at_the_page_edges():
    page = np.full((40, 50, 3), 7, np.uint8)
    gray = np.full((33, 31), 7, np.uint8)
    boxes = [np.asarray([[0, 0, 20, 5], [30, 35, 20, 5], [10, 10, 30, 8], [49, 0, 1, 40]], np.int32),
             np.asarray([[0, 0, 31, 33], [5, 6, 20, 4]], np.int32)]
    pages, shapes = CCA._pages.check_pages([page.copy(), gray.copy()], CCA.MIN_SIDE, CCA.MAX_SIDE, False, upload=False)
    CCA._paint(TW, pages, shapes, boxes, CCA.OUTLINE)
    assert np.array_equal(pages[0], R.outline(page, boxes[0])) and np.array_equal(pages[1], R.outline(gray, boxes[1]))
    assert (pages[0] == (0, 255, 0)).all(-1).any() and (pages[1] == 255).any()
    pages, shapes = CCA._pages.check_pages([page.copy(), gray.copy()], CCA.MIN_SIDE, CCA.MAX_SIDE, False, upload=False)
    CCA._paint(TW, pages, shapes, boxes, CCA.FILL)
    for p, src, bs in zip(pages, (page, gray), boxes):
        want = src.copy()
        for x, y, w, h in bs:
            want[y:y + h, x:x + w] = 255
        assert np.array_equal(p, want)


def test_the_golden_sample_page_equals_the_oracle():
    page = K.golden_page()
    o = K.golden_oracle()
    r = CCA.analyse_scan([page], annotate=True, device=False)[0]
    for key in ("line_boxes", "cleaned", "heights", "histogram", "annotated"):
        assert np.array_equal(r[key], o[key]), key
    assert r["mode_bin"] == o["mode_bin"] == (24, 28)


def test_pages_of_the_largest_side_equal_the_oracle():
    for nm, page in K.long_pages().items():
        pages, shapes = CCA._pages.check_pages([page], CCA.MIN_SIDE, CCA.MAX_SIDE, False, upload=False)
        hor, ver, _off, bw = CCA._lines_mask(TW, pages, shapes, bw=True)
        wbw, whor, wver = R.line_masks(page)
        assert np.array_equal(bw.reshape(page.shape), wbw) and np.array_equal(hor.reshape(page.shape), whor), nm
        assert np.array_equal(ver.reshape(page.shape), wver), nm
        line = whor if page.shape[1] > page.shape[0] else wver
        assert line.any() and len(R.components(line)) == 2                                      # the rules of 600 and 584, not the one of 500
        closed, _off = CCA._text_mask(TW, pages, shapes)
        assert np.array_equal(closed.reshape(page.shape), R.text_stages(page)[4]), nm
        cleaned, boxes = CCA.remove_graphical_lines([page], device=False)
        wcleaned, wboxes = R.remove_lines(page)
        assert np.array_equal(boxes[0], wboxes) and np.array_equal(cleaned[0], wcleaned), nm


def label_raw(img, cap, external=1):
    hs, ws = np.asarray([img.shape[0]], np.int32), np.asarray([img.shape[1]], np.int32)
    capa, off = np.asarray([cap], np.int32), np.zeros(1, np.int64)
    counts, boxes = np.full(1, -1, np.int32), np.full(4 * max(cap, 1), -1, np.int32)
    ptrs = (C.c_void_p * 1)(img.ctypes.data)
    rc = L.lib.rtn_cca_label_host(1, ptrs, hs.ctypes.data, ws.ctypes.data, external, capa.ctypes.data, off.ctypes.data,
                                  counts.ctypes.data, boxes.ctypes.data, 16 * max(cap, 1))
    return rc, int(counts[0]), boxes.reshape(-1, 4)


def test_capacity_overflow_reports_the_true_count_and_einval():
    img = K.binaries()["isolated_pixels"]
    want = K.oracle_components("isolated_pixels", True)
    rc, count, boxes = label_raw(img, 10)
    assert rc == -1 and count == len(want) == 936                                               # RTN_EINVAL, never a silent cut
    assert "936 components, capacity 10" in L.lib.rtn_last_error(None).decode()
    assert np.array_equal(boxes, want[:10])
    rc, count, boxes = label_raw(img, 936)
    assert rc == 0 and count == 936 and np.array_equal(boxes, want)
    rc, count, _ = label_raw(img, 0)
    assert rc == -1 and count == 936
    with pytest.raises(L.RtnError):
        CCA._label(TW, [img], [img.shape], capacity=[935])
    assert len(CCA._label(TW, [img], [img.shape])[0]) == 936                                    # the default capacity cannot overflow


def test_sides_outside_30_to_16384_raise_before_anything_runs():
    ok = np.zeros((30, 30, 3), np.uint8)
    for bad in (np.zeros((29, 40, 3), np.uint8), np.zeros((40, 29), np.uint8), np.zeros((30, 16385), np.uint8)):
        for fn in (CCA.remove_graphical_lines, CCA.text_components, CCA.component_heights, CCA.analyse_scan):
            with pytest.raises(ValueError, match="page 1"):
                fn([ok, bad], device=False)
    with pytest.raises(ValueError, match="page 0"):
        CCA.analyse_scan([np.zeros((40, 40, 4), np.uint8)], device=False)
    with pytest.raises(ValueError, match="page 0"):
        CCA.analyse_scan([np.zeros((40, 40, 3), np.float32)], device=False)
    # the C entries check by themselves
    img = np.zeros((29, 64), np.uint8)
    assert label_raw(img, 4)[0] == -1 and "30 .. 16384" in L.lib.rtn_last_error(None).decode()
    assert L.lib.rtn_cca_workspace_bytes(1, np.asarray([29], np.int32).ctypes.data, np.asarray([64], np.int32).ctypes.data, 0) == 0
    assert CCA.analyse_scan([], device=False) == []
