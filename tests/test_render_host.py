"""CPU tests of the detection renderer's host half (csrc/rtn_render.h): the per-pixel rule (rtn_render_host) and the
kernel's tile walk run on the CPU (rtn_render_tiles_host) against a NumPy page put through the unchanged draw_box / extract_box /
draw_caption in render_detections' order; the caption mask helper; the kept-list helper; the empty-crop rule through the planner."""
import os

import numpy as np
import pytest

import render_cases as K

U = K.U
GUARD = 37           # bytes around the output buffer that must stay untouched; not a multiple of 16, so images start at odd alignments


def run_host(fn, pages, plan):
    """One call of a host twin over NumPy pages -> {(page, k): image}; nothing may be written outside the images."""
    buf = np.full(plan["out_bytes"] + 2 * GUARD, 0xA5, np.uint8)
    before = [p.copy() for p in pages]
    args = U._render_args(plan, [p.ctypes.data for p in pages], plan["masks"].ctypes.data if plan["masks"].size else None,
                          buf.ctypes.data + GUARD)
    rc = fn(*args)
    assert rc == 0, U.L.lib.rtn_last_error(None)
    assert all(np.array_equal(a, b) for a, b in zip(before, pages))
    out = buf[GUARD:GUARD + plan["out_bytes"]]
    used = np.zeros(out.size, bool)
    for _p, _k, h, w, off in plan["images"]:
        used[off:off + h * w * 3] = True
    assert np.all(buf[:GUARD] == 0xA5) and np.all(buf[GUARD + plan["out_bytes"]:] == 0xA5) and np.all(out[~used] == 0xA5)
    return K.images_of(plan, out)


def twins(pkg):
    return (("pixels", pkg._lib.lib.rtn_render_host), ("tiles", pkg._lib.lib.rtn_render_tiles_host))


@pytest.mark.parametrize("thickness", K.THICKNESSES)
def test_twins_equal_the_numpy_sequence_on_the_grid(pkg, thickness):
    pages, kept, want = K.grid_case(thickness)
    plan = U._render_plan([p.shape[:2] for p in pages], kept, K.LABELS, thickness=thickness)
    assert any(c is None for crops, _ in want for c in crops) and any(c is not None and c.shape[:2] == (1, 1) for crops, _ in want for c in crops)
    for name, fn in twins(pkg):
        K.assert_images(run_host(fn, pages, plan), kept, want, (name, thickness))


def test_twins_equal_the_numpy_sequence_on_300_boxes(pkg):
    pages, kept, want = K.many_case()
    assert len(kept[0]) == 300
    plan = U._render_plan([p.shape[:2] for p in pages], kept, K.LABELS)
    for name, fn in twins(pkg):
        K.assert_images(run_host(fn, pages, plan), kept, want, name)


def test_cases_cover_what_they_claim():
    """The case list holds what its comments say: captions clipped at the top, at the right, wholly off the page and whole; a later
    outline over an earlier caption and the reverse."""
    mh, mw = U._caption_mask("table 0.999").shape
    assert (mh, mw) == (40, 204)
    H, W = 37, 130
    b = K.boxes_for(H, W)
    assert 0 < b[6][1] - 10 < mh and b[6][0] + mw > W                              # clipped at the top and at the right
    assert b[10][0] >= W                                                           # caption wholly off the page
    H2, W2 = K.EXTRA_SHAPES[0]
    assert b[11][1] - 10 - mh >= 0 and b[11][1] - 10 <= H2 and b[11][0] + mw <= W2   # whole on the extra page
    page = np.full((H, W, 3), 100, np.uint8)
    dets = K.detections_for(H, W)
    _, after = K.numpy_sequence(page, dets[:7] + dets[7:8])
    _, without = K.numpy_sequence(page, dets[:7])
    red_before = (without == (0, 0, 255)).all(axis=2)
    assert (red_before & (after == 0).all(axis=2)).any()                           # outline 7 painted over caption 6
    _, with8 = K.numpy_sequence(page, dets[:9])
    black7 = (after == 0).all(axis=2)
    assert (black7 & (with8 == (0, 0, 255)).all(axis=2)).any()                     # caption 8 painted over outline 7


def test_caption_mask_is_what_draw_caption_paints():
    for text, size in (("table 0.912", 5), ("x", 1), ("table 1.000", 3)):
        mask = U._caption_mask(text, size)
        h, w = mask.shape
        canvas = np.full((h + 30, w + 20, 3), 7, np.uint8)
        U.draw_caption(canvas, [5, h + 15, 50, h + 20], text, font_size=size)
        want = np.full_like(canvas, 7)
        want[5:5 + h, 5:5 + w][mask] = (0, 0, 255)
        assert mask.dtype == bool and mask.any() and np.array_equal(canvas, want)
        gray = np.zeros((h + 30, w + 20), np.uint8)
        U.draw_caption(gray, [5, h + 15, 50, h + 20], text, font_size=size)
        assert np.array_equal(gray[5:5 + h, 5:5 + w] == 255, mask)


def render_inputs():
    """The inputs of tests/test_render.py."""
    boxes = np.full((1, 300, 4), -1, np.float32)
    scores = np.full((1, 300), -1, np.float32)
    labels = np.full((1, 300), -1, np.int32)
    boxes[0, 0], scores[0, 0], labels[0, 0] = [20, 40, 120, 160], 0.93, 0
    boxes[0, 1], scores[0, 1], labels[0, 1] = [30, 100, 140, 190], 0.71, 0
    boxes[0, 2], scores[0, 2], labels[0, 2] = [5, 5, 10, 10], 0.41, 0
    return boxes, scores, labels


def test_kept_helper_returns_what_render_detections_returns(tmp_path):
    boxes, scores, labels = render_inputs()
    for n, (scale, thr, first) in enumerate(((0.5, 0.6, 0.93), (1.0, 0.6, 0.3), (0.37, 0.2, 0.93))):
        scores[0, 0] = first
        page = np.full((400, 300, 3), 230, np.uint8)
        want = U.render_detections(None, page, boxes, scores, labels, scale, str(tmp_path / str(n)), "page_7.png", score_threshold=thr)
        got, ended = U._kept_detections(boxes, scores, labels, scale, thr)
        assert len(got) == len(want) and ended is not None
        for (gb, gs, gl), (wb, ws, wl) in zip(got, want):
            assert gb.dtype == wb.dtype and np.array_equal(gb, wb) and gs == ws and gl == wl and type(gs) is float and type(gl) is int
        assert ended == scores[0, len(got)]
    scores[:] = 0.9
    got, ended = U._kept_detections(boxes, scores, labels, 1.0, 0.6)
    assert len(got) == 300 and ended is None


def test_empty_crop_writes_no_file_and_leaves_the_others(pkg, tmp_path):
    """Planner + twin, no GPU: detection 1 lies off the page, so there is no file for k = 1, while k = 0 and k = 2 keep their
    numbers and pixels and the annotated page still shows outline and caption 1's visible parts."""
    from PIL import Image
    H, W = 60, 90
    page = K.page_of(H, W, 5)
    boxes = [(10, 20, 50, 55), (W + 1, 30, W + 20, 50), (30, 52, 80, 58)]
    kept = [K.detections_for(H, W, boxes), []]
    other = K.page_of(20, 30, 6)
    plan = U._render_plan([(H, W), (20, 30)], kept, K.LABELS)
    assert [(p, k) for p, k, *_ in plan["images"]] == [(0, 0), (0, 2), (0, None)]
    got = run_host(pkg._lib.lib.rtn_render_host, [page, other], plan)
    crops, annotated = K.numpy_sequence(page, kept[0])
    assert crops[1] is None and np.array_equal(got[(0, 0)], crops[0]) and np.array_equal(got[(0, 2)], crops[2])
    assert np.array_equal(got[(0, None)], annotated)
    rendered = [got[(p, k)] for p, k, *_ in plan["images"]]
    paths, images = U._render_files(plan, kept, [None, np.float32(0.25)], [page, other], rendered, str(tmp_path), ["a_1.png", "b.png"])
    for path, image in zip(paths, images):
        U.write_image(path, image)
    assert sorted(os.listdir(tmp_path / "detections_cropped")) == ["a_1_0.png", "a_1_2.png", "b_noDete_minScore-_0.25.png"]
    assert sorted(os.listdir(tmp_path / "detections_inImage")) == ["a_1.png", "b.png"]
    read = lambda *parts: np.asarray(Image.open(os.path.join(tmp_path, *parts)).convert("RGB"))[:, :, ::-1]
    assert np.array_equal(read("detections_cropped", "a_1_0.png"), crops[0]) and np.array_equal(read("detections_cropped", "a_1_2.png"), crops[2])
    assert np.array_equal(read("detections_inImage", "a_1.png"), annotated)
    assert np.array_equal(read("detections_inImage", "b.png"), other)
    assert np.array_equal(read("detections_cropped", "b_noDete_minScore-_0.25.png"), other)


def test_invalid_tables_are_refused_with_a_reason(pkg):
    lib = pkg._lib.lib
    page = K.page_of(8, 8, 1)
    kept = [K.detections_for(8, 8, [(1, 1, 6, 6)])]

    def call(change, fn=lib.rtn_render_host):
        plan = U._render_plan([(8, 8)], kept, K.LABELS)
        change(plan)
        buf = np.full(plan["out_bytes"], 0xA5, np.uint8)
        rc = fn(*U._render_args(plan, [page.ctypes.data], plan["masks"].ctypes.data, buf.ctypes.data))
        assert np.all(buf == 0xA5) or rc == 0
        return rc, lib.rtn_last_error(None).decode()

    assert call(lambda p: None)[0] == 0
    for fn in (lib.rtn_render_host, lib.rtn_render_tiles_host):
        for change, word in (
                (lambda p: p["out_rects"].__setitem__((0, 2), 9), "rectangle"),               # wider than the page
                (lambda p: p["out_rects"].__setitem__((1, 0), -1), "rectangle"),
                (lambda p: p["out_outlines"].__setitem__(0, 2), "outlines"),                  # more than the page has
                (lambda p: p["out_offsets"].__setitem__(1, p["out_bytes"] - 8), "bytes"),     # leaves the buffer
                (lambda p: p["out_offsets"].__setitem__(1, 3), "overlap"),
                (lambda p: p["mask_bits"].__setitem__(0, 8 * p["masks"].size - 100), "mask"),
                (lambda p: p["mask_pitch"].__setitem__(0, 8), "pitch"),
                (lambda p: p["boxes"].__setitem__((0, 0), 2 ** 31 - 1), "coordinate"),
                (lambda p: p["op_begin"].__setitem__(1, 2), "operations"),
                (lambda p: p["heights"].__setitem__(0, 0), "sides"),
                (lambda p: p.__setitem__("thickness", -1), "thickness")):
            rc, text = call(change, fn)
            assert rc == -1 and word in text, (word, rc, text)
    assert lib.rtn_render_workspace_bytes(-1, 0, 0) == 0 and lib.rtn_render_workspace_bytes(2, 600, 602) >= 2 * 24 + 600 * 48 + 602 * 40 + 603 * 4
    assert lib.rtn_render_pages(None, *U._render_args(U._render_plan([(8, 8)], kept, K.LABELS), [page.ctypes.data], None, None), None, 0) == -1
