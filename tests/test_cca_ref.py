"""The scan-analysis oracle (tests/cca_ref.py) against independent statements of the same things (no GPU): the external set against
hole filling, the histogram against np.histogram, hand-computed boxes, the blur taps, and the golden sample page's figures."""
import numpy as np
from scipy import ndimage

import cca_cases as K
import cca_ref as R

CCA = K.CCA


def test_external_components_equal_the_hole_filling_definition():
    nested = 0
    for nm, img in K.binaries().items():
        ext = R.components(img, True)
        assert np.array_equal(ext, R.components_by_hole_filling(img)), nm
        nested += len(R.components(img, False)) - len(ext)
    rng = np.random.default_rng(11)
    for i in range(120):
        h, w = rng.integers(5, 41, 2)
        img = (rng.random((h, w)) < rng.choice([0.3, 0.5, 0.6, 0.7])).astype(np.uint8)
        ext = R.components(img, True)
        assert np.array_equal(ext, R.components_by_hole_filling(img)), i
        nested += len(R.components(img, False)) - len(ext)
    assert nested > 20                                             # the two definitions were compared where they matter


def test_components_are_ordered_by_their_first_pixel_and_boxed_by_their_pixels():
    img = K.binaries()["random_50"]
    lab, n = ndimage.label(img != 0, structure=np.ones((3, 3)))
    want = []
    for i in range(1, n + 1):
        yx = np.argwhere(lab == i)                                  # in raster order
        (y0, x0), (y1, x1) = yx.min(0), yx.max(0)
        want.append((int(yx[0][0]) * img.shape[1] + int(yx[0][1]), [x0, y0, x1 - x0 + 1, y1 - y0 + 1]))
    assert R.components(img, False).tolist() == [b for _first, b in sorted(want)]


def test_hand_computed_boxes_of_the_ring_cases():
    assert R.components(K.binaries()["diagonal_ring"], True).tolist() == [list(b) for b in K.DIAGONAL_RING_BOXES[False]]
    assert R.components(K.binaries()["diagonal_ring_gap"], True).tolist() == [list(b) for b in K.DIAGONAL_RING_BOXES[True]]
    assert R.components(K.binaries()["diagonal_ring"], False).tolist() == [[10, 10, 31, 26], [20, 20, 6, 4]]
    # nested_rings: the outer ring and the free blob are external; seven components in all
    assert R.components(K.binaries()["nested_rings"], True).tolist() == [[5, 4, 66, 57], [80, 66, 10, 4]]
    assert len(R.components(K.binaries()["nested_rings"], False)) == 7
    assert R.components(K.binaries()["frame_with_blobs"], True).tolist() == [[0, 0, 67, 50]]
    assert len(R.components(K.binaries()["isolated_pixels"], True)) == CCA.max_components(51, 71) == 26 * 36
    assert len(R.components(K.binaries()["blank"], True)) == 0


def test_height_histogram_equals_numpy():
    rng = np.random.default_rng(3)
    lists = [[], [0], [100], [101, -1, 4], [3, 4, 4, 8, 99, 100, 100, 96], rng.integers(0, 130, 500), rng.integers(20, 32, 64)]
    for heights in lists:
        counts, lo, hi = CCA.height_histogram(heights)
        want, edges = np.histogram(np.asarray(heights, np.float64), 25, (0, 100))
        assert np.array_equal(counts, want)
        assert (lo, hi) == (edges[np.argmax(want)], edges[np.argmax(want)] + 4) == R.histogram(heights)[1:]


def test_blur_taps_and_the_folded_dilation():
    assert R.blur_taps().tolist() == [0, 27, 202, 27, 0]
    th = K.oracle("page_window")["stages_page"][2]
    assert np.array_equal(K.oracle("page_window")["stages_page"][3], R.dilate(th, 28, 18, 1))     # 9 x (1x4 at 2) = 1x28 at 18


def test_the_ruled_table_has_its_rules_found_and_the_exact_width_blob_kept():
    o = K.oracle("ruled_table")
    w = K.pages()["ruled_table"].shape[1]
    hor = o["horizontal"]
    # a run of exactly L = 6 at 90 .. 95: the erosion by [x - 3, x + 2] leaves x = 93, the dilation by the same window (no
    # reflection) gives 91 .. 96; a run of 5 leaves nothing
    assert w // 30 == 6 and hor[48:52, 91:97].all() and not hor[48:52, 90].any()
    assert not hor[120:126, 138:148].any()
    assert hor[80, 0:120].all()                                    # the rule from the page's edge
    assert (o["cleaned"][20:22, 15:185] == 255).all() and (o["cleaned"][20:142, 70:72] == 255).all()


def test_golden_sample_page_figures():
    o = K.golden_oracle()
    closed = R.text_stages(o["cleaned"])[4]
    assert len(o["line_boxes"]) == 0                               # the page has no rules
    assert len(o["text_boxes"]) == 252 == len(R.components(closed, False))      # all of them external
    assert len(o["heights"]) == 62
    assert o["mode_bin"] == (24, 28)
    assert o["histogram"].tolist() == [0, 1, 1, 3, 2, 7, 26, 14, 7, 1] + [0] * 15
