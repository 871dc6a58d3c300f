"""GPU tests of table structure (csrc/rtn_lattice.hip): every device output against its CPU twin's bytes on one mixed
batch, in two calls on the same buffers; the 30 x 16384 page; table_cells against the NumPy oracle (tests/lattice_ref.py) from
CUDA tensors and from NumPy arrays; cells_files on three small files; detect_files(cells=True) on a stub model with fixed boxes."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import lattice_cases as K
import lattice_ref as R

pytestmark = pytest.mark.gpu
S = K.S
KW = dict(flavor="auto", line_scale=15, line_tol=2, cover=50, col_gap=12, row_gap=4, margin=10)
STAGES = ("profiles", "edges", "cell_ink", "cell_box")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def stages(pages, boxes, device, bufs=None):
    pages, shapes = S._pages.check_pages(pages, S.MIN_SIDE, S.MAX_SIDE, device)
    be = S._pages.Device(pages[0].device) if device else S._pages.Twins()
    raw = {}
    grids = S._grids(be, pages, shapes, S._check_boxes(boxes, len(pages)), bufs=bufs, raw=raw, **KW)
    return grids, raw


def assert_same(got, want):
    assert got["live"] == want["live"] and got["flavors"] == want["flavors"]
    for key in ("bw", "hm", "vm", "ink"):
        assert np.array_equal(got["masks"][key], want["masks"][key]), key
    for key in STAGES:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key


def test_every_device_output_equals_the_twins_on_the_mixed_batch_twice(pkg):
    names = list(K.cases())
    pages, boxes = [K.cases()[nm]["page"] for nm in names], [K.cases()[nm]["boxes"] for nm in names]
    assert any(p.ndim == 2 for p in pages) and any(len(b) == 0 for b in boxes) and any(len(b) == 2 for b in boxes)
    _wgrids, want = stages(pages, boxes, False)
    assert {"lattice", "stream", "none"} <= set(want["flavors"]) and want["edges"].size > 100 and want["cell_ink"].size > 50
    dev, bufs = [cuda(p) for p in pages], {}
    _g, got = stages(dev, boxes, True, bufs)
    assert_same(got, want)
    first = {k: v.data_ptr() for k, v in bufs.items()}
    for v in bufs.values():                                                     # whatever the buffers hold, the second call gives the same bytes
        v.fill_(85)
    _g, again = stages(dev, boxes, True, bufs)
    assert {k: v.data_ptr() for k, v in bufs.items()} == first
    assert_same(again, want)
    assert all(np.array_equal(d.cpu().numpy(), p) for d, p in zip(dev, pages))                    # the pages are only read


def test_the_longest_page(pkg):
    c = K.long_case()
    _wg, want = stages([c["page"]], [c["boxes"]], False)
    grids, got = stages([cuda(c["page"])], [c["boxes"]], True)
    assert_same(got, want)
    assert K.same_grid(grids[0][0], K.oracle("long")[0]) is None


@pytest.mark.parametrize("source", ["cuda", "numpy"])
def test_table_cells_equals_the_oracle(pkg, source):
    names = list(K.cases()) + ["golden"]
    cs = [K.golden_case() if nm == "golden" else K.cases()[nm] for nm in names]
    pages = [cuda(c["page"]) if source == "cuda" else c["page"] for c in cs]
    got = S.table_cells(pages, [c["boxes"] for c in cs])
    for nm, grids in zip(names, got):
        want = K.oracle(nm)
        assert len(grids) == len(want)
        for k, (g, w) in enumerate(zip(grids, want)):
            assert K.same_grid(g, w) is None, (nm, k, K.same_grid(g, w))
    assert sum(len(g.cells) for g in got[-1]) > 0


def read_bgr(path):
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def write_pages(tmp_path, names):
    paths = []
    for nm in names:
        paths.append(str(tmp_path / (nm + ".png")))
        Image.fromarray(np.ascontiguousarray(K.cases()[nm]["page"][:, :, ::-1])).save(paths[-1])
    return paths


def test_cells_files_writes_the_csvs_and_the_outlined_pages(pkg, tmp_path):
    names = ["table_ell", "borderless", "overlapping"]
    paths = write_pages(tmp_path, names)
    out = str(tmp_path / "out")
    grids = S.cells_files(paths, [K.cases()[nm]["boxes"] for nm in names], out, outline=True)
    expected = set()
    for nm, page_grids in zip(names, grids):
        want = K.oracle(nm)
        for k, w in enumerate(want):
            assert K.same_grid(page_grids[k], w) is None
            expected.add("%s_table%d_cells.csv" % (nm, k))
            assert open(os.path.join(out, "%s_table%d_cells.csv" % (nm, k)), newline="").read() == R.csv_text(w)
        boxes = [(max(c[4], 0), max(c[5], 0), c[6] - max(c[4], 0), c[7] - max(c[5], 0)) for w in want for c in w["cells"]]
        expected.add(nm + "_cells.png")
        assert np.array_equal(read_bgr(os.path.join(out, nm + "_cells.png")), R.outline(K.cases()[nm]["page"], boxes)), nm
    assert set(os.listdir(out)) == expected
    plain = str(tmp_path / "plain")
    S.cells_files(paths[:1], [K.cases()["table_ell"]["boxes"]], plain, device=False)
    assert os.listdir(plain) == ["table_ell_table0_cells.csv"]
    assert open(os.path.join(plain, "table_ell_table0_cells.csv")).read() == open(os.path.join(out, "table_ell_table0_cells.csv")).read()


class StubModel:
    """The inference model detect_files asks for, whose engine reports fixed boxes page after page (score 0.9, label 0)."""
    bbox, nms, class_specific_filter, dtype = True, True, True, "f32"

    def __init__(self, per_page):
        self.per_page, self.seen = per_page, 0

    def _root(self):
        return self

    def engine(self):
        return self

    def detect(self, canvas, nms=True, class_specific_filter=True):
        n = canvas.shape[0]
        boxes, scores = torch.zeros(n, 300, 4), torch.full((n, 300), -1.0)
        labels = torch.full((n, 300), -1, dtype=torch.int32)
        for i in range(n):
            b = self.per_page[self.seen + i]
            boxes[i, :len(b)] = torch.as_tensor(np.asarray(b, np.float32).reshape(-1, 4))
            scores[i, :len(b)] = 0.9
            labels[i, :len(b)] = 0
        self.seen += n
        return boxes.cuda(), scores.cuda(), labels.cuda()


def tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _s, fs in os.walk(root) for f in fs}


def test_detect_files_with_cells_writes_the_same_csvs_and_nothing_else_changes(pkg, tmp_path):
    import importlib
    U = importlib.import_module("retinanet-for-table-detection_amd.model.utils")
    names = ["overlapping", "table_ell", "borderless"]                          # 150 x 200, 150 x 200 and 120 x 200: two batches
    paths = write_pages(tmp_path, names)
    per_page = [K.cases()[nm]["boxes"] for nm in names]
    kw = dict(batch_size=2, min_side=150, max_side=200)                         # every page keeps its size: the boxes are page pixels
    with_cells, without = str(tmp_path / "cells"), str(tmp_path / "plain")
    kept = U.detect_files(StubModel(per_page), paths, paths, with_cells, cells=True, **kw)
    assert [len(k) for k in kept] == [2, 1, 1]
    U.detect_files(StubModel(per_page), paths, paths, without, **kw)
    got, plain = tree(with_cells), tree(without)
    assert plain and not any(k.startswith("cellResults") for k in plain)
    assert {k: v for k, v in got.items() if not k.startswith("cellResults")} == plain           # cells=True adds files and changes none
    csvs = {k: v.decode() for k, v in got.items() if k.startswith("cellResults")}
    want = {}
    for nm, page_kept in zip(names, kept):
        page = K.cases()[nm]["page"]
        for k, (box, _score, _label) in enumerate(page_kept):
            want[os.path.join("cellResults", "%s_table%d_cells.csv" % (nm, k))] = R.csv_text(R.grid(page, box))
    assert csvs == want and len(want) == 4
    assert want[os.path.join("cellResults", "table_ell_table0_cells.csv")] == R.csv_text(K.oracle("table_ell")[0])
