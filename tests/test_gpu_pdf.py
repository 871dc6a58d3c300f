"""GPU tests of scanned-PDF input (model/pdf.py, csrc/rtn_compose.hip, detect_pdf_files): the corpus of
tests/pdf_cases.py read in one call with the builder's pixels bit for bit, on the device decoders and through Pillow; the compose
kernels against the CPU twin on the grid of tests/test_pdf_host.py in one mixed batch, twice; the page that needs no compose;
write_pages_pdf read back; detect_pdf_files with a stub model against the oracle's box mapping and against detect_raw_files on the
same pages as PNG files.  Every test but the last fails without the feature: the module and the entry do not exist."""
import ctypes as C
import hashlib
import importlib
import os
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_cases as LK  # noqa: E402
import pdf_cases as K  # noqa: E402
import pdf_ref as R  # noqa: E402
from test_gpu_lattice import StubModel, tree  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module("retinanet-for-table-detection_amd.model.pdf")


@pytest.fixture(scope="module")
def U(pkg):
    return importlib.import_module("retinanet-for-table-detection_amd.model.utils")


@pytest.fixture
def device_path(monkeypatch):
    for name in ("RTN_TIFF_MIN", "RTN_PNG_STREAM_MIN", "RTN_PNG_LAYOUT_MIN", "RTN_PDF_G4_MIN"):
        monkeypatch.setenv(name, "1")
    return monkeypatch


def readable():
    return [(name, case) for name, case in K.corpus().items() if case.error is None]


def check_corpus(P, device_only):
    names, cases = zip(*readable())
    pages, infos = P.read_pdfs_pages([c.pdf for c in cases], return_info=True)
    assert len(pages) == len(infos) == len(cases)
    for name, case, got, info in zip(names, cases, pages, infos):
        assert len(got) == len(case.pages) == len(info.pages), name
        for g, want, page in zip(got, case.pages, info.pages):
            if isinstance(want, str):
                assert g is None and want in page.refused, name
                continue
            assert g is not None, (name, page.refused)
            assert g.is_cuda and g.dtype == torch.uint8 and g.is_contiguous() and tuple(g.shape) == want.shape, name
            assert np.array_equal(g.cpu().numpy(), want), name
            assert all(im.route in ("device", "host") for im in page.images)
            if device_only and not case.host_only:
                assert [im.route for im in page.images] == ["device"] * len(page.images), name


def test_corpus_in_one_call_on_the_device_decoders(P, device_path):
    check_corpus(P, device_only=True)


def test_corpus_in_one_call_with_the_default_minimums(P, monkeypatch):
    for name in ("RTN_TIFF_MIN", "RTN_PNG_STREAM_MIN", "RTN_PNG_LAYOUT_MIN", "RTN_PDF_G4_MIN", "RTN_TIFF_G4_ONE_STRIP"):
        monkeypatch.delenv(name, raising=False)
    check_corpus(P, device_only=False)


def test_a_refused_file_raises_pdferror(P):
    for name, case in K.corpus().items():
        if case.error is not None:
            with pytest.raises(P.PdfError, match=case.error):
                P.read_pdf_pages(case.pdf)


def test_compose_equals_the_twin_on_the_grid_in_one_batch_twice(pkg, P):
    from test_pdf_host import run_twin
    L = pkg._lib
    pages_hw, items = K.compose_grid()
    rc, why, want = run_twin(pkg, pages_hw, items)
    assert rc == 0, why
    sources = {id(it[0]): torch.from_numpy(it[0]).cuda() for it in items}
    canvases = [torch.full((h, w, 3), 7, dtype=torch.uint8, device="cuda") for h, w in pages_hw]
    table = (L.ComposeItem * len(items))()
    for e, (S, code, invert, page, x, y, cx, cy, cw, ch) in zip(table, items):
        e.src, e.h, e.w, e.orientation, e.invert = sources[id(S)].data_ptr(), S.shape[0], S.shape[1], code, invert
        e.page, e.x, e.y, e.crop_x, e.crop_y, e.crop_w, e.crop_h = page, x, y, cx, cy, cw, ch
    ptrs = (C.c_void_p * len(canvases))(*[c.data_ptr() for c in canvases])
    widths, heights = (np.ascontiguousarray([hw[k] for hw in pages_hw], np.int32) for k in (1, 0))
    h = importlib.import_module("retinanet-for-table-detection_amd.model._rt").handle()
    wsb = int(L.lib.rtn_page_compose_workspace_bytes(len(items), len(canvases)))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    for fill in (7, 200):
        for c in canvases:
            c.fill_(fill)
        ws.fill_(fill)
        h.check(L.lib.rtn_page_compose(h.raw, len(items), table, len(canvases), ptrs, widths.ctypes.data, heights.ctypes.data, ws.data_ptr(), wsb))
        torch.cuda.synchronize()
        for k, (g, w) in enumerate(zip(canvases, want)):
            assert np.array_equal(g.cpu().numpy(), w), (fill, k)
    # the plan check on the device entry: refused before anything is launched
    table[1].x = pages_hw[table[1].page][1]
    for c in canvases:
        c.fill_(9)
    rc = L.lib.rtn_page_compose(h.raw, len(items), table, len(canvases), ptrs, widths.ctypes.data, heights.ctypes.data, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    assert rc == -1 and "outside its page" in L.lib.rtn_last_error(h.raw).decode()
    assert all(bool((c == 9).all()) for c in canvases[:4])


def test_a_single_upright_image_is_the_decoders_tensor(P, device_path, monkeypatch):
    PIO = importlib.import_module("retinanet-for-table-detection_amd.model.page_io")
    seen = []
    real = PIO._decode_datas

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.extend(out[0])
        return out

    def no_compose(*a, **kw):
        raise AssertionError("rtn_page_compose must not be launched for a page that is one upright image")

    monkeypatch.setattr(PIO, "_decode_datas", spy)
    monkeypatch.setattr(P, "_compose", no_compose)
    for name in ("flate_png15_rgb_icc", "g4_blackis1", "dct_gray", "raw_gray", "pillow_three_pages"):
        del seen[:]
        got = P.read_pdf_pages(K.corpus()[name].pdf)
        assert len(got) == len(seen) and all(g is s for g, s in zip(got, seen)), name
    with pytest.raises(AssertionError, match="must not be launched"):
        P.read_pdf_pages(K.corpus()["rotate_90"].pdf)


def bilevel_pages():
    return [K.gray_image(h, w, 200 + h) for h, w in ((263, 131), (64, 64), (70, 131))]


def test_write_pages_pdf_g4_reads_back_to_the_thresholded_pages(P, monkeypatch):
    for name in ("RTN_TIFF_MIN", "RTN_PDF_G4_MIN", "RTN_TIFF_G4_ONE_STRIP"):
        monkeypatch.delenv(name, raising=False)
    pages = bilevel_pages()
    data = P.write_pages_pdf(None, pages, tiff="g4")
    info = P.pdf_inspect(data)
    assert [(p.width, p.height, len(p.images)) for p in info.pages] == [(131, 263, 5), (64, 64, 1), (131, 70, 2)]
    assert all(im.filter == "CCITTFaxDecode" and im.height <= 64 for p in info.pages for im in p.images)
    got, info = P.read_pdf_pages(data, return_info=True)
    for g, page in zip(got, pages):
        want = np.where(page < 128, 0, 255).astype(np.uint8)
        assert np.array_equal(g.cpu().numpy(), np.repeat(want[:, :, None], 3, axis=2))
    assert [im.route for p in info.pages for im in p.images] == ["device"] * 8          # one wave per strip, RTN_TIFF_MIN at its default


def test_write_pages_pdf_jpeg_reads_back_to_pillows_decode(P, tmp_path):
    pages = [K.bgr(K.rgb_image(70, 131, 300)), K.gray_image(65, 129, 301), torch.from_numpy(K.bgr(K.rgb_image(33, 31, 302))).cuda()]
    path = str(tmp_path / "archive.pdf")
    assert P.write_pages_pdf(path, pages, quality=90, dpi=200) is None
    data = open(path, "rb").read()
    want = K.pillow_jpeg_pixels(data)
    got, info = P.read_pdf_pages(path, return_info=True)
    assert len(got) == len(want) == 3 and [p.refused for p in info.pages] == [None] * 3
    assert all(abs(p.sx - 200 / 72) < 1e-6 for p in info.pages)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    assert np.array_equal(P.read_pdf_pages_host(data)[1], want[1])


# ---- detect_pdf_files -------------------------------------------------------------------------------------------------------------------------
NAMES = ["overlapping", "table_ell", "borderless"]               # 150 x 200, 150 x 200 and 120 x 200 pages with their table boxes
KW = dict(batch_size=2, min_side=150, max_side=200)             # every page keeps its size: the boxes are page pixels


def scan_page(b_g_r, rotate=None, content=None):
    """A page showing the B,G,R array after its /Rotate: the image is stored turned back."""
    stored = np.ascontiguousarray(np.rot90(b_g_r, (rotate or 0) // 90))
    h, w = stored.shape[:2]
    d = K.image_dict(w, h, "/ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /FlateDecode")
    return {"media": (0, 0, w, h), "rotate": rotate, "contents": [("", content or K.draw("Im0", K.upright(w, h)))],
            "images": {"Im0": (d, zlib.compress(stored[:, :, ::-1].tobytes()), [])}}


def write_corpus(tmp_path):
    """first.pdf: a page and a page with text (refused); second.pdf: a /Rotate 90 page and a page.  -> (paths, the three read pages
    as (file, page index, lattice case))."""
    cases = LK.cases()
    first = K.simple([scan_page(cases[NAMES[0]]["page"]), scan_page(cases[NAMES[0]]["page"], content=b"BT ET\n")])[0]
    second = K.simple([scan_page(cases[NAMES[1]]["page"], rotate=90), scan_page(cases[NAMES[2]]["page"])], xref="stream")[0]
    paths = [str(tmp_path / "first.pdf"), str(tmp_path / "second.pdf")]
    for path, data in zip(paths, (first, second)):
        with open(path, "wb") as f:
            f.write(data)
    return paths, [(0, 0, NAMES[0]), (1, 0, NAMES[1]), (1, 1, NAMES[2])]


def test_detect_pdf_files_against_the_oracle_and_detect_raw_files(P, U, tmp_path):
    paths, read = write_corpus(tmp_path)
    cases = LK.cases()
    per_page = [cases[nm]["boxes"] for _f, _k, nm in read]
    out = str(tmp_path / "pdf")
    with pytest.warns(UserWarning, match="page 2 skipped.*operator BT"):
        got = U.detect_pdf_files(StubModel(per_page), paths, out, cells=True, **KW)
    assert [(p, k) for p, k, _kept in got] == [(paths[0], 0), (paths[0], 1), (paths[1], 0), (paths[1], 1)]
    assert got[1][2] is None and [len(g[2]) for g in got if g[2] is not None] == [len(b) for b in per_page]
    names = ["first_Page1-72.png", "second_Page1-72.png", "second_Page2-72.png"]
    files = tree(out)
    for name in names:
        assert os.path.join("detections_inImage", name) in files, sorted(files)
    # the CSVs in points: the oracle's way back from the stub's boxes
    infos = [P.pdf_inspect(open(p, "rb").read()) for p in paths]
    want = {0: [], 1: []}
    for (f, k, _nm), kept in zip(read, [g[2] for g in got if g[2] is not None]):
        page = infos[f].pages[k]
        for box, _score, _label in kept:
            pts = R.pixels_to_points(tuple(float(v) for v in box), page.media_box, page.sx, page.sy, page.rotate, (page.width, page.height))
            want[f].append("%s_Page%d,%s,table" % (("first", "second")[f], k + 1, ",".join(str(int(v)) for v in pts)))
    for f, stem in enumerate(("first", "second")):
        text = files[os.path.join("pdfResults", stem + "_tables.csv")].decode()
        assert text == "\r\n".join(["image_id,xmin,ymin,xmax,ymax,label"] + want[f]) + "\r\n", stem
    assert len(want[0]) + len(want[1]) == sum(len(b) for b in per_page) >= 3
    assert infos[1].pages[0].rotate == 90 and (infos[1].pages[0].width, infos[1].pages[0].height) == (200, 150)
    # the same pages as PNG files under the same names through detect_raw_files: the same files, cells included
    png_dir = tmp_path / "png"
    png_dir.mkdir()
    png_paths = []
    for name, (_f, _k, nm) in zip(names, read):
        png_paths.append(str(png_dir / name))
        Image.fromarray(np.ascontiguousarray(cases[nm]["page"][:, :, ::-1])).save(png_paths[-1])
    raw = str(tmp_path / "raw")
    U.detect_raw_files(StubModel(per_page), png_paths, raw, factors=[1.0] * 3, cells=True, **KW)
    theirs = tree(raw)
    assert any(k.startswith("cellResults") for k in theirs)
    assert {k: v for k, v in files.items() if not k.startswith("pdfResults")} == theirs


RAW_DIGEST = "48a0e47de9ded0419276d623344af640a822106e876f22302c74fc950df80fc4"


def test_detect_raw_files_writes_the_parent_commits_bytes(U, tmp_path):
    """detect_raw_files shares its batch body with detect_pdf_files now; its files must not change by a byte.  RAW_DIGEST is the
    SHA-256 over the sorted (relative path, bytes) of everything the parent commit (1e74b86) wrote for this call on an MI355X,
    recorded there before the body was shared."""
    cases = LK.cases()
    paths = []
    for nm in NAMES:
        paths.append(str(tmp_path / (nm + ".png")))
        Image.fromarray(np.ascontiguousarray(cases[nm]["page"][:, :, ::-1])).save(paths[-1])
    out = str(tmp_path / "out")
    U.detect_raw_files(StubModel([cases[nm]["boxes"] for nm in NAMES]), paths, out, factors=[1.0, 1.0, 1.0], cells=True, headers=False, **KW)
    assert raw_digest(out) == RAW_DIGEST


def raw_digest(root):
    h = hashlib.sha256()
    for rel, data in sorted(tree(root).items()):
        h.update(rel.encode() + b"\0" + str(len(data)).encode() + b"\0" + data)
    return h.hexdigest()
