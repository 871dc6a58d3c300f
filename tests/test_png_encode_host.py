"""rtn_png_encode_bound (host only): equals the derivation restated in tests/png_encode_ref.py over a grid of shapes, is 0 for
an invalid page, and is exact: a file of the layout with every chunk stored has that many bytes."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_ref as R  # noqa: E402


def lib():
    return importlib.import_module("retinanet-for-table-detection_amd._lib").lib


def test_chunk_size_is_the_header_s():
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtn.h")
    (line,) = [ln for ln in open(inc) if ln.startswith("#define RTN_PNG_CHUNK")]
    assert int(line.split()[2]) == R.CHUNK <= 32768


def test_bound_equals_the_formula():
    L = lib()
    shapes = [(1, 1), (1, 17), (17, 1), (5, 7), (333, 250), (1712, 2200), (65500, 1), (1, 65500), (30000, 20000)]
    # rows that end exactly on a chunk edge, and one byte past it: gray 1 + w = 32768, 32769; colour 1 + 3 w = 32768 has no
    # solution, so heights that make the whole stream a multiple: w = 1365 (row 4096 bytes), h = 8, 9; w = 341 (row 1024), h = 32, 33
    shapes += [(32767, 1), (32768, 1), (32767, 2), (32768, 2), (1365, 8), (1365, 9), (341, 32), (341, 33), (341, 64)]
    for w, h in shapes:
        for c in (1, 3):
            want = R.encode_bound(w, h, c)
            assert L.rtn_png_encode_bound(w, h, c) == want, (w, h, c)
            if want:
                s = h * (1 + w * c)
                assert want == 56 + s + 22 * -(-s // R.CHUNK)
    assert L.rtn_png_encode_bound(32767, 1, 1) == 56 + 32768 + 22          # one full chunk
    assert L.rtn_png_encode_bound(32768, 1, 1) == 56 + 32769 + 44          # one byte past it: a second chunk


def test_bound_is_zero_for_invalid_pages():
    L = lib()
    for w, h, c in [(0, 5, 3), (5, 0, 3), (-1, 5, 3), (5, -1, 1), (5, 5, 0), (5, 5, 2), (5, 5, 4), (5, 5, -3),
                    (65536, 32768, 1), (30000, 30000, 3)]:             # the last two: a filtered stream of 2^31 bytes or more
        assert L.rtn_png_encode_bound(w, h, c) == 0, (w, h, c)
        assert R.encode_bound(w, h, c) == 0, (w, h, c)
    assert L.rtn_png_encode_bound(65535, 32767, 1) == R.encode_bound(65535, 32767, 1) > 0      # 32767 * 65536 < 2^31


def test_all_stored_file_hits_the_bound():
    L = lib()
    rng = np.random.RandomState(1)
    for shape in [(1, 1), (1, 40, 3), (40, 1), (64, 511), (64, 512), (128, 255, 3), (200, 301, 3), (8, 1365, 3), (9, 1365, 3)]:
        page = rng.randint(0, 256, shape).astype(np.uint8)
        f = R.build_file(page, "up", stored=True)
        R.check_file(f, page)
        assert len(f) == L.rtn_png_encode_bound(shape[1], shape[0], 1 if len(shape) == 2 else 3), shape


def test_workspace_is_zero_for_invalid_arguments():
    L = lib()
    a = lambda *v: np.ascontiguousarray(v, np.int32)                    # noqa: E731
    w, h, c = a(10, 20), a(10, 20), a(3, 1)
    assert L.rtn_png_encode_workspace_bytes(2, w.ctypes.data, h.ctypes.data, c.ctypes.data) > 0
    assert L.rtn_png_encode_workspace_bytes(0, w.ctypes.data, h.ctypes.data, c.ctypes.data) == 0
    assert L.rtn_png_encode_workspace_bytes(2, None, h.ctypes.data, c.ctypes.data) == 0
    bad = a(3, 2)
    assert L.rtn_png_encode_workspace_bytes(2, w.ctypes.data, h.ctypes.data, bad.ctypes.data) == 0
