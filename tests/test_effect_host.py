"""CPU tests of the colour effects' host half (csrc/rtn_effect.h): the CPU twin rtn_visual_effect_host against the NumPy
oracle (tests/effect_ref.py) bit for bit on every case, in one batched call, with guard bytes around every output and the inputs
unchanged; in place; the argument errors."""
import ctypes as C
import importlib

import numpy as np

import effect_cases as K

L = importlib.import_module("retinanet-for-table-detection_amd")._lib
GUARD = 37           # bytes around every output that must stay untouched; odd, so every buffer starts unaligned
FILL = 0xA5


def ptrs(addresses):
    return (C.c_void_p * max(len(addresses), 1))(*addresses)


def run_twin(pages, params, flags, in_place=False):
    """One call of the twin over the whole batch -> the outputs; checks the guards and, out of place, that no input changed."""
    pages = [np.ascontiguousarray(p) for p in pages]
    heights, widths, par, fl = K.batch_arrays(pages, params, flags)
    bufs = [np.full(p.size + 2 * GUARD, FILL, np.uint8) for p in pages]
    if in_place:
        for b, p in zip(bufs, pages):
            b[GUARD:GUARD + p.size] = p.reshape(-1)
    src = [b.ctypes.data + GUARD for b in bufs] if in_place else [p.ctypes.data for p in pages]
    before = [p.copy() for p in pages]
    rc = L.lib.rtn_visual_effect_host(len(pages), ptrs(src), heights.ctypes.data, widths.ctypes.data, par.ctypes.data, fl.ctypes.data,
                                      ptrs([b.ctypes.data + GUARD for b in bufs]))
    assert rc == 0, L.lib.rtn_last_error(None)
    assert all(np.array_equal(a, b) for a, b in zip(before, pages))
    for b, p in zip(bufs, pages):
        assert np.all(b[:GUARD] == FILL) and np.all(b[GUARD + p.size:] == FILL), "the twin wrote outside an output"
    return [b[GUARD:GUARD + p.size].reshape(p.shape) for b, p in zip(bufs, pages)]


def assert_cases(got, where):
    for i, (name, _page, _params, _flags) in enumerate(K.cases()):
        want = K.oracle(i)
        assert np.array_equal(got[i], want), "%s, %s: %d bytes differ" % (where, name, int((got[i] != want).sum()))


def test_twin_equals_the_oracle_on_every_case_in_one_call():
    cs = K.cases()
    assert_cases(run_twin([c[1] for c in cs], [c[2] for c in cs], [c[3] for c in cs]), "out of place")


def test_twin_in_place():
    cs = K.cases()
    assert_cases(run_twin([c[1] for c in cs], [c[2] for c in cs], [c[3] for c in cs], in_place=True), "in place")


def test_null_flags_mean_no_flags_and_an_empty_batch_is_accepted():
    page = K.random_page(5, 17, 9)
    out = np.zeros_like(page)
    h, w, par, _ = K.batch_arrays([page], [(1.2, 0.1, 0.05, 0.9)], [0])
    assert L.lib.rtn_visual_effect_host(1, ptrs([page.ctypes.data]), h.ctypes.data, w.ctypes.data, par.ctypes.data, None,
                                        ptrs([out.ctypes.data])) == 0
    assert np.array_equal(out, K.R.effect(page, (1.2, 0.1, 0.05, 0.9)))
    assert L.lib.rtn_visual_effect_host(0, None, None, None, None, None, None) == 0
    assert L.lib.rtn_visual_effect_workspace_bytes(0, None, None) == 0


def test_cases_cover_what_they_claim():
    exact = K.exact_means_page()
    assert np.array_equal(K.R.channel_means(exact)[:2], [100.0, 0.0]) and set(exact[..., 0].ravel()) == set(range(256))
    ramp = K.ramp_page()
    assert set(ramp[..., 0].ravel()) == set(range(256)) == set(ramp[..., 1].ravel())
    names = [c[0] for c in K.cases()]
    i = names.index("raw_hue_%g" % K.TINY_HUE)
    assert K.oracle(i)[0, 0, 0] == 180                                      # mod(0 - 1.8e-20, 180) is 180.0
    i = names.index("hue_%g" % K.TINY_HUE)
    hsv = K.R.hue(K.R.bgr2hsv(K.cases()[i][1]), K.TINY_HUE)
    assert (hsv[..., 0] == 180).any()                                       # ... and that byte reaches HSV2BGR
    page = K.cases()[names.index("steps_0000")][1]
    lossy = K.oracle(names.index("forced_round_trip"))
    assert np.array_equal(K.oracle(names.index("steps_0000")), page) and (lossy != page).any()      # the round trip is no no-op
    stretched = K.R.contrast(page, 3.0)                                      # the contrast step clips at both ends ...
    assert (stretched == 0).any() and (stretched == 255).any() and len(np.unique(stretched)) > 2
    for d, end in ((1.0, 255), (-1.0, 0)):                                   # ... and the brightness step then clips all of it
        assert np.all(K.oracle(names.index("both_clips_%g" % d)) == end)


def fails(n, pages, heights, widths, params, flags, outs, text):
    rc = L.lib.rtn_visual_effect_host(n, pages, heights, widths, params, flags, outs)
    assert rc == -1 and text in L.lib.rtn_last_error(None), L.lib.rtn_last_error(None)


def test_twin_refuses_bad_arguments():
    page = K.random_page(6, 8, 1)
    out = np.zeros_like(page)
    h, w, par, fl = K.batch_arrays([page], [(1.1, 0.0, 0.0, 0.0)], [0])
    src, dst = ptrs([page.ctypes.data]), ptrs([out.ctypes.data])
    arg = lambda a: a.ctypes.data
    fails(-1, src, arg(h), arg(w), arg(par), arg(fl), dst, b"pages")
    fails(65536, src, arg(h), arg(w), arg(par), arg(fl), dst, b"pages")
    fails(1, src, None, arg(w), arg(par), arg(fl), dst, b"heights")
    fails(1, None, arg(h), arg(w), arg(par), arg(fl), dst, b"expected")
    fails(1, src, arg(h), arg(w), None, arg(fl), dst, b"expected")
    fails(1, ptrs([0]), arg(h), arg(w), arg(par), arg(fl), dst, b"missing")
    fails(1, src, arg(h), arg(w), arg(par), arg(fl), ptrs([0]), b"missing")
    for bad in (0, 65501):
        fails(1, src, arg(np.array([bad], np.int32)), arg(w), arg(par), arg(fl), dst, b"65500")
        fails(1, src, arg(h), arg(np.array([bad], np.int32)), arg(par), arg(fl), dst, b"65500")
        assert L.lib.rtn_visual_effect_workspace_bytes(1, arg(np.array([bad], np.int32)), arg(w)) == 0
    for v in (np.nan, np.inf, -np.inf):
        fails(1, src, arg(h), arg(w), arg(np.array([1.0, 0.0, v, 0.0])), arg(fl), dst, b"finite")
    fails(1, src, arg(h), arg(w), arg(par), arg(np.array([2], np.uint32)), dst, b"flag")
    fails(1, src, arg(h), arg(w), arg(par), arg(fl), ptrs([page.ctypes.data + 3]), b"overlaps")
    assert np.all(out == 0)
