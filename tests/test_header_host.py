"""CPU tests of header detection's host half (csrc/rtn_header.h): every CPU twin (rtn_header_*_host) against the NumPy
oracle (tests/header_ref.py) bit for bit on every case, with guard bytes around every output; the size limit; header_files' names."""
import ctypes as C
import os

import numpy as np
import pytest

import header_cases as K
import header_ref as R

HDR = K.HDR
L = HDR.L
GUARD = 37           # bytes around every output that must stay untouched; odd, so every buffer starts unaligned
FILL = 0xA5


class Guarded:
    """A byte buffer of n bytes between two guards."""

    def __init__(self, n):
        self.n = n
        self.buf = np.full(n + 2 * GUARD, FILL, np.uint8)
        self.ptr = self.buf.ctypes.data + GUARD

    def bytes(self):
        assert np.all(self.buf[:GUARD] == FILL) and np.all(self.buf[GUARD + self.n:] == FILL), "a twin wrote outside its output"
        return self.buf[GUARD:GUARD + self.n]

    def view(self, dtype):
        return np.frombuffer(self.bytes().tobytes(), dtype)


def check(rc):
    assert rc == 0, L.lib.rtn_last_error(None)


def run_twins(crops, ks=None, max_iter=300):
    """The four twins over one batch, called directly -> (plan, hsv, (centres, counts, passes, fx, labels), ks, hist, patches)."""
    crops = [np.ascontiguousarray(c) for c in crops]
    plan = HDR._plan([c.shape[:2] for c in crops])
    n, total = plan["n"], plan["total"]
    before = [c.copy() for c in crops]
    ptrs = (C.c_void_p * max(n, 1))(*[crops[i].ctypes.data for i in plan["idx"]])
    layout = (n, plan["dst"].ctypes.data, plan["offsets"].ctypes.data)
    hsv = Guarded(3 * total)
    check(L.lib.rtn_header_sample_host(n, ptrs, plan["heights"].ctypes.data, plan["widths"].ctypes.data, *layout[1:], hsv.ptr, hsv.n))
    assert all(np.array_equal(a, b) for a, b in zip(before, crops))
    hsv_b = hsv.bytes().copy()
    outs = [Guarded(n * 9 * 9 * 3 * 4), Guarded(n * 9 * 9 * 4), Guarded(n * 9 * 4), Guarded(n * 9 * 8), Guarded(9 * total)]
    check(L.lib.rtn_header_cluster_host(*layout, hsv.ptr, hsv.n, max_iter, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr,
                                        outs[4].ptr, outs[4].n))
    assert np.array_equal(hsv.bytes(), hsv_b)
    centres = outs[0].view(np.float32).reshape(n, 9, 9, 3)
    counts = outs[1].view(np.uint32).reshape(n, 9, 9)
    passes = outs[2].view(np.int32).reshape(n, 9)
    fx = outs[3].view(np.uint64).reshape(n, 9)
    labels = outs[4].bytes()
    if ks is None:
        ks = [HDR.opt_k([int(d) / 65536 / int(plan["points"][i]) for d in fx[i]]) or 5 for i in range(n)]
    ks_a = np.asarray(ks, np.int32)
    hist = Guarded(n * 9 * 3 * 256 * 4)
    check(L.lib.rtn_header_stats_host(*layout, ks_a.ctypes.data, hsv.ptr, hsv.n, outs[4].ptr, outs[4].n, hist.ptr))
    hist_a = hist.view(np.uint32).reshape(n, 9, 3, 256)
    # one patch per non-empty cluster of the chosen k, thresholds from the oracle's rule on the twin's histograms
    patch_crop, low, high = [], [], []
    for i in range(n):
        for j in range(ks[i]):
            if counts[i, ks[i] - 1, j]:
                st = HDR.histogram_stats(hist_a[i, j])
                patch_crop.append(i)
                low.append(np.array(np.clip(st["Q1"], 0, 255), dtype=np.uint8))
                high.append(np.array(np.clip(st["Q3"], 0, 255), dtype=np.uint8))
    pc = np.asarray(patch_crop, np.int32)
    lo, hi = np.ascontiguousarray(low, np.uint8).reshape(-1, 3), np.ascontiguousarray(high, np.uint8).reshape(-1, 3)
    gap = 5                                                        # unused bytes between patches stay untouched too
    sizes = plan["points"][pc] * 3
    offs = (np.concatenate([[0], np.cumsum(sizes + gap)])[:-1]).astype(np.int64)
    out = Guarded(int((sizes + gap).sum()))
    check(L.lib.rtn_header_patches_host(*layout, hsv.ptr, hsv.n, len(pc), pc.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                                        offs.ctypes.data, out.ptr, out.n))
    ob = out.bytes()
    patches = []
    for j in range(len(pc)):
        patches.append((int(pc[j]), lo[j], hi[j], ob[offs[j]:offs[j] + sizes[j]].reshape(-1, 500, 3)))
        assert np.all(ob[offs[j] + sizes[j]:offs[j] + sizes[j] + gap] == FILL)
    return plan, hsv_b, (centres, counts, passes, fx, labels), ks, hist_a, patches


def test_every_twin_equals_the_oracle_on_every_case():
    names = list(K.cases())
    plan, hsv, (centres, counts, passes, fx, labels), ks, hist, patches = run_twins([K.cases()[nm] for nm in names])
    assert [names[i] for i in plan["idx"]] == [nm for nm in names if nm != K.SKIPPED] and K.oracle(K.SKIPPED) is None
    for i, ci in enumerate(plan["idx"]):
        want = K.oracle(names[ci])
        off, N = int(plan["offsets"][i]), int(plan["points"][i])
        pts = hsv[3 * off:3 * (off + N)].reshape(-1, 3)
        assert np.array_equal(pts.reshape(want["hsv"].shape), want["hsv"]), names[ci]
        for k in range(1, 10):
            f = want["fits"][k - 1]
            where = (names[ci], k)
            assert np.array_equal(centres[i, k - 1, :k].view(np.uint32), f["centres"].view(np.uint32)), where
            assert np.all(centres[i, k - 1, k:].view(np.uint32) == 0) and np.all(counts[i, k - 1, k:] == 0), where
            assert np.array_equal(counts[i, k - 1, :k], f["counts"]) and passes[i, k - 1] == f["passes"], where
            assert int(fx[i, k - 1]) == f["distortion_fx"], where
            assert np.array_equal(labels[9 * off + (k - 1) * N:9 * off + k * N], f["labels"]), where
        assert ks[i] == want["k"]
        assert np.array_equal(hist[i], R.histograms(pts, want["fits"][ks[i] - 1]["labels"])), names[ci]
        mine = [p for p in patches if p[0] == i]
        assert len(mine) == len(want["patches"])
        for (_c, lo, hi, got), wp in zip(mine, want["patches"]):
            assert np.array_equal(got, wp), (names[ci], lo, hi)


def test_cases_cover_what_they_claim():
    c = K.cases()
    dh = {nm: R.sampled_height(*img.shape[:2]) for nm, img in c.items()}
    assert dh["identity_500x12"] == 12 and dh["half_1000x37"] == 18 and dh["fraction_1333x211"] == 79 and dh["enlarge_123x45"] == 182
    assert dh["one_pixel"] == 500 and dh[K.SKIPPED] == 0
    assert np.array_equal(R.box_resample(c["identity_500x12"], 12), c["identity_500x12"])
    one, two = K.oracle("one_pixel"), K.oracle("two_colours")
    assert all(int((f["counts"] > 0).sum()) == 1 for f in one["fits"])                    # every split has e = 0: the new cluster stays empty
    assert all(int((f["counts"] > 0).sum()) == min(k + 1, 2) for k, f in enumerate(two["fits"]))
    assert any(p > 2 for nm in c if nm != K.SKIPPED for p in K.oracle(nm)["passes"])      # some fit moves labels after its first pass


def test_explicit_k_keeps_the_indices_of_non_empty_clusters():
    got = HDR.detect_headers_twins([K.cases()["two_colours"], K.cases()[K.SKIPPED]], k=7)
    want = R.detect(K.cases()["two_colours"], k=7, chain=K.oracle("two_colours")["fits"])
    assert got[1] is None and got[0]["k"] == 7 and len(got[0]["clusters"]) == 2
    K.assert_result(got[0], want, "two colours, k = 7")
    assert [d["cluster_index"] for d in got[0]["dominant"]] == sorted(
        (c["cluster_index"] for c in got[0]["clusters"]), key=lambda j: -want["fits"][6]["counts"][j])
    with pytest.raises(ValueError):
        HDR.detect_headers_twins([K.cases()["two_colours"]], k=10)


def test_a_crop_past_the_point_limit_raises_before_any_entry_is_called(monkeypatch):
    calls = []
    monkeypatch.setattr(HDR._pages.Twins, "call", lambda self, name, args, workspace=None, extra=(): calls.append(name))
    assert R.sampled_height(*K.TOO_LARGE.shape[:2]) * 500 > 2 ** 21
    with pytest.raises(ValueError, match="crop 1"):
        HDR.detect_headers_twins([K.cases()["two_colours"], K.TOO_LARGE])
    assert calls == []
    ok = np.zeros((4194, 500, 3), np.uint8)                                              # the largest crop that passes: 2,097,000 points
    assert HDR._plan([ok.shape[:2]])["total"] == 4194 * 500 <= 2 ** 21
    with pytest.raises(ValueError):
        HDR._plan([(4195, 500)])


def test_twins_refuse_a_layout_that_does_not_fit():
    dst, off = np.array([2], np.int32), np.array([0], np.int64)
    hsv = np.zeros(3000, np.uint8)
    small = np.zeros(10, np.uint8)
    rc = L.lib.rtn_header_cluster_host(1, dst.ctypes.data, off.ctypes.data, hsv.ctypes.data, hsv.size, 300, small.ctypes.data,
                                       small.ctypes.data, small.ctypes.data, small.ctypes.data, small.ctypes.data, small.size)
    assert rc == -1 and b"labels" in L.lib.rtn_last_error(None)
    rc = L.lib.rtn_header_cluster_host(1, dst.ctypes.data, off.ctypes.data, hsv.ctypes.data, 2999, 300, None, None, None, None, None, 0)
    assert rc == -1 and b"H,S,V" in L.lib.rtn_last_error(None)


def test_header_files_names_through_the_twins(tmp_path):
    from PIL import Image
    src = tmp_path / "crops"
    src.mkdir()
    names = ["two_colours", K.SKIPPED, "table_sigma2"]
    paths = []
    for nm in names:
        p = str(src / ("%s.v1.png" % nm))
        Image.fromarray(K.cases()[nm][:, :, ::-1]).save(p)
        paths.append(p)
    out = str(tmp_path / "headerResults")
    results = HDR.header_files(paths, out, twins=True, k=None)
    assert sorted(os.listdir(out)) == sorted("test_%s" % nm for nm in names)           # the name up to the first dot
    assert os.listdir(os.path.join(out, "test_" + K.SKIPPED)) == ["OrigImage.png"] and results[1] is None

    def read(path):
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"))[:, :, ::-1]

    for nm, res in zip(names, results):
        if res is None:
            continue
        want = K.oracle(nm)
        K.assert_result(res, want, nm)
        d = os.path.join(out, "test_" + nm)
        expect = ["OrigImage.png", "colorBar.png"] + ["%s_HSVpatch_%d.png" % ("Selected" if c["selected"] else "Not_Selected",
                                                                             c["cluster_index"]) for c in want["clusters"]]
        assert sorted(os.listdir(d)) == sorted(expect)
        assert np.array_equal(read(os.path.join(d, "OrigImage.png")), K.cases()[nm])
        for c, p in zip(want["clusters"], want["patches"]):
            assert np.array_equal(read(os.path.join(d, expect[2 + want["clusters"].index(c)])), p)
        bar = read(os.path.join(d, "colorBar.png"))[:, :, ::-1]                          # R,G,B
        assert bar.shape == (100, 500, 3) and np.all(bar == bar[:1])
        edge = 0.0
        for x in want["dominant"][:-1]:                                                  # int-truncated edges, left to right by falling share
            nxt = edge + x["color_percentage"] * 500
            if int(nxt) - 1 > int(edge):
                assert tuple(bar[0, int(nxt) - 1]) == tuple(int(v) for v in x["RGB_color"])
            edge = nxt
    two = K.oracle("two_colours")                                                       # empty clusters are in neither list
    assert two["k"] == 2 and [c["cluster_index"] for c in two["clusters"]] == [0, 1]
    assert [d["cluster_index"] for d in two["dominant"]] == [0, 1] and two["dominant"][0]["color_percentage"] == 0.6
