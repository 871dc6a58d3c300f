"""GPU tests of the colour effects (csrc/rtn_effect.hip): rtn_visual_effect_u8 against the NumPy oracle
(tests/effect_ref.py) bit for bit on every case, all of them in one batched call; in place; unaligned pages; the surface of
model/transform.py; a CSVGenerator batch with effects against oracle effect -> oracle warp -> resize with the tolerance
tests/test_gpu_generator.py uses for that pipeline; the default generator unchanged."""
import ctypes as C
import importlib
import random
import warnings

import numpy as np
import pytest
import torch

import effect_cases as K
from oracle import ref_generator as G
from test_gpu_generator import TRAIN_KW, make_dataset, oracle_batch

pytestmark = pytest.mark.gpu
FILL = 0xA5
GAP = 256            # bytes between two pages of a packed buffer; they must stay untouched


@pytest.fixture(scope="module")
def CG():
    return importlib.import_module("retinanet-for-table-detection_amd.csv_generator")


@pytest.fixture(scope="module")
def T():
    return importlib.import_module("retinanet-for-table-detection_amd.model.transform")


def pack(pages, shift, fill_pages=True):
    """One device buffer of FILL with page i at a 256-byte aligned offset plus `shift` -> (buffer, offsets)."""
    offs, pos = [], GAP
    for p in pages:
        offs.append(pos + shift)
        pos = (pos + shift + p.size + GAP + 255) & ~255
    host = np.full(pos, FILL, np.uint8)
    if fill_pages:
        for p, o in zip(pages, offs):
            host[o:o + p.size] = p.reshape(-1)
    buf = torch.as_tensor(host).cuda()
    assert buf.data_ptr() % 256 == 0
    return buf, offs


def unpack(buf, pages, offs):
    """The pages of a packed buffer; everything between them must still be FILL."""
    host = buf.cpu().numpy()
    keep = np.ones(host.size, bool)
    out = []
    for p, o in zip(pages, offs):
        out.append(host[o:o + p.size].reshape(p.shape))
        keep[o:o + p.size] = False
    assert np.all(host[keep] == FILL), "a kernel wrote outside an output"
    return out


def run_device(pkg, handle, pages, params, flags, src_shift=0, dst_shift=0, in_place=False):
    """One call of rtn_visual_effect_u8 over the whole batch -> the outputs on the host."""
    n = len(pages)
    heights, widths, par, fl = K.batch_arrays(pages, params, flags)
    src, src_offs = pack(pages, src_shift)
    dst, dst_offs = (src, src_offs) if in_place else pack(pages, dst_shift, fill_pages=False)
    wsb = int(pkg.lib.rtn_visual_effect_workspace_bytes(n, heights.ctypes.data, widths.ctypes.data))
    ws = torch.full((wsb,), 0x5A, dtype=torch.uint8, device="cuda")         # whatever the workspace held must not matter
    sp = (C.c_void_p * n)(*[src.data_ptr() + o for o in src_offs])
    dp = (C.c_void_p * n)(*[dst.data_ptr() + o for o in dst_offs])
    handle.check(pkg.lib.rtn_visual_effect_u8(handle.raw, n, sp, heights.ctypes.data, widths.ctypes.data, par.ctypes.data,
                                              fl.ctypes.data, dp, ws.data_ptr(), wsb))
    torch.cuda.synchronize()
    if not in_place:
        assert all(np.array_equal(a, b) for a, b in zip(unpack(src, pages, src_offs), pages)), "an input changed"
    return unpack(dst, pages, dst_offs)


def assert_cases(got, where):
    for i, (name, _page, _params, _flags) in enumerate(K.cases()):
        want = K.oracle(i)
        assert np.array_equal(got[i], want), "%s, %s: %d bytes differ" % (where, name, int((got[i] != want).sum()))


def columns():
    cs = K.cases()
    return [c[1] for c in cs], [c[2] for c in cs], [c[3] for c in cs]


def test_every_case_in_one_batched_call_equals_the_oracle(pkg, handle):
    assert len(K.cases()) > 17 and len(set(c[1].shape for c in K.cases())) >= len(K.SHAPES)      # every shape, one call
    assert_cases(run_device(pkg, handle, *columns()), "aligned, out of place")


def test_in_place_equals_out_of_place(pkg, handle):
    assert_cases(run_device(pkg, handle, *columns(), in_place=True), "aligned, in place")
    assert_cases(run_device(pkg, handle, *columns(), src_shift=5, in_place=True), "unaligned, in place")


def test_pages_of_any_alignment(pkg, handle):
    assert_cases(run_device(pkg, handle, *columns(), src_shift=1, dst_shift=3), "both unaligned")
    assert_cases(run_device(pkg, handle, *columns(), src_shift=4, dst_shift=0), "source on a dword only")
    assert_cases(run_device(pkg, handle, *columns(), src_shift=0, dst_shift=8), "output on 8 bytes only")


def test_device_entry_rejects_bad_arguments(pkg, handle):
    page = K.random_page(6, 8, 1)
    heights, widths, par, fl = K.batch_arrays([page], [(1.1, 0.0, 0.0, 0.0)], [0])
    x = torch.as_tensor(page).cuda()
    y = torch.zeros_like(x)
    wsb = int(pkg.lib.rtn_visual_effect_workspace_bytes(1, heights.ctypes.data, widths.ctypes.data))
    assert wsb > 0 and wsb % 256 == 0
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda")
    sp, dp = (C.c_void_p * 1)(x.data_ptr()), (C.c_void_p * 1)(y.data_ptr())
    f = pkg.lib.rtn_visual_effect_u8
    args = (heights.ctypes.data, widths.ctypes.data, par.ctypes.data, fl.ctypes.data)
    assert f(handle.raw, 1, sp, *args, dp, ws.data_ptr(), wsb - 1) == -3 and b"workspace" in pkg.lib.rtn_last_error(handle.raw)
    assert f(handle.raw, 1, sp, *args, dp, ws.data_ptr() + 16, wsb) == -1 and b"aligned" in pkg.lib.rtn_last_error(handle.raw)
    assert f(handle.raw, 1, sp, *args, dp, None, wsb) == -1
    big = np.array([65501], np.int32)
    assert f(handle.raw, 1, sp, big.ctypes.data, *args[1:], dp, ws.data_ptr(), wsb) == -1 and b"65500" in pkg.lib.rtn_last_error(handle.raw)
    bad = np.array([1.0, np.nan, 0.0, 0.0])
    assert f(handle.raw, 1, sp, args[0], args[1], bad.ctypes.data, args[3], dp, ws.data_ptr(), wsb) == -1
    assert f(None, 1, sp, *args, dp, ws.data_ptr(), wsb) == -1
    assert f(handle.raw, 0, None, None, None, None, None, None, None, 0) == 0
    torch.cuda.synchronize()
    assert torch.all(y == 0)
    assert f(handle.raw, 1, sp, *args, dp, ws.data_ptr(), wsb) == 0
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), K.R.effect(page, (1.1, 0.0, 0.0, 0.0)))


def test_visual_effect_call_on_numpy_and_on_a_tensor(T):
    page = K.random_page(90, 120, 4)
    before = page.copy()
    for params in ((1.2, -0.1, 0.04, 0.9), (0.0, 0.0, 0.0, 1.0), (0.0, 0.3, 0.0, 0.0), (0, 0, 0, 0)):
        effect = T.VisualEffect(*params)
        want = K.R.effect(page, params)
        got = effect(page)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want) and np.array_equal(page, before)
        dev = effect(torch.as_tensor(page).cuda())
        assert dev.is_cuda and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), want)
    with pytest.raises(ValueError):
        T.VisualEffect(1, 0, 0, 0)(page.astype(np.float32))
    with pytest.raises(ValueError):
        T.VisualEffect(1, 0, 0, 0)(page[..., 0])
    np.random.seed(3)
    effect = next(T.random_visual_effect_generator())
    assert np.array_equal(effect(page), K.R.effect(page, effect.params()))


def test_adjust_functions_one_step_at_a_time(T):
    page = K.random_page(47, 33, 6)
    hsv = K.ramp_page()
    for v in (1.4, 0.0):                                                     # called on their own the steps run at 0 too
        assert np.array_equal(T.adjust_contrast(page, v), K.R.contrast(page, v))
        assert np.array_equal(T.adjust_brightness(page, v - 0.3), K.R.brightness(page, v - 0.3))
        for fn, ref, arg in ((T.adjust_hue, K.R.hue, v - 0.6), (T.adjust_saturation, K.R.saturation, v)):
            want = ref(hsv, arg)
            mine = hsv.copy()
            got = fn(mine, arg)
            assert got is mine and np.array_equal(mine, want)                # in place, as the reference
            dev = torch.as_tensor(hsv).cuda()
            assert fn(dev, arg) is dev and np.array_equal(dev.cpu().numpy(), want)
    dev = T.adjust_contrast(torch.as_tensor(page).cuda(), 0.7)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), K.R.contrast(page, 0.7))


RANGES = dict(contrast_range=(0.6, 1.4), brightness_range=(-0.2, 0.2), hue_range=(-0.3, 0.3), saturation_range=(0.5, 1.5))
GEN_KW = dict(batch_size=2, group_method="none", shuffle_groups=False, image_min_side=224, image_max_side=288, dtype=torch.float32)


def test_csv_generator_batch_with_effects_matches_oracle(tmp_path, CG, T):
    csvf, d, pages = make_dataset(tmp_path, n=2)
    random.seed(1)
    np.random.seed(5)
    order = ("contrast_range", "brightness_range", "hue_range", "saturation_range")
    want_params = [[np.random.uniform(*RANGES[k]) for k in order] for _ in range(2)]
    np.random.seed(5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gen = CG.CSVGenerator(csvf, d, {"table": 0}, transform_generator=T.random_transform_generator(prng=np.random.RandomState(21), **TRAIN_KW),
                              transform_parameters=T.TransformParameters(), visual_effect_generator=T.random_visual_effect_generator(**RANGES),
                              apply_visual_effect=True, **GEN_KW)
        assert len(gen) == 1 and gen.groups[0] == [0, 1]
        inputs, (reg, lab) = gen[0]
    prng = np.random.RandomState(21)
    tfs = [G.random_transform(prng, **TRAIN_KW) for _ in gen.groups[0]]
    names = [gen.image_data[i].name for i in gen.groups[0]]
    coloured = {n: K.R.effect(pages[n], p) for n, p in zip(names, want_params)}
    assert all((coloured[n] != pages[n]).any() for n in names)
    want_in, want_reg, want_lab, want_boxes = oracle_batch(gen, gen.groups[0], coloured, tfs, 224, 288)
    assert inputs.is_cuda and tuple(inputs.shape) == want_in.shape
    assert np.abs(inputs.cpu().numpy() - want_in).max() <= 1e-5              # the tolerance of test_csv_generator_batch_matches_oracle
    for a, b in zip(gen.last_annotations, want_boxes):
        assert np.array_equal(a["bboxes"], b)
    assert np.array_equal(reg.cpu().numpy(), want_reg) and np.array_equal(lab.cpu().numpy(), want_lab)
    # the group methods on their own: one page, and a group without a generator passes through
    page = torch.as_tensor(pages[names[0]]).cuda()
    np.random.seed(9)
    p = [np.random.uniform(*RANGES[k]) for k in order]
    np.random.seed(9)
    got, ann = gen.random_visual_effect_group_entry(page, {"bboxes": np.zeros((0, 4))})
    torch.cuda.synchronize()                                                 # the group methods queue on the generator's own stream
    assert np.array_equal(got.cpu().numpy(), K.R.effect(pages[names[0]], p)) and ann["bboxes"].shape == (0, 4)
    gen.visual_effect_generator = None
    assert gen.random_visual_effect_group([page], [ann])[0][0] is page
    gen.close()


class Counting:
    """An effect generator that counts how often it is advanced."""

    def __init__(self, inner):
        self.inner, self.n = inner, 0

    def __iter__(self):
        return self

    def __next__(self):
        self.n += 1
        return next(self.inner)


def test_default_generator_is_unchanged_and_never_advances_the_effects(tmp_path, CG, T):
    csvf, d, _pages = make_dataset(tmp_path, n=2)
    batches = []
    counting = Counting(T.random_visual_effect_generator(**RANGES))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for extra in ({}, {"visual_effect_generator": counting}):
            random.seed(1)
            gen = CG.CSVGenerator(csvf, d, {"table": 0}, transform_generator=T.random_transform_generator(prng=np.random.RandomState(21), **TRAIN_KW),
                                  transform_parameters=T.TransformParameters(), **extra, **GEN_KW)
            assert gen.apply_visual_effect is False and gen.visual_effect_generator is extra.get("visual_effect_generator")
            inputs, (reg, lab) = gen[0]
            batches.append((inputs.clone(), reg.clone(), lab.clone()))
            gen.close()
    assert counting.n == 0
    for a, b in zip(*batches):
        assert torch.equal(a, b)
