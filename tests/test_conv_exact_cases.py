"""Host check of the exact-operand cases (tests/conv_exact.py): every case the GPU modules compare kernels with must meet the three
conditions that make an equality on it meaningful - every partial sum below 2^24, the final rounding exercised (>= 5 % of a compared
tensor not representable before it, >= 2 % exact ties), not degenerate after a ReLU / in a mask - and its reference must change
when the final rounding is replaced by truncation, so that the case can tell a truncating store from round-to-nearest-even.
A case that misses a condition is a bug of the test, found here without a GPU."""
import pytest
import torch

import conv_exact as X


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_case_meets_the_conditions(name):
    c = X.case(name)
    for row in c.stats():
        print("%-32s %-6s %-5s needs rounding %5.1f %%  ties %5.1f %%  worst sum bound %d" % ((name,) + row[:2] + (100 * row[2], 100 * row[3], row[4])))
    c.check()


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("mode", X.EPI_MODES)
@pytest.mark.parametrize("form", sorted(X.EPI_FORMS))
def test_register_epilogue_form_meets_the_conditions(form, mode, relu):
    """The operands of the register-epilogue tests of tests/test_gpu_conv.py, in every mode (a few more than those tests launch)."""
    for step, stage in X.epi_stages(form, mode, relu):
        stage.check()
    if "mask" in mode:
        for x, other, act, y, bound in X.epi_exact_operands(form)[2]:
            X.check_mask(act)


def test_the_instruments_tell_the_roundings_apart():
    """bf16: 257 is a tie (256 | 258), 259 a tie that goes up, 258.5 is above the midpoint; e4m3: 17 is a tie (16 | 18), 19 goes up."""
    x = torch.tensor([257.0, 259.0, 258.5, 256.0, -257.0, 513.0, 514.0, 0.0], dtype=torch.float64)
    assert X.bf16(x).tolist() == [256.0, 260.0, 258.0, 256.0, -256.0, 512.0, 512.0, 0.0]
    assert X.trunc_bf16(x).tolist() == [256.0, 258.0, 258.0, 256.0, -256.0, 512.0, 512.0, 0.0]
    assert X.rounding_shares(x, "bf16") == (6 / 8, 4 / 8)       # 514 lies between 512 and 516
    y = torch.tensor([17.0, 19.0, 16.0, -19.0, 500.0, 17.5, 0.0, 21.0], dtype=torch.float64)
    assert X.e4m3(y).tolist() == [16.0, 20.0, 16.0, -20.0, 448.0, 18.0, 0.0, 20.0]
    assert X.trunc_e4m3(y).tolist() == [16.0, 18.0, 16.0, -18.0, 448.0, 16.0, 0.0, 20.0]
    assert X.rounding_shares(y, "e4m3") == (5 / 8, 4 / 8)


def test_the_pool_rule_is_first_maximum_in_scan_order():
    x = torch.zeros(1, 4, 4, 1, dtype=torch.float64)       # H1 = 4: pad 0 / 1; window (0, 0) = rows 0..2, window (1, 1) = rows 2..4
    x[0, 1, 2, 0] = 5.0
    x[0, 2, 1, 0] = 5.0
    pooled, idx = X.pool_tfsame_idx(x)
    assert pooled[0, :, :, 0].tolist() == [[5.0, 5.0], [5.0, 0.0]]
    assert idx[0, :, :, 0].tolist() == [[5, 3], [1, 0]]    # (0,0): taps 5 and 7 tie, 5 first; (1,1): its four in-image taps are 0: tap 0
    x[0, 3, 3, 0] = 5.0
    assert X.pool_tfsame_idx(x)[1][0, 1, 1, 0] == 4
