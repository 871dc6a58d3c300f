"""The premise of the quarter forms of rtn_bottleneck64_fwd (Engine.skip_unread_c2): in inference nothing reads C2, the output of the
64-channel stage's last block, except stage 3's first block, and that block reads it through two 1x1 / stride-2 convolutions - at
pixels whose row and column are both even.  Here every other pixel of C2 is NaN in the fp32 oracle: the network's outputs must keep
their bits and stay finite.  A graph change that adds a reader of C2 (a P2 level, a 3x3 first convolution in stage 3) fails this."""
import importlib

import numpy as np
import pytest
import torch

from oracle.ref_net import RefNet, STAGE_BLOCKS, block_char


class PoisonedC2(RefNet):
    """RefNet whose C2 holds NaN wherever the row or the column is odd."""

    def conv(self, x, name, *args, **kw):
        y = super().conv(x, name, *args, **kw)
        last = "res2%s_branch2c" % block_char(self.backbone, 0, STAGE_BLOCKS[self.backbone][0] - 1)
        if name == last:                                   # NCHW
            y = y.clone()
            y[:, :, 1::2, :] = float("nan")
            y[:, :, :, 1::2] = float("nan")
            self.poisoned = int(torch.isnan(y).sum())
        return y


@pytest.mark.parametrize("canvas", [(70, 102), (75, 109)])       # C2 is 18 x 26 and 19 x 28: an even and an odd number of rows
def test_outputs_do_not_depend_on_the_odd_pixels_of_c2(pkg, canvas):
    Wt = importlib.import_module(pkg.__name__ + ".weights")
    state = Wt.init_state("resnet50", 1, 9, seed=0, randomize_bn=True, cls_bias=0.0, tame=True)
    g = torch.Generator().manual_seed(canvas[0])
    x = (torch.rand(2, canvas[0], canvas[1], 3, generator=g) * 2 - 1).numpy()
    reg, cls = RefNet(state, dtype=torch.float32).forward(x)
    net = PoisonedC2(state, dtype=torch.float32)
    preg, pcls = net.forward(x)
    assert net.poisoned > 0
    assert bool(torch.isfinite(preg).all()) and bool(torch.isfinite(pcls).all())
    assert np.array_equal(reg.numpy(), preg.numpy()) and np.array_equal(cls.numpy(), pcls.numpy())
