"""The 8 -> 1 conv3d kernel (`prob`; also the last layer of cvp_mvsnet's and vis_mvsnet's regularisers) marches
plane-stationary: one input plane per step feeds the three output planes it touches.  Checked against float64 on the CPU
and, bit for bit, against the output-stationary ring kernel it replaced, which the experiments library keeps under
MVD_K4_PROB_RING.  The volumes cover a partial last chunk of 16 planes, a single plane / row / voxel, chunks of one and two
planes, and 62-column tile edges on both sides (w = 62, 63, 64, 125)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ATOL = RTOL = 1e-4  # tests/test_hip_shapes.py

VOLUMES = [(2, 19, 5, 63), (1, 1, 1, 1), (1, 2, 3, 125), (1, 33, 9, 62), (1, 16, 4, 64)]
SCALE, SHIFT = 1.7, -0.3  # the folded BatchNorm affine of the one output channel


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(B, D, h, w):
    """inputs (x and skip channel-last, weight (1,8,3,3,3)) and the float64 convolution, computed once per volume"""
    g = torch.Generator().manual_seed(B * 1000003 + D * 10007 + h * 101 + w)
    x = torch.randn(B, D, h, w, 8, generator=g)
    wgt = torch.randn(1, 8, 3, 3, 3, generator=g) * 0.1
    skip = torch.randn(B, D, h, w, 1, generator=g)
    conv = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3).double(), wgt.double(), padding=1)  # (B,1,D,h,w)
    return x, wgt, skip, conv.permute(0, 2, 3, 4, 1).contiguous()


def run(vol, relu, with_skip, dev):
    from robustmvd_amd import _lib as L
    from robustmvd_amd import ops
    x, wgt, skip, _ = case(*vol)
    packed, cin, cout = ops.pack_conv3d_weights(wgt.to(dev), L.CONV3D_STRIDE1)
    assert (cin, cout) == (8, 1)
    sc = torch.full((1,), SCALE, device=dev)
    sh = torch.full((1,), SHIFT, device=dev)
    return ops.conv3d_bn_relu(x.to(dev), packed, 8, 1, sc, sh, L.CONV3D_STRIDE1, relu=relu,
                              skip=skip.to(dev) if with_skip else None)


@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("vol", VOLUMES)
def test_prob_matches_float64(vol, relu, with_skip, dev):
    _, _, skip, conv = case(*vol)
    want = conv * SCALE + SHIFT
    if relu:
        want = want.clamp_min(0.0)
    if with_skip:
        want = want + skip.double()
    got = run(vol, relu, with_skip, dev)
    assert got.shape == want.shape
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("vol", VOLUMES)
def test_prob_is_bit_identical_to_the_ring_kernel(vol, relu, with_skip, dev, monkeypatch):
    """every chain of the plane-stationary kernel takes its terms in the ring kernel's order: the same bits"""
    from robustmvd_amd import _lib as L
    if not os.path.exists(L.EXP_LIB_PATH):
        pytest.skip("the experiments library is not built (make -C robustmvd_amd/csrc exp)")
    monkeypatch.setenv("MVD_K4_PROB_RING", "1")
    got = run(vol, relu, with_skip, dev)  # product library: ignores the environment
    with L.use_experiments_library():
        ring = run(vol, relu, with_skip, dev)
    assert torch.equal(got, ring)
    assert torch.equal(got.view(torch.int32), ring.view(torch.int32))  # the signs of zeros too
