"""The plane-marching split-operand kernel (conv0_split_kernel, csrc/conv3d_split.hip) issues five MFMAs where its first
version issued six (the lo-term taps of two planes share one MFMA's column halves, which change places between steps), and a
workgroup marches one or more segments of planes: even depth groups on the ordinary grid, or the persistent runs that the
experiments library starts.  Neither changes the order of any accumulation chain:
the outputs and max |y| are compared bit for bit with the six-MFMA schedule that the experiments library keeps under
MVD_CONV0_LEGACY=1, the persistent runs (MVD_CONV0_SLOTS=n, any n) with the ordinary grid of the same library, and two volumes
with a float64 convolution at the gate of tests/test_hip_f16.py."""
import copy
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# smallest; D = 2; D = 3 (every column half changes place once with live data); crosses td = 32 with partial tiles in y and x
# and B = 2; an exact tile
VOLUMES = [(1, 1, 1, 1), (1, 2, 3, 31), (1, 3, 5, 33), (2, 35, 6, 65), (1, 9, 4, 32)]
CHANNELS = [(32, 8), (32, 16), (16, 8), (16, 16)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def exp_lib():
    from robustmvd_amd import _lib as L
    if not os.path.exists(L.EXP_LIB_PATH):
        pytest.skip("the experiments library is not built (make -C robustmvd_amd/csrc exp)")
    return L.use_experiments_library


@functools.lru_cache(maxsize=None)
def case(vol, cin, cout):
    """x channel-last (B, D, h, w, cin) with channel magnitudes over three decades, the weight and the folded BatchNorm affine"""
    B, D, h, w = vol
    g = torch.Generator().manual_seed(B * 1000003 + D * 10007 + h * 101 + w + 7 * cin + cout)
    x = torch.randn(B, D, h, w, cin, generator=g) * torch.tensor([1e-2, 1.0, 20.0])[torch.randint(0, 3, (cin,), generator=g)]
    wgt = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (cin * 27)) ** 0.5
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    return x, wgt, scale, shift


def run(x, wgt, scale, shift, relu, dev, x_absmax=None):
    """-> (y of the plain variant, y and max |y| of the max |y| variant); packs with whichever library is current"""
    from robustmvd_amd import ops
    packed = ops.pack_conv3d_weights_split(wgt.to(dev))
    args = (x.to(dev), packed, scale.to(dev), shift.to(dev))
    y = ops.conv3d_bn_relu_split(*args, relu=relu, x_absmax=x_absmax)
    y2, amax = ops.conv3d_bn_relu_split(*args, relu=relu, x_absmax=x_absmax, return_absmax=True)
    return y, y2, amax


def assert_same_bits(got, want):
    for a, b in zip(got, want):
        assert a.shape == b.shape
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # NaN payloads and the signs of zeros too


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("vol", VOLUMES)
def test_bit_identical_to_the_six_mfma_schedule(vol, cin, cout, relu, dev, exp_lib, monkeypatch):
    x, wgt, scale, shift = case(vol, cin, cout)
    monkeypatch.setenv("MVD_CONV0_LEGACY", "1")
    got = run(x, wgt, scale, shift, relu, dev)  # product library: ignores the environment
    with exp_lib():
        want = run(x, wgt, scale, shift, relu, dev)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert_same_bits(got, want)
    assert torch.equal(got[0], got[1])  # the max |y| variant stores what the plain one stores
    assert float(got[2]) == float(got[0].abs().max())


def test_bit_identical_with_a_loose_x_absmax(dev, exp_lib, monkeypatch):
    """any upper bound of max |x| is a valid scale: 4 x the true maximum shifts every operand by two bits in both schedules"""
    x, wgt, scale, shift = case((2, 35, 6, 65), 32, 8)
    loose = (x.abs().max() * 4.0).reshape(1).to(dev)
    monkeypatch.setenv("MVD_CONV0_LEGACY", "1")
    got = run(x, wgt, scale, shift, True, dev, x_absmax=loose)
    with exp_lib():
        want = run(x, wgt, scale, shift, True, dev, x_absmax=loose)
    assert_same_bits(got, want)


@pytest.mark.parametrize("cin,cout", [(32, 8), (16, 16)])
def test_bit_identical_with_nan_and_inf(cin, cout, dev, exp_lib, monkeypatch):
    """a NaN at a tile corner, +inf in a halo column and -inf in the last plane reach the same outputs with the same bits: no
    chain has gained a term (a zero-weight column would turn an inf into a NaN)"""
    vol = (2, 35, 6, 65)
    x, wgt, scale, shift = case(vol, cin, cout)
    x = x.clone()
    x[0, 3, 4, 32, 5] = float("nan")    # first voxel of tile (1, 1)
    x[1, 20, 2, 31, 0] = float("inf")   # the last column of tile column 0: halo of tile column 1
    x[0, 34, 1, 64, 9] = float("-inf")  # last plane, the one column of the partial tile
    monkeypatch.setenv("MVD_CONV0_LEGACY", "1")
    got = run(x, wgt, scale, shift, False, dev)
    with exp_lib():
        want = run(x, wgt, scale, shift, False, dev)
    assert not torch.isfinite(got[0]).all() and torch.isfinite(got[0]).any()
    assert_same_bits(got, want)


@pytest.mark.parametrize("cin,cout", [(32, 8), (16, 16)])
@pytest.mark.parametrize("vol", [(2, 35, 6, 65), (1, 3, 5, 33)])
def test_matches_float64(vol, cin, cout, dev):
    """the gate of tests/test_hip_f16.py for this kernel: against a float64 convolution of the same fp32 data the largest error
    is at most 1.5 x that of the fp32-MFMA kernel"""
    from robustmvd_amd import _lib as L
    from robustmvd_amd import ops
    x, wgt, _, _ = case(vol, cin, cout)
    one, zero = torch.ones(cout), torch.zeros(cout)
    ref = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3).double(), wgt.double(), padding=1).permute(0, 2, 3, 4, 1)
    got = run(x, wgt, one, zero, False, dev)[0].cpu().double()
    w32, _, _ = ops.pack_conv3d_weights(wgt.to(dev), L.CONV3D_STRIDE1)
    base = ops.conv3d_bn_relu(x.to(dev), w32, cin, cout, one.to(dev), zero.to(dev), L.CONV3D_STRIDE1, relu=False).cpu().double()
    err_s, err_f = float((got - ref).abs().max()), float((base - ref).abs().max())
    print(f"{vol} {cin} -> {cout}: split {err_s:.3e}  fp32-MFMA {err_f:.3e}  max |y| {float(ref.abs().max()):.3e}")
    assert err_s <= 1.5 * err_f, (err_s, err_f)


# (1, 7, 9, 70): 3 x 3 tiles of 7 planes; shares of 21, 12 - 13 and 7 - 8 planes cross tile and XCD boundaries and leave segments
# of one plane.  (2, 5, 4, 40) with 16 output channels: shares cross batch and cout-block boundaries (the fragments reload)
@pytest.mark.parametrize("slots", [3, 5, 8])
@pytest.mark.parametrize("vol,cin,cout", [((1, 7, 9, 70), 32, 8), ((2, 5, 4, 40), 32, 16), ((2, 5, 4, 40), 16, 16)])
def test_persistent_runs_are_bit_identical_to_the_ordinary_grid(vol, cin, cout, slots, dev, exp_lib, monkeypatch):
    x, wgt, scale, shift = case(vol, cin, cout)
    with exp_lib():
        monkeypatch.setenv("MVD_CONV0_SLOTS", "0")
        want = run(x, wgt, scale, shift, True, dev)
        monkeypatch.setenv("MVD_CONV0_SLOTS", str(slots))
        got = run(x, wgt, scale, shift, True, dev)
    assert_same_bits(got, want)


def test_more_than_one_round_of_workgroups(dev, exp_lib, monkeypatch):
    """The smallest volume with more than one round of workgroups on the device at hand: one 4 x 32 tile and D = 8 (2 CUs + 1) - 7
    planes.  At 8 planes per workgroup (the rule under 2048 workgroups) that is 2 CUs + 1 workgroups, one more than are
    resident.  The product library against the six-MFMA schedule on the same grid, and against the persistent runs of 2 CUs
    workgroups (8 - 9 planes each) that the experiments library starts."""
    slots = 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    vol = (1, 8 * slots + 1, 4, 32)
    x, wgt, scale, shift = case(vol, 32, 8)
    got = run(x, wgt, scale, shift, True, dev)
    monkeypatch.setenv("MVD_CONV0_SLOTS", str(slots))
    with exp_lib():
        persistent = run(x, wgt, scale, shift, True, dev)
    monkeypatch.setenv("MVD_CONV0_LEGACY", "1")
    monkeypatch.setenv("MVD_CONV0_SLOTS", "0")
    monkeypatch.setenv("MVD_CONV0_TD", "8")
    with exp_lib():
        want = run(x, wgt, scale, shift, True, dev)
    assert_same_bits(got, want)
    assert_same_bits(persistent, want)


def test_costregnet_forward_is_bit_identical(dev, exp_lib, monkeypatch):
    """MVSNet's regulariser on its default path (split-operand layers), D = 8, 16 x 40: the same cost volume bits"""
    import robustmvd_amd as R
    torch.manual_seed(3)
    net = R.MVSNet(num_sampling_steps=8).eval().cost_regularization
    for m in net.modules():  # BatchNorm statistics that are not the identity
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0.0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    legacy = copy.deepcopy(net).to(dev)  # its own packed weights, packed by the library that runs it
    net = net.to(dev)
    x = torch.randn(1, 8, 16, 40, 32, device=dev).abs()
    got = net.forward_channels_last(x)
    monkeypatch.setenv("MVD_CONV0_LEGACY", "1")
    with exp_lib():
        want = legacy.forward_channels_last(x)
    assert got.shape == (1, 8, 16, 40)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
