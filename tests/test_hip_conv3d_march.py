"""The 3-D layers' march along depth (conv3d_split_march_kernel in conv2d_split.hip): a workgroup owns a pixel tile and a run of
output planes, stages every input plane once and feeds it to every depth tap it serves.  Every output is the same sum in the same
order as on conv2d_split_kernel / conv2d_split_persist_kernel, so the results are compared bit by bit.

Experiments library: MVD_C3_MARCH = 1 (the built-in rule), 2, 3 and 64 (runs of that many planes, forced at any shape) against 0.
MVD_C2_KSPLIT=1 holds for both sides: the default plan splits the reduction of grids this small over several workgroups and adds the
halves afterwards, which is another order of the same sum, and the march is planned for an unsplit reduction only.
Product library: shapes at which the rule takes the march, against torch's float64 convolution (the bar of
test_hip_conv2d_split.py: 3e-6 of the output scale)."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (stride, Cin, Cout, B, D, h, w, with_skip)
CASES = {
    "s1_ragged": (1, 16, 16, 1, 5, 17, 33, False),     # ragged tiles, D no multiple of any run, halo planes of real data
    "s1_one_plane": (1, 16, 16, 1, 1, 16, 16, False),  # both neighbours outside the volume
    "s1_two_planes": (1, 16, 16, 1, 2, 16, 16, False),
    "s1_batch_skip": (1, 8, 16, 2, 4, 20, 18, True),   # runs do not cross batch elements; one channel chunk (resident weights)
    "s1_three_chunks": (1, 24, 16, 1, 3, 16, 40, False),
    "s2_skip": (2, 8, 16, 1, 6, 18, 34, True),
    "s2_two_tiles": (2, 16, 32, 2, 4, 34, 18, False),  # Cout 32: two 16-channel tiles
    "s1_ragged_nonfinite": (1, 16, 16, 1, 5, 17, 33, False),  # NaN in plane 2 (a halo plane of the runs of 2 and of 3), +inf in the last
}
# product library: the rule (C3_MARCH_TD, C3_MARCH_MIN_WGS in conv2d_split.hip) takes the march for stride-2 layers with at least
# 256 (tile, run) pairs at runs of 16 planes, and for no stride-1 layer (conv2 measured slower on it), so there is no stride-1
# product case: stride 1 is covered by the experiments-library cases above.  A thin volume of many planes reaches 256 pairs
# below 40 MB: 2033 output planes of 17 x 3 (two ragged tiles) = 2 x 128 runs, x 26.5 MB
PRODUCT = {
    "s2_8_16_march": (2, 8, 16, 1, 4066, 34, 6, True),
}
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _exp_or_skip():
    from robustmvd_amd import _lib as L
    if not os.path.exists(L.EXP_LIB_PATH):
        pytest.skip("the experiments library is not built (make -C robustmvd_amd/csrc exp)")
    return L


def _case(name, dev, table=CASES):
    if name not in _cache:
        stride, cin, cout, B, D, h, w, with_skip = table[name]
        g = torch.Generator().manual_seed(stride * 1000 + cin * 10 + cout + D + h)
        x = torch.randn(B, D, h, w, cin, generator=g) * (torch.rand(cin, generator=g) * 3)
        if name.endswith("nonfinite"):
            x[0, 2, 5, 7, 3] = float("nan")
            x[0, D - 1, 16, 32, 9] = float("inf")
        wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (cin * 27)) ** 0.5
        scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
        skip = torch.randn(B, D // stride, h // stride, w // stride, cout, generator=g).to(dev) if with_skip else None
        _cache[name] = (x.to(dev), wt.to(dev), scale.to(dev), shift.to(dev), stride - 1, skip)
    return _cache[name]


def _run(case):
    from robustmvd_amd import ops
    x, wt, scale, shift, mode, skip = case
    packed = ops.pack_conv3d_weights_igemm(wt, mode)
    return ops.conv3d_bn_relu_igemm(x, ops.absmax(x), packed, wt.shape[1], wt.shape[0], scale, shift, mode, relu=True, skip=skip,
                                    return_absmax=True)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_march_equals_the_chunked_depth_taps(name, dev, monkeypatch):
    L = _exp_or_skip()
    case = _case(name, dev)
    monkeypatch.setenv("MVD_C2_KSPLIT", "1")
    monkeypatch.setenv("MVD_C3_MARCH", "0")
    with L.use_experiments_library():
        ref, ref_amax = _run(case)
    if name.endswith("nonfinite"):  # the ReLU turns a NaN sum into 0 (fmaxf), +inf stays: what matters is that both forms agree
        assert bool(torch.isnan(case[0]).any()) and bool(torch.isinf(case[0]).any())
    for v in ("1", "2", "3", "64"):
        monkeypatch.setenv("MVD_C3_MARCH", v)
        with L.use_experiments_library():
            got, amax = _run(case)
        assert _same_bits(got, ref), f"MVD_C3_MARCH={v}"
        assert float(amax) == float(ref_amax), f"MVD_C3_MARCH={v}"


@pytest.mark.parametrize("name", list(PRODUCT))
def test_product_march_vs_float64(name, dev):
    case = _case(name, dev, PRODUCT)
    x, wt, scale, shift, mode, skip = case
    got, amax = _run(case)
    ref = F.conv3d(x.permute(0, 4, 1, 2, 3).double().cpu(), wt.double().cpu(), stride=mode + 1, padding=1)
    ref = F.relu(ref * scale.double().cpu().view(1, -1, 1, 1, 1) + shift.double().cpu().view(1, -1, 1, 1, 1))
    if skip is not None:
        ref = ref + skip.permute(0, 4, 1, 2, 3).double().cpu()
    out_scale = float(ref.abs().max())
    err = float((got.permute(0, 4, 1, 2, 3).double().cpu() - ref).abs().max())
    print(f"{name}: max error {err:.3e}, bound {3e-6 * out_scale:.3e}")
    assert err <= 3e-6 * out_scale, (err, out_scale)
    assert float(amax) == float(got.abs().max())


def test_costregnet_march_equal_bits(dev, monkeypatch):
    """CostRegNet.forward_channels_last at (1, 16, 16, 24, 32) through the experiments library: conv1, conv2, conv3 and conv5 on the
    march with runs of 2 planes (conv3 and conv5 with their channel tile narrowed to 16), against no march"""
    L = _exp_or_skip()
    import robustmvd_amd as R
    torch.manual_seed(11)
    net = R.CostRegNet().eval().to(dev)
    x = torch.rand(1, 16, 16, 24, 32, device=dev)
    monkeypatch.setenv("MVD_C2_KSPLIT", "1")
    out = {}
    for v in ("0", "2"):
        monkeypatch.setenv("MVD_C3_MARCH", v)
        with L.use_experiments_library():
            out[v] = net.forward_channels_last(x)
    assert _same_bits(out["2"], out["0"])
