"""The persistent, software-pipelined form of the split-operand implicit GEMM (conv2d_split_persist_kernel: a workgroup walks
several tiles with the next patch prefetched), the narrowed channel tile of under-filled 3-D grids, and the border-only zeroing of
K3's staging map.

Product library: layers with more tiles than the persistent grid holds, and 3-D layers whose channel tile the plan narrows, against torch's float64 convolution on the CPU with the
bar of test_hip_conv2d_split.py (3e-6 of the output scale).  Experiments library: the forms selected by MVD_C2_PERSIST / MVD_C2_BN
are bit-identical to one tile per workgroup, because every output is the same sum in the same order."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# The product library runs the persistent form where it measured faster (C2_PERSIST_WGS in conv2d_split.hip): the 3 x 3 layers
# with 8-channel chunks and a 16-channel tile, on at most 256 CUs x 4 = 1024 workgroups.  The cases marked `loops` have more tiles
# of 16 x 16 output pixels than that, so that a workgroup of the product library walks more than one tile.  The other kinds run one
# tile per workgroup there, and every case runs persistent on three workgroups in the experiments library below.
# 2-D: (k, stride, cin, cout, B, H, W); 3-D: (stride, cin, cout, D, h, w, with_skip)
C2 = {
    "3x3_16_16": (3, 1, 16, 16, 4, 200, 264),         # ragged in both directions; 4 * 13 * 17 = 884 tiles
    "3x3_16_16_loops": (3, 1, 16, 16, 5, 200, 264),   # 1105 tiles
    "3x3_32_32": (3, 1, 32, 32, 5, 100, 136),         # 32-channel chunks, 9 K steps; 315 tiles
    "5x5s2_8_16": (5, 2, 8, 16, 4, 400, 520),         # 7 K steps; 884 tiles
    "tiny2d": (3, 1, 16, 16, 1, 37, 75),
}
C3 = {
    "s1_16_16": (1, 16, 16, 24, 40, 56, False),        # 288 tiles
    "s1_16_16_loops": (1, 16, 16, 90, 40, 56, False),  # 1080 tiles
    "s2_8_16_skip": (2, 8, 16, 32, 48, 80, True),
    "s2_8_16_loops": (2, 8, 16, 520, 34, 66, True),    # 260 planes of 2 x 3 tiles = 1560
    "s1_64_64": (1, 64, 64, 6, 24, 36, False),         # 36 tiles of 64 channels: too few to narrow (K is split); the tiles of the test below
    # stride-1 grids of 128 .. 511 tiles at the packing rule's channel tile: the product library narrows the tile to 16 channels
    "s1_64_64_narrowed": (1, 64, 64, 16, 48, 64, False),  # 192 tiles of 64 channels -> 768 of 16
    "s1_32_32_narrowed": (1, 32, 32, 16, 48, 64, False),  # 192 tiles of 32 channels -> 384 of 16
    "s1_64_48_narrowed": (1, 64, 48, 12, 40, 56, True),   # 144 tiles of 64 (48 used) -> 432 of 16: ncp 64 -> 48, with skip
    "tiny3d": (1, 32, 32, 3, 17, 16, False),
}
_cache = {}


def _case2d(name, dev):
    """inputs (on the device, the input as an NHWC slice of a wider buffer), packed weights and the float64 reference: built once"""
    if name not in _cache:
        from robustmvd_amd import ops
        k, stride, cin, cout, B, H, W = C2[name]
        g = torch.Generator().manual_seed(k * 1000 + cin + cout + H)
        x = torch.randn(B, cin, H, W, generator=g) * torch.rand(1, cin, 1, 1, generator=g) * 4
        wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        bias = torch.randn(cout, generator=g) * 0.1
        want = F.leaky_relu(F.conv2d(x.double(), wt.double(), bias.double(), stride=stride, padding=k // 2), 0.2)
        buf = torch.full((B, H, W, cin + 4), 7.0, device=dev)  # the input is a channel slice of a wider buffer; all tensors < 40 MB
        buf[..., 4:4 + cin] = x.permute(0, 2, 3, 1).to(dev)
        _cache[name] = (buf[..., 4:4 + cin], ops.absmax(x.to(dev)), (wt.to(dev), bias.to(dev), stride), want)
    return _cache[name]


def _run2d(case, dev):
    from robustmvd_amd import ops
    xin, xam, (wt, bias, stride), want = case
    wts = ops.pack_conv2d_weights_split(wt, bias, stride=stride)
    B, cout, Ho, Wo = want.shape
    obuf = torch.full((B, Ho, Wo, cout + 8), -3.0, device=dev)
    amax = torch.zeros(1, device=dev)
    got = ops.conv2d_split(xin, xam, wts, act=1, slope=0.2, out=obuf[..., 4:4 + cout], out_absmax=amax)
    return got, amax, obuf


def _case3d(name, dev):
    if name not in _cache:
        stride, cin, cout, D, h, w, with_skip = C3[name]
        g = torch.Generator().manual_seed(stride * 100 + cin + cout + D)
        x = torch.randn(1, cin, D, h, w, generator=g) * torch.rand(1, cin, 1, 1, 1, generator=g) * 3
        wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (cin * 27)) ** 0.5
        scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
        ref = F.conv3d(x.double(), wt.double(), stride=stride, padding=1)
        ref = F.relu(ref * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1))
        skip = torch.randn(ref.shape, generator=g) if with_skip else None
        if with_skip:
            ref = ref + skip.double()
        sk = skip.permute(0, 2, 3, 4, 1).contiguous().to(dev) if with_skip else None
        _cache[name] = (x.permute(0, 2, 3, 4, 1).contiguous().to(dev), wt.to(dev), scale.to(dev), shift.to(dev), stride - 1, sk, ref)
    return _cache[name]


def _run3d(case):
    from robustmvd_amd import ops
    xc, wt, scale, shift, mode, sk, _ = case
    packed = ops.pack_conv3d_weights_igemm(wt, mode)
    return ops.conv3d_bn_relu_igemm(xc, ops.absmax(xc), packed, wt.shape[1], wt.shape[0], scale, shift, mode, relu=True, skip=sk,
                                    return_absmax=True)


@pytest.mark.parametrize("name", [n for n in C2 if n != "tiny2d"])
def test_persistent_conv2d_vs_float64(name, dev):
    case = _case2d(name, dev)
    got, amax, obuf = _run2d(case, dev)
    want = case[3]
    scale = float(want.abs().max())
    err = float((got.permute(0, 3, 1, 2).double().cpu() - want).abs().max())
    print(f"{name}: max error {err:.3e}, bound {3e-6 * scale:.3e}")
    assert err <= 3e-6 * scale, (err, scale)
    assert float(amax) == float(got.abs().max())
    cout = want.shape[1]  # the neighbouring channels of the destination buffer are untouched
    assert float(obuf[..., :4].min()) == -3.0 and float(obuf[..., :4].max()) == -3.0
    assert float(obuf[..., 4 + cout:].min()) == -3.0 and float(obuf[..., 4 + cout:].max()) == -3.0


@pytest.mark.parametrize("name", [n for n in C3 if n != "tiny3d"])
def test_persistent_conv3d_vs_float64(name, dev):
    case = _case3d(name, dev)
    got, amax = _run3d(case)
    ref = case[-1]
    scale = float(ref.abs().max())
    err = float((got.permute(0, 4, 1, 2, 3).double().cpu() - ref).abs().max())
    print(f"{name}: max error {err:.3e}, bound {3e-6 * scale:.3e}")
    assert err <= 3e-6 * scale, (err, scale)
    assert float(amax) == float(got.abs().max())


def _exp_or_skip():
    from robustmvd_amd import _lib as L
    if not os.path.exists(L.EXP_LIB_PATH):
        pytest.skip("the experiments library is not built (make -C robustmvd_amd/csrc exp)")
    return L


@pytest.mark.parametrize("name", list(C2) + list(C3))
def test_persistent_forms_equal_one_tile_per_workgroup(name, dev, monkeypatch):
    """MVD_C2_PERSIST = 0 (one tile per workgroup), 1 (the built-in rule) and 3 (three workgroups walk every tile: they cross plane,
    batch and cout-block boundaries and get unequal tile counts) and the product library: the same bits."""
    L = _exp_or_skip()
    two_d = name in C2
    case = _case2d(name, dev) if two_d else _case3d(name, dev)
    run = (lambda: _run2d(case, dev)[:2]) if two_d else (lambda: _run3d(case))
    ref, ref_amax = run()  # product library: ignores the environment
    for v in ("0", "1", "3"):
        monkeypatch.setenv("MVD_C2_PERSIST", v)
        with L.use_experiments_library():
            got, amax = run()
        assert torch.equal(got, ref), f"MVD_C2_PERSIST={v}"
        assert float(amax) == float(ref_amax)


@pytest.mark.parametrize("bn", ["16", "32"])
@pytest.mark.parametrize("persist", ["0", "1", "3"])
def test_narrowed_channel_tile_equals_the_wide_one(bn, persist, dev, monkeypatch):
    """the 64 -> 64 3-D layer on 16- and 32-channel tiles: the same packed fragments, not a single sum changes.  All forms with the
    reduction in one piece (MVD_C2_KSPLIT=1): the default plan splits K in two for the 36 tiles of the 64-channel form and adds the
    halves afterwards, which is another order of the same sum (that plan is held to the float64 bound above)."""
    L = _exp_or_skip()
    case = _case3d("s1_64_64", dev)
    monkeypatch.setenv("MVD_C2_KSPLIT", "1")
    monkeypatch.setenv("MVD_C2_BN", "64")
    monkeypatch.setenv("MVD_C2_PERSIST", "0")
    with L.use_experiments_library():
        ref, ref_amax = _run3d(case)
    monkeypatch.setenv("MVD_C2_BN", bn)
    monkeypatch.setenv("MVD_C2_PERSIST", persist)
    with L.use_experiments_library():
        got, amax = _run3d(case)
    assert torch.equal(got, ref) and float(amax) == float(ref_amax)
    ref64 = case[-1]
    assert float((got.permute(0, 4, 1, 2, 3).double().cpu() - ref64).abs().max()) <= 3e-6 * float(ref64.abs().max())


def test_border_zeroing_of_the_staging_map(dev):
    """LAYOUT_NHWC_BORDER into a buffer full of NaN: the border comes out exactly 0 (mvd_zero_border_nhwc_f32), the interior is the
    LAYOUT_NHWC result"""
    import robustmvd_amd as R
    from robustmvd_amd import _lib as L
    from robustmvd_amd import ops
    torch.manual_seed(7)
    net = R.blocks.FeatureNet().eval().to(dev)
    x = torch.randn(2, 3, 64, 128, device=dev)
    want = net.forward_layout(x, L.LAYOUT_NHWC)
    assert tuple(want.shape) == (2, 16, 32, 32)
    buf = torch.full((2, 19, 35, 32), float("nan"), device=dev)
    got = net.forward_layout(x, L.LAYOUT_NHWC_BORDER, out=buf)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(got[:, 1:17, 1:33], want)
    border = got.clone()
    border[:, 1:17, 1:33] = 0
    assert torch.equal(border, torch.zeros_like(border))
    fresh = net.forward_layout(x, L.LAYOUT_NHWC_BORDER)
    assert torch.equal(fresh, got)
    # the entry alone, odd sizes: the interior is left as it was
    b2 = torch.full((3, 8, 13, 8), float("nan"), device=dev)
    ops.zero_border_nhwc(b2)
    assert bool(torch.isnan(b2[:, 1:6, 1:11]).all())
    b2[:, 1:6, 1:11] = 0
    assert torch.equal(b2, torch.zeros_like(b2))
