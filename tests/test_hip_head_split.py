"""FeatureNet's conv0 -> conv1 launch with conv1 on the fp16 matrix instruction (mvd_conv2d_head_split_f32): the fp32 launch's
bound against float64 (2e-6 of max |want|) on ragged tiles, images smaller than a tile and a second tile column one and two
pixels wide; over image magnitudes; per tile where a tile's neighbour is 1e7 times larger; next to inf / NaN pixels; the
per-tile max |y| by-product; the weights packed once per model; FeatureNet with the head on and off."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_common as gc
from test_oracle_golden import featurenet_shapes

pytestmark = pytest.mark.gpu
BOUND = 2e-6  # the project's bound for this layer pair (test_conv2d_head_matches_float64_and_two_launches)
SHAPES = [(2, 64, 128), (1, 37, 75), (3, 8, 64), (1, 5, 3), (1, 9, 65), (1, 17, 130)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def weights(mag=1.0):
    """the layer pair of test_conv2d_head_matches_float64_and_two_launches; the shifts follow the image's magnitude"""
    g = torch.Generator(device="cpu").manual_seed(11)
    w0, w1 = torch.randn(8, 3, 3, 3, generator=g) * 0.3, torch.randn(8, 8, 3, 3, generator=g) * 0.2
    s0, b0, s1, b1 = (torch.randn(8, generator=g) for _ in range(4))
    return w0, w1, s0, b0 * mag, s1, b1 * mag


def reference(img, mag=1.0):
    w0, w1, s0, b0, s1, b1 = (t.double() for t in weights(mag))
    ref = F.relu(F.conv2d(img.double(), w0, padding=1) * s0.view(1, -1, 1, 1) + b0.view(1, -1, 1, 1))
    ref = F.relu(F.conv2d(ref, w1, padding=1) * s1.view(1, -1, 1, 1) + b1.view(1, -1, 1, 1))
    return ref.permute(0, 2, 3, 1)


def run(img, dev, mag=1.0, split=True, return_absmax=False):
    from robustmvd_amd import ops
    w0, w1, s0, b0, s1, b1 = (t.to(dev) for t in weights(mag))
    w0p = w0.permute(2, 3, 1, 0).contiguous()
    if split:
        return ops.conv2d_head_split(img.to(dev), w0p, s0, b0, ops.pack_conv2d_head_weights_split(w1), s1, b1, return_absmax=return_absmax)
    return ops.conv2d_head(img.to(dev), w0p, s0, b0, w1.permute(2, 3, 1, 0).contiguous(), s1, b1, return_absmax=return_absmax)


@functools.lru_cache(maxsize=None)
def image(shape):
    g = torch.Generator(device="cpu").manual_seed(11)
    return torch.randn(shape[0], 3, shape[1], shape[2], generator=g)


@pytest.mark.parametrize("shape", SHAPES)
def test_head_split_matches_float64(shape, dev):
    img = image(shape)
    want = reference(img)
    got = run(img, dev)
    assert tuple(got.shape) == (shape[0], shape[1], shape[2], 8)
    got2, amax = run(img, dev, return_absmax=True)  # per-tile maxima, reduced: exactly max |y|
    assert torch.equal(got2, got) and float(amax) == float(got.abs().max())
    scale = float(want.abs().max())
    err = float((got.double().cpu() - want).abs().max())
    err32 = float((run(img, dev, split=False).double().cpu() - want).abs().max())
    print(f"{shape}: error {err / scale:.3g} of max |want|, the fp32 launch {err32 / scale:.3g}: ratio {err / max(err32, 1e-300):.2f}")
    assert err <= BOUND * scale


@pytest.mark.parametrize("mag", [1e-30, 1.0, 1e4])
def test_head_split_over_magnitudes(mag, dev):
    """the per-tile and per-channel powers of two carry the range: the same bound at every uniform magnitude"""
    img = image((1, 20, 70)) * mag
    want = reference(img, mag)
    got = run(img, dev, mag)
    assert float((got.double().cpu() - want).abs().max()) <= BOUND * float(want.abs().max())


def tile_errors(got, want):
    """per 8 x 64 tile: max |got - want| over the tile / max |want| over the tile grown by two pixels"""
    _, H, W, _ = want.shape
    out = []
    for r in range(0, H, 8):
        for c in range(0, W, 64):
            e = float((got[:, r:r + 8, c:c + 64] - want[:, r:r + 8, c:c + 64]).abs().max())
            out.append(e / float(want[:, max(r - 2, 0):r + 10, max(c - 2, 0):c + 66].abs().max()))
    return out


def test_head_split_scales_per_tile(dev):
    """columns < 64 of magnitude 1e-4, columns >= 64 of 1e3: every tile meets the bound relative to its own surroundings (the
    fp32 launch measured on the same image: see the printed figures)"""
    img = image((1, 16, 192)).clone()
    img[..., :64] *= 1e-4
    img[..., 64:] *= 1e3
    w0, w1, s0, b0, s1, b1 = weights()
    want = reference(img, 0.0)  # no shifts: the small tile's outputs stay small
    got = run(img, dev, 0.0).double().cpu()
    got32 = run(img, dev, 0.0, split=False).double().cpu()
    e, e32 = tile_errors(got, want), tile_errors(got32, want)
    print("per-tile error / max |want| nearby: split " + " ".join(f"{v:.3g}" for v in e) + "; fp32 " + " ".join(f"{v:.3g}" for v in e32))
    assert max(e32) <= BOUND
    assert max(e) <= BOUND


def test_head_split_non_finite_pixels_stay_local(dev):
    """one inf and one NaN pixel: outputs outside their 5 x 5 neighbourhoods are finite and within the bound of the reference
    computed without them (the K pad slot reads an always-zero pixel, never a neighbour)"""
    img = image((1, 24, 140)).clone()
    clean = img.clone()
    spots = [(0, 5, 63, float("inf")), (2, 17, 100, float("nan"))]
    far = torch.ones(24, 140, dtype=torch.bool)
    for ch, r, c, v in spots:
        img[0, ch, r, c] = v
        clean[0, ch, r, c] = 0.0
        far[r - 2:r + 3, c - 2:c + 3] = False
    want = reference(clean)[0][far]
    got = run(img, dev)[0].cpu()[far]
    assert bool(torch.isfinite(got).all())
    assert float((got.double() - want).abs().max()) <= BOUND * float(want.abs().max())


def featurenet(dev):
    import robustmvd_amd as R
    net = R.blocks.FeatureNet().eval()
    full = net.state_dict()
    for k, v in gc.fill_state_dict(featurenet_shapes(), 3).items():
        full[k] = torch.from_numpy(v)
    net.load_state_dict(full)
    return net.to(dev)


def test_featurenet_head_split_on_and_off(dev):
    from robustmvd_amd import ops
    net = featurenet(dev)
    assert net.head_split and net.fused_head and net.split_layers
    x = torch.from_numpy(gc.rng_array(5, (2, 3, 32, 48), 0.5)).to(dev)
    on = net(x)
    pk = net._packed
    assert pk is not None and pk.head_w1 is not None
    ptr = pk.head_w1.data_ptr()
    on2 = net(x)
    assert net._packed is pk and pk.head_w1.data_ptr() == ptr  # packed once, reused
    assert torch.equal(on, on2)
    c1 = ops.conv2d_head_split(x, *pk.head[:3], pk.head_w1, *pk.head[4:])
    c1_32 = ops.conv2d_head(x, *pk.head)
    assert float((c1 - c1_32).abs().max()) <= BOUND * float(c1_32.abs().max())
    net.head_split = False
    off = net(x)
    assert net._packed is pk
    np.testing.assert_allclose(on.cpu().numpy(), off.cpu().numpy(), atol=1e-4, rtol=1e-4)  # tests/test_hip_parity.py, g9
