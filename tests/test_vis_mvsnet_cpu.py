"""vis_mvsnet without a GPU: registry entry, the reference's state-dict keys, the two weight-packing identities of its regulariser,
the adapter's normalisation, and the conditions of the fixtures tests/golden/g17_vis_mvsnet*.npz, which make_golden_vis.py records
from the reference's own VisMvsnet (case a in g17_vis_mvsnet.npz, case b in g17_vis_mvsnet_b.npz, the stage-3 volume of a small
third case in g17_vis_mvsnet_c.npz).  Also the inputs and float64 references that the GPU tests of the three kernels share."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import gen_common as gc

CASES = {"a": "g17_vis_mvsnet", "b": "g17_vis_mvsnet_b", "c": "g17_vis_mvsnet_c"}


def vis_state_dict(shapes, seed, gain_final, gain_feat, gain_head):
    """The weights of the g17 fixtures, rebuilt from their seed and three gains (only those are stored).  shapes: {key: shape} of the
    model's state dict; key i in sorted order draws gen_common.rng_array(seed + i, shape) =: N and becomes
      convolution weights     N * sqrt(1 / (3 fan_in)) * gain: the variance of torch's default initialisation; gain_final on the six
                              8 -> 1 `final_conv` of the stages (peaked score volumes), gain_feat on FeatExt's three `final_conv_*`,
                              gain_head on the UncertNets' `head_convs` (fusion weights away from 1 / V)
      BatchNorm weight        1 + 0.1 N         BatchNorm bias           0.05 N
      running_mean            0.1 N             running_var              0.5 + U(0, 1) (default_rng(seed + i).random)
      num_batches_tracked     left out (the module's own zero).
    Returns {key: float32 ndarray}."""
    out = {}
    for i, key in enumerate(sorted(shapes)):
        shape = tuple(shapes[key])
        if key.endswith("num_batches_tracked"):
            continue
        n = gc.rng_array(seed + i, shape)
        if key.endswith("running_var"):
            v = 0.5 + np.random.default_rng(seed + i).random(shape)
        elif key.endswith("running_mean"):
            v = 0.1 * n
        elif key.endswith("weight") and len(shape) == 1:
            v = 1.0 + 0.1 * n
        elif key.endswith("bias"):
            v = 0.05 * n
        else:
            gain = gain_final if key.startswith("stage") and ".final_conv." in key else gain_feat if key.startswith("feat_ext.final_conv_") else \
                gain_head if ".uncert_net.head_convs." in key else 1.0
            v = n * np.sqrt(1.0 / (3.0 * np.prod(shape[1:]))) * gain
        out[key] = v.astype(np.float32)
    return out


def golden_state_dict(g, model):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = vis_state_dict(shapes, int(g["weights_seed"]), float(g["gain_final"]), float(g["gain_feat"]), float(g["gain_head"]))
    full = model.state_dict()
    for k, v in sd.items():
        full[k] = torch.from_numpy(v)
    return full


MEAN = np.array([0.485, 0.456, 0.406], np.float32).reshape(3, 1, 1)
STD = np.array([0.229, 0.224, 0.225], np.float32).reshape(3, 1, 1)


def normalise_numpy(image_u8):
    """(..., 3, H, W) uint8 RGB -> the model's input in numpy: / 255, ImageNet mean / std, channels flipped to BGR; float32."""
    x = (image_u8.astype(np.float32) / np.float32(255.0) - MEAN) / STD
    return np.ascontiguousarray(np.flip(x, -3))


def window_jump_mask(p, window=2.0, eps=1e-3, mass=1e-5):
    """Condition 3.  p (B,D,h,w) float64 probabilities -> (index (B,h,w), jump (B,h,w) bool): the pixels where some bin i sits within
    eps of the window's edge, | |i - index| - window | < eps, AND carries mass p_i > `mass`: there, and only there, a rounding of the
    index can move more than `mass` into or out of the windowed sum.  (Not "index near an integer": a saturated softmax sits on an
    integer while its edge bins are empty.)"""
    D = p.shape[1]
    i = np.arange(D, dtype=np.float64).reshape(1, D, 1, 1)
    index = (p * i).sum(1)
    jump = ((np.abs(np.abs(i - index[:, None]) - window) < eps) & (p > mass)).any(1)
    return index, jump


# ------------------------------------------------------------------------------------------------ registry and state dict
def test_registered_by_name_and_list_models_unchanged():
    import robustmvd_amd as R
    assert R.has_model("vis_mvsnet")
    assert R.list_models() == ["mvsnet_train", "robust_mvd", "robust_mvd_5M"]  # unchanged: registered by name only
    assert not R.has_model("vis_mvsnet", trainable_only=True)
    model = R.create_model("vis_mvsnet", num_gpus=0)
    assert model.name == "vis_mvsnet" and callable(model.run) and not model.training and isinstance(model, R.VisMvsnet)


def test_state_dict_keys_and_shapes_are_the_references():
    import robustmvd_amd as R
    g = load_golden(CASES["a"])
    sd = R.VisMvsnet(num_sampling_steps=192).state_dict()
    assert len(sd) == 367
    want = {str(k): tuple(int(x) for x in s) for k, s in zip(g["state_dict_keys"], g["state_dict_shapes"])}
    got = {k: tuple(v.shape) + (0,) * (5 - v.dim()) for k, v in sd.items()}  # shapes are stored padded with zeros to 5 entries
    assert got == want


def test_strict_load_round_trips(tmp_path):
    import robustmvd_amd as R
    g = load_golden(CASES["a"])
    m = R.VisMvsnet()
    full = golden_state_dict(g, m)
    m.load_state_dict(full, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, full[k]), k
    path = tmp_path / "vis.pt"
    torch.save({"model_state_dict": {"module." + k: v for k, v in full.items()}}, path)
    m2 = R.create_model("vis_mvsnet", weights=str(path), num_gpus=0)  # the registry entry honours a weights file
    for k, v in m2.state_dict().items():
        assert torch.equal(v, full[k]), k


# ------------------------------------------------------------------------------------------------ packing identities
def test_center_tap_weight_is_the_1x1x1_stride_2_convolution():
    from robustmvd_amd.vis_mvsnet import center_tap_weight
    torch.manual_seed(3)
    x = torch.randn(2, 8, 6, 4, 10, dtype=torch.float64)
    w1 = torch.randn(16, 8, 1, 1, 1, dtype=torch.float64)
    w3 = center_tap_weight(w1)
    assert tuple(w3.shape) == (16, 8, 3, 3, 3) and int((w3 != 0).sum()) == 16 * 8
    want = torch.nn.functional.conv3d(x, w1, stride=2)
    got = torch.nn.functional.conv3d(x, w3, stride=2, padding=1)
    assert got.shape == want.shape and torch.equal(got, want)


def test_split_post_concat_is_the_convolution_of_the_concatenation():
    from robustmvd_amd.vis_mvsnet import split_concat_weight
    torch.manual_seed(4)
    a, b = torch.randn(2, 8, 4, 6, 6, dtype=torch.float64), torch.randn(2, 8, 4, 6, 6, dtype=torch.float64)
    w = torch.randn(8, 16, 3, 3, 3, dtype=torch.float64)
    wa, wb = split_concat_weight(w)
    want = torch.nn.functional.conv3d(torch.cat([a, b], 1), w, padding=1)
    got = torch.nn.functional.conv3d(a, wa, padding=1) + torch.nn.functional.conv3d(b, wb, padding=1)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)  # float64: only the order of the sum differs


def test_engine_regulariser_module_is_the_references_on_torch():
    """Reg3d.forward (the torch restatement the packing is derived from) on the fixture's cost volume reproduces the reference's Reg and
    RegFuse outputs: the module tree computes what the reference's does (fp32 CPU against fp32 CPU: 1e-5)."""
    import robustmvd_amd as R
    g = load_golden(CASES["a"])
    m = R.VisMvsnet().eval()
    m.load_state_dict(golden_state_dict(g, m), strict=True)
    cost = torch.from_numpy(g["cost_1"])
    with torch.no_grad():
        pair = m.stage1.reg_pair(m.stage1.reg(cost))
        fuse = m.stage1.reg_fuse(cost)
    np.testing.assert_allclose(pair.numpy(), g["reg_pair_1"], atol=1e-5 * np.abs(g["reg_pair_1"]).max(), rtol=1e-5)
    np.testing.assert_allclose(fuse.numpy(), g["reg_fuse_1"], atol=1e-5 * np.abs(g["reg_fuse_1"]).max(), rtol=1e-5)


# ------------------------------------------------------------------------------------------------ adapter
def test_normalise_image_against_numpy():
    from robustmvd_amd.vis_mvsnet import normalise_image
    rng = np.random.default_rng(5)
    im = rng.uniform(0, 255.999, (2, 3, 9, 11)).astype(np.float32)
    im[0, :, 0, 0] = (0.0, 255.0, 254.99998)
    got = normalise_image(torch.from_numpy(im)).numpy()
    want = normalise_numpy(im.astype(np.uint8))  # astype truncates
    assert got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)
    # channel 0 of the result is the BLUE channel: normalised with blue's mean and std
    np.testing.assert_allclose(got[:, 0], (np.trunc(im[:, 2]) / 255 - 0.406) / 0.225, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ the fixtures' conditions
@pytest.mark.parametrize("case", ["a", "b"])
def test_fixture_conditions(case):
    from robustmvd_amd.vis_mvsnet import DEPTH_NUMS, S_SCALES
    g = load_golden(CASES[case])
    H, W = g["images"].shape[-2:]
    assert g["depth_3"].shape[1:] == (H // S_SCALES[2], W // S_SCALES[2]) and g["depth_1"].shape[1:] == (H // S_SCALES[0], W // S_SCALES[0])
    assert 0 <= g["index_f64"].min() and g["index_f64"].max() <= DEPTH_NUMS[2] - 1
    pct = lambda x: float(np.percentile(x, 95) - np.percentile(x, 5))
    # 1: sensitivity
    assert pct(g["uncertainty"]) >= 0.2
    assert pct(g["pair_entropy_3"]) >= 1.0
    u = g["pair_heads_3"][:, 0].astype(np.float64)  # (V, B, h, w): head 0 of every pair
    wgt = np.exp(-u[0]) / np.exp(-u).sum(0)
    assert pct(wgt) >= 0.1
    # 2: conditioning
    assert float(g["ref_f32_vs_f64_rel"]) <= 1e-4
    # 3: window jumps
    jump = np.unpackbits(g["jump_3"])[:g["index_f64"].size].reshape(g["index_f64"].shape).astype(bool)
    assert jump.mean() <= 0.01 and (g["jump_fraction"] <= 0.01).all()
    assert abs(jump.mean() - g["jump_fraction"][2]) < 1e-12
    for k in g.files:
        assert g[k].dtype.kind in "fiubUS", k  # arrays, seeds and names only


# ------------------------------------------------------------------ inputs and references of the GPU tests of the two stage kernels
SA_SHAPES = [(2, 16, 5, 7), (1, 64, 3, 130), (1, 1, 4, 4), (1, 33, 9, 9)]


def sa_inputs(B, D, h, w, seed=43):
    """scores whose scale varies per pixel from 0.01 (flat: entropy log D) to 30 (saturated: probabilities below the entropy's clamp),
    a scalar and a per-pixel start, and the intervals."""
    rng = np.random.default_rng(seed)
    scale = np.geomspace(0.01, 30.0, h * w).reshape(1, 1, h, w)
    score = rng.standard_normal((B, D, h, w)) * rng.permuted(scale, axis=3)
    start = 1.0 + rng.random(B)
    start_pp = 1.0 + rng.random((B, h, w))
    interval = 0.05 + 0.1 * rng.random(B)
    return tuple(a.astype(np.float32) for a in (score, start, start_pp, interval))


def sa_reference(score, start, interval, window):
    """float64 torch, the reference's formulas (blocks/utils.py:51-68) -> depth, entropy, prob_map, keep (condition 3's complement)"""
    c = torch.from_numpy(score).double()
    B, D = c.shape[:2]
    p = torch.softmax(c, 1)
    i = torch.arange(D, dtype=torch.float64).view(1, D, 1, 1)
    out = (p * i).sum(1, keepdim=True)
    st = torch.from_numpy(start).double().reshape(B, -1, 1)
    st = st.reshape(B, 1, 1) if st.shape[1] == 1 else st.reshape(B, *c.shape[2:])
    depth = out[:, 0] * torch.from_numpy(interval).double().view(B, 1, 1) + st
    ent = (-p * p.clamp(1e-9, 1.0).log()).sum(1)
    prob = (p * ((i - out).abs() <= window).double()).sum(1)
    _, jump = window_jump_mask(p.numpy(), window)
    return depth.numpy(), ent.numpy(), prob.numpy(), ~jump


@pytest.mark.parametrize("shape", SA_SHAPES)
def test_sa_inputs_are_flat_and_saturated_and_keep_99_percent(shape):
    from robustmvd_amd.vis_mvsnet import WINDOW  # the window the model's final regression uses
    B, D, h, w = shape
    score, start, start_pp, interval = sa_inputs(B, D, h, w)
    _, ent, prob, keep = sa_reference(score, start, interval, WINDOW)
    assert keep.mean() >= 0.99
    if D > 1:
        assert ent.max() > 0.95 * np.log(D) and ent.min() < 1e-3  # some pixels flat, some saturated
        p = torch.softmax(torch.from_numpy(score).double(), 1)
        assert float(((p < 1e-9) & (p > 0)).double().mean()) > 0.01  # the clamp of the entropy is exercised


FUSE_SHAPES = [(2, 4, 5, 7, 8, 3), (1, 3, 9, 13, 8, 1), (1, 2, 4, 4, 16, 4)]


def fuse_inputs(B, D, h, w, C, V, seed=41):
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal((B, D, h, w, C)).astype(np.float32) for _ in range(V)]
    us = [rng.uniform(-3.0, 3.0, (B, h, w)).astype(np.float32) for _ in range(V)]
    return xs, us


def fuse_reference(xs, us):
    wts = [np.exp(-u.astype(np.float64))[:, None, :, :, None] for u in us]
    return sum(x.astype(np.float64) * wt for x, wt in zip(xs, wts)) / sum(wts)


def groupcorr_reference(feats, Ms, depth, groups, grid_clamp=1.1):
    """float64 torch on the CPU, the reference's formulas (homography_warping + interpolate + groupwise_correlation, blocks/utils.py:
    71-89,154-186) for the sweep's [R|t] form: feats [key, src_0 ..] (B,C,h,w), Ms V x (B,3,4), depth (B,D) shared planes.  Pixel
    positions (x + 0.5, y + 0.5, 1); warped position (X / Z, Y / Z) of (X,Y,Z) = R pos d + t; normalised grid pos / size * 2 - 1 clamped
    to +-grid_clamp; grid_sample(bilinear, zeros, align_corners=False); correlation summed per channel group.
    Returns V volumes (B,D,h,w,groups) float64."""
    key = feats[0].double()
    B, C, h, w = key.shape
    D = depth.shape[1]
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64) + 0.5, torch.arange(w, dtype=torch.float64) + 0.5, indexing="ij")
    pos = torch.stack((xs, ys, torch.ones_like(xs)), 0).reshape(1, 3, -1)
    out = []
    for src, M in zip(feats[1:], Ms):
        M = M.double()
        p = (M[:, :, :3] @ pos)[:, None] * depth.double()[:, :, None, None] + M[:, None, :, 3:4]  # (B,D,3,hw)
        grid = torch.stack((p[:, :, 0] / p[:, :, 2] / w, p[:, :, 1] / p[:, :, 2] / h), -1) * 2 - 1
        grid = grid.clamp(-grid_clamp, grid_clamp).reshape(B * D, h, w, 2)
        warped = torch.nn.functional.grid_sample(src.double()[:, None].expand(B, D, C, h, w).reshape(B * D, C, h, w), grid, mode="bilinear",
                                                 padding_mode="zeros", align_corners=False).reshape(B, D, groups, C // groups, h, w)
        out.append((key.reshape(B, 1, groups, C // groups, h, w) * warped).sum(3).permute(0, 1, 3, 4, 2).contiguous())
    return out
