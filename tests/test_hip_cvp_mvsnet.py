"""cvp_mvsnet on the GPU: the two kernels it adds (mvd_sweep_reduce_nhwc_f32, mvd_softmax_regress_pp_f32), its regulariser alone and
the whole model against the reference's own CVPMVSNet (tests/golden/g16_cvp_mvsnet*.npz, made by tests/golden/make_golden_cvp.py)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import gen_common as gc
from sweep_reduce_cases import sweep_inputs
from test_cvp_mvsnet_cpu import CASES, PP_SHAPES, golden_state_dict, pp_confidence_mask, pp_inputs, pp_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


# ---------------------------------------------------------------------------------------------------------- sweep_reduce_nhwc
def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def bordered(x):
    """(B,C,h,w) -> zero-bordered channel-last (B,h+3,w+3,C) with the map at (1,1)"""
    B, C, h, w = x.shape
    buf = torch.zeros((B, h + 3, w + 3, C), dtype=torch.float32, device=x.device)
    buf[:, 1:h + 1, 1:w + 1, :] = x.permute(0, 2, 3, 1)
    return buf


def border_crossings(Ms, shared, h, w):
    """what the shared planes do, accumulated over views, batch, planes and pixels: a sample in front of the camera leaves the map
    through each of its four borders (the kernel clamps at -1 and w / h), one stays inside, and one lies behind the camera"""
    dev = shared.device
    B = shared.shape[0]
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    pix = torch.stack((xs, ys, torch.ones_like(xs)), 0).reshape(1, 3, -1)
    seen = dict(left=False, right=False, top=False, bottom=False, inside=False, behind=False)
    for M in Ms:
        p = (M[:, :, :3] @ pix)[:, :, None, :] * shared[:, None, :, None] + M[:, :, 3].reshape(B, 3, 1, 1)
        z = p[:, 2]
        x, y = p[:, 0] / z * (w / (w - 1)) - 0.5, p[:, 1] / z * (h / (h - 1)) - 0.5  # the kernel's sample index
        front = z > 0
        for name, cond in (("left", x < -1), ("right", x > w), ("top", y < -1), ("bottom", y > h),
                           ("inside", (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1))):
            seen[name] |= bool((cond & front).any())
        seen["behind"] |= bool((z < 0).any())
    return seen


# (1, 16, 19, 9, 13, 2): more planes than one workgroup's chunk of 8, and not a multiple of it (grid.y = 3 with a tail of 3)
@pytest.mark.parametrize("shape", [(2, 16, 8, 12, 20, 2), (1, 16, 3, 9, 13, 1), (1, 64, 5, 8, 8, 3), (1, 16, 19, 9, 13, 2)])
def test_sweep_reduce_nhwc_is_sweep_reduce_permuted(shape, dev):
    """bit for bit, both variance modes, shared and per-pixel depth"""
    from robustmvd_amd import _lib as L, ops, sweep_modes as SM
    B, C, D, h, w, V = shape
    feats, Ms, shared, per_pixel = sweep_inputs(B, C, h, w, D, V, 7, dev)
    key, srcs = nhwc(feats[0]), [bordered(f) for f in feats[1:]]
    for mode in (L.REDUCE_VARIANCE, L.REDUCE_VARIANCE_KEYSQ):
        for depth in (shared, per_pixel):
            want = SM.sweep_reduce_inference(feats[0], feats[1:], Ms, depth, mode)
            got = ops.sweep_reduce_nhwc(key, srcs, Ms, depth, mode)
            assert tuple(got.shape) == (B, D, h, w, C)
            assert torch.equal(got, want.permute(0, 2, 3, 4, 1))
            assert torch.isfinite(got).all()
    assert all(border_crossings(Ms, shared, h, w).values())


@pytest.mark.parametrize("name", ["pp", "pl"])
def test_sweep_reduce_nhwc_cvp_golden(name, dev):
    """g11's proj_cost fixtures (the reference's own function, with its aliasing) at the project's atol = rtol = 1e-4"""
    from robustmvd_amd import _lib as L, ops, sweep_modes as SM
    g = load_golden("g11_sweep_modes")
    ref, srcs = T(g["cvp_ref"], dev), [T(g["cvp_src0"], dev), T(g["cvp_src1"], dev)]
    ref_in, src_in, ref_ex, src_ex = (T(g[k], dev) for k in ("cvp_ref_in", "cvp_src_in", "cvp_ref_ex", "cvp_src_ex"))
    Ms = [SM._cvp_transform(ref_in, src_in[:, v], ref_ex, src_ex[:, v]) for v in range(2)]
    got = ops.sweep_reduce_nhwc(nhwc(ref), [bordered(s) for s in srcs], Ms, T(g[f"cvp_hyp_{name}"], dev), L.REDUCE_VARIANCE_KEYSQ)
    np.testing.assert_allclose(got.permute(0, 4, 1, 2, 3).cpu().numpy(), g[f"cvp_{name}_cost"], atol=1e-4, rtol=1e-4)


def test_sweep_reduce_nhwc_rejects_group_correlation(dev):
    from robustmvd_amd import _lib as L, ops
    B, C, D, h, w, V = 1, 16, 3, 9, 13, 1
    feats, Ms, shared, _ = sweep_inputs(B, C, h, w, D, V, 7, dev)
    out = torch.empty((B, D, h, w, C), device=dev)
    with pytest.raises(RuntimeError, match=r"status 1"):  # MVD_ERR_INVALID_ARG
        ops.call("mvd_sweep_reduce_nhwc_f32", dev, nhwc(feats[0]), [bordered(feats[1])], Ms, shared, 0, 0.0, 1.0, 1.0, -0.5,
                 L.REDUCE_GROUPCORR, B, C, D, h, w, V, out)
    with pytest.raises(ValueError):
        ops.sweep_reduce_nhwc(nhwc(feats[0]), [bordered(feats[1])], Ms, shared, L.REDUCE_GROUPCORR)


# ---------------------------------------------------------------------------------------------------------- softmax_regress_pp
@pytest.mark.parametrize("shape", PP_SHAPES)
def test_softmax_regress_pp_vs_float64(shape, dev):
    from robustmvd_amd import ops
    B, D, h, w = shape
    cost, hyp = pp_inputs(B, D, h, w)
    want_d, want_c, index = pp_reference(cost, hyp)
    depth, conf = ops.softmax_regress_pp(T(cost, dev), T(hyp, dev))
    np.testing.assert_allclose(depth.cpu().numpy(), want_d, atol=1e-5, rtol=1e-5)
    keep = pp_confidence_mask(index, D)
    np.testing.assert_allclose(conf.cpu().numpy()[keep], want_c[keep], atol=1e-5, rtol=0)
    depth2, none = ops.softmax_regress_pp(T(cost, dev), T(hyp, dev), with_confidence=False)  # conf_out = NULL
    assert none is None and torch.equal(depth2, depth)


@pytest.mark.parametrize("shape", PP_SHAPES)
def test_softmax_regress_pp_with_shared_hypotheses_is_k5(shape, dev):
    from robustmvd_amd import ops
    B, D, h, w = shape
    cost, hyp = pp_inputs(B, D, h, w)
    shared = T(hyp[:, :, 0, 0], dev)
    depth, conf = ops.softmax_regress_pp(T(cost, dev), shared[:, :, None, None].expand(B, D, h, w).contiguous())
    k5_depth, k5_conf = ops.softmax_regress(T(cost, dev), shared)
    np.testing.assert_allclose(depth.cpu().numpy(), k5_depth.cpu().numpy(), atol=1e-6, rtol=1e-6)
    keep = pp_confidence_mask(pp_reference(cost, hyp)[2], D)
    np.testing.assert_allclose(conf.cpu().numpy()[keep], k5_conf.cpu().numpy()[keep], atol=1e-5, rtol=0)


# ---------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def model(dev):
    import robustmvd_amd as R
    m = R.CVPMVSNet().eval()
    m.load_state_dict(golden_state_dict(load_golden(CASES["a"]), m), strict=True)
    return R.add_run_function(m.to(dev))


def fresh_model(dev):
    import robustmvd_amd as R
    m = R.CVPMVSNet().eval()
    m.load_state_dict(golden_state_dict(load_golden(CASES["a"]), m), strict=True)
    return m.to(dev)


def golden_inputs(g, dev):
    images = [T(im, dev).float() / torch.full((1,), 255.0, device=dev) for im in g["images"]]
    return dict(images=images, poses=[T(p, dev) for p in g["poses"]], intrinsics=[T(k, dev) for k in g["intrinsics"]], keyview_idx=0,
                depth_range=(g["depth_range"][0], g["depth_range"][1]))


REG_ATOL, REG_RTOL = 2e-4, 1e-3  # the project's gate for the same kind of stack (g5)


@pytest.mark.parametrize("case,level", [("a", 4), ("a", 3), ("c", 0)])
def test_regulariser_alone(case, level, model, dev):
    """the reference's own cost volumes through the eleven layers: the coarse level of case a (48 planes on 4 x 6), its level 3, and
    a level-0 volume (8 planes at full resolution: case c, 32 x 64, the largest whose volume a committed file can hold; case a's
    level 0, 64 x 96, is compared in test_whole_model_vs_reference)"""
    g = load_golden(CASES[case])
    with torch.no_grad():
        got = model.cost_reg_refine(T(g[f"cost_{level}"], dev))
    np.testing.assert_allclose(got.cpu().numpy(), g[f"reg_{level}"], atol=REG_ATOL, rtol=REG_RTOL)


@pytest.mark.parametrize("case", ["a", "b"])
def test_whole_model_vs_reference(case, model, dev, monkeypatch):
    g = load_golden(CASES[case])
    regs, reg = [], model.cost_reg_refine.forward_channels_last
    monkeypatch.setattr(model.cost_reg_refine, "forward_channels_last", lambda x: regs.append(reg(x)) or regs[-1])
    with torch.no_grad():
        pred, aux = model(**golden_inputs(g, dev))
    n, _, H, W = g["images"].shape[1:]
    # all five regulariser outputs, coarse first, each fed by the model's own cost volume of that level
    assert len(regs) == 5
    for got, level in zip(regs, range(4, -1, -1)):
        np.testing.assert_allclose(got.cpu().numpy(), g[f"reg_{level}"], atol=REG_ATOL, rtol=REG_RTOL, err_msg=f"regulariser output, level {level}")
    assert tuple(pred["depth"].shape) == (n, 1, H, W) and tuple(pred["depth_uncertainty"].shape) == (n, 1, H, W)
    assert len(aux["depths_all"]) == 5
    rels = [float(np.max(np.abs(aux["depths_all"][l].cpu().numpy() - g[f"depth_{l}"]) / np.abs(g[f"depth_{l}"]))) for l in range(5)]
    unc = pred["depth_uncertainty"][:, 0].cpu().numpy()
    keep = np.abs(g["index_f64"] - np.round(g["index_f64"])) > 1e-3
    print(f"case {case}: max relative depth error per level (finest first) {rels}; max uncertainty error "
          f"{np.max(np.abs(unc - g['uncertainty'])[keep]):.3e}; excluded {1 - keep.mean():.4f}; reference f32 vs f64 {float(g['ref_f32_vs_f64_rel']):.2e}")
    assert keep.mean() >= 0.99
    for l in range(4, -1, -1):  # coarse first: the first level that is off is the one to look at
        np.testing.assert_allclose(aux["depths_all"][l].cpu().numpy(), g[f"depth_{l}"], rtol=1e-3, atol=0, err_msg=f"level {l}")
    assert torch.equal(pred["depth"][:, 0], aux["depths_all"][0])
    np.testing.assert_allclose(unc[keep], g["uncertainty"][keep], atol=2e-3, rtol=0)


def test_run_numpy_unbatched(model, dev):
    """batch element 0 of case b (64 x 64: the adapter leaves a multiple of 64 as it is) as raw 0 .. 255 images through run()"""
    g = load_golden(CASES["b"])
    pred, aux = model.run(images=[im[0].astype(np.float32) for im in g["images"]], keyview_idx=0, poses=[p[0] for p in g["poses"]],
                          intrinsics=[k[0] for k in g["intrinsics"]], depth_range=(np.float32(425.0), np.float32(935.0)))
    assert isinstance(pred["depth"], np.ndarray) and pred["depth"].shape == (1, 64, 64) and pred["depth_uncertainty"].shape == (1, 64, 64)
    assert [d.shape for d in aux["depths_all"]] == [(64 >> l, 64 >> l) for l in range(5)]
    np.testing.assert_allclose(pred["depth"][0], g["depth_0"][0], rtol=1e-3, atol=0)


def test_adapter_upscales_to_a_multiple_of_64(model, dev):
    """70 x 100 -> 128 x 128, default depth range (0.2 .. 100: the range at which the reference's own hypothesis count breaks)"""
    s = gc.synthetic_sample(3, 70, 100, 2)
    pred, _ = model.run(images=s["images"], keyview_idx=0, poses=s["poses"], intrinsics=s["intrinsics"])
    assert pred["depth"].shape == (1, 128, 128) and pred["depth_uncertainty"].shape == (1, 128, 128)
    assert np.isfinite(pred["depth"]).all() and np.isfinite(pred["depth_uncertainty"]).all()


def test_buffer_cache_is_keyed_by_shape_and_views(model, dev):
    """two forwards with different (H, W, V) in one model, then the first again: each the same bits as a fresh model's"""
    ga, gb = load_golden(CASES["a"]), load_golden(CASES["b"])
    ia, ib = golden_inputs(ga, dev), golden_inputs(gb, dev)
    for k in ("images", "poses", "intrinsics"):  # case b with ONE source view: (2, 64, 64, 1) against (1, 64, 96, 2)
        ib[k] = ib[k][:2]
    with torch.no_grad():
        want_a, want_b = fresh_model(dev)(**ia)[0], fresh_model(dev)(**ib)[0]
        shared = fresh_model(dev)
        got_a, got_b, again_a = shared(**ia)[0], shared(**ib)[0], shared(**ia)[0]
    assert len(shared._bufs) == 2
    for got, want in ((got_a, want_a), (got_b, want_b), (again_a, want_a)):
        assert torch.equal(got["depth"], want["depth"]) and torch.equal(got["depth_uncertainty"], want["depth_uncertainty"])
    assert torch.isfinite(want_b["depth"]).all()
