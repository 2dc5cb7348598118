"""GPU tests of the differentiable sweep consumers: sweep_reduce / cvp_proj_cost / vis_cost_volumes
(mvd_sweep_reduce_backward_f32) and the warp-only sweep (mvd_sweep_warp_backward_f32).

Golden parity: gradients by autograd through the reference's own functions (tests/golden/g15_sweep_grads.npz) at g11's and g13's
shapes, atol 2e-4 / rtol 1e-4 (the project's tolerance for scatter-add gradients, tests/test_hip_backward.py); the forward value of
the autograd path must be the inference path's, bit for bit.
Other shapes: the float64 restatement that tests/test_sweep_grads_cpu.py pins against the same fixture, atol 3e-4 / rtol 1e-3
(as test_warp_variance_backward_ragged_vs_oracle).  Every case uses valid inputs."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import gen_common as gc
import test_sweep_grads_cpu as RS
from test_hip_shapes import mvs_inputs

pytestmark = pytest.mark.gpu
GOLD = dict(atol=2e-4, rtol=1e-4)
RAGGED = dict(atol=3e-4, rtol=1e-3)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def T(x, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_(grad)


def close(got, want, what, tol):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    print(f"{what}: max |diff| {np.abs(got - want).max():.3e}, max |want| {np.abs(want).max():.3e}")
    assert np.isfinite(got).all(), what
    np.testing.assert_allclose(got, want, err_msg=what, **tol)


def backward(outs, cots, inputs, dev):
    loss = sum((o * T(c, dev)).sum() for o, c in zip(outs, cots))
    return torch.autograd.grad(loss, inputs)


# ------------------------------------------------------------------------------------------------ golden parity
@pytest.mark.parametrize("name", ["pp", "pl"])
@pytest.mark.parametrize("alias", [True, False])
def test_cvp_proj_cost_gradients_golden(name, alias, dev):
    import robustmvd_amd as R
    g, gr = load_golden("g11_sweep_modes"), load_golden("g15_sweep_grads")
    key, srcs = T(g["cvp_ref"], dev, True), [T(g["cvp_src0"], dev, True), T(g["cvp_src1"], dev, True)]
    calib = [T(g[k], dev) for k in ("cvp_ref_in", "cvp_src_in", "cvp_ref_ex", "cvp_src_ex")]
    hyp = T(g[f"cvp_hyp_{name}"], dev)
    out = R.cvp_proj_cost(key, srcs, *calib, hyp, reproduce_alias_bug=alias)
    assert out.requires_grad
    with torch.no_grad():
        assert torch.equal(out, R.cvp_proj_cost(key, srcs, *calib, hyp, reproduce_alias_bug=alias))
    tag, suf = (f"cvp_{name}", "") if alias else (f"cvp_{name}_noalias", "_f64")
    got = backward([out], [gc.rng_array(int(gr[tag + "_seed"]), tuple(out.shape))], [key] + srcs, dev)
    for a, k in zip(got, ("dkey", "dsrc0", "dsrc1")):
        close(a, gr[f"{tag}_{k}{suf}"], f"{tag}_{k}", GOLD)


@pytest.mark.parametrize("name", ["s", "p"])
def test_vis_cost_volumes_gradients_golden(name, dev):
    import robustmvd_amd as R
    g, gr = load_golden("g11_sweep_modes"), load_golden("g15_sweep_grads")
    key, srcs = T(g["vis_ref"], dev, True), [T(g["vis_src0"], dev, True), T(g["vis_src1"], dev, True)]
    args = (T(g["vis_ref_cam"], dev), srcs, [T(g["vis_src_cam0"], dev), T(g["vis_src_cam1"], dev)], 5, T(g[f"vis_ds_{name}"], dev),
            T(g[f"vis_di_{name}"], dev))
    outs = R.vis_cost_volumes(key, *args, groups=8)
    assert isinstance(outs, list) and len(outs) == 2 and all(o.requires_grad for o in outs)
    with torch.no_grad():
        for a, b in zip(outs, R.vis_cost_volumes(key, *args, groups=8)):
            assert torch.equal(a, b)
    seed = int(gr[f"vis_{name}_seed"])
    got = backward(outs, [gc.rng_array(seed + v, tuple(o.shape)) for v, o in enumerate(outs)], [key] + srcs, dev)
    for a, k in zip(got, ("dkey", "dsrc0", "dsrc1")):
        close(a, gr[f"vis_{name}_{k}"], f"vis_{name}_{k}", GOLD)


@pytest.mark.parametrize("norm,name", [("dim", "none"), (False, "none"), ("before", "before"), ("after", "after"), (True, "after")])
def test_warp_only_gradients_golden(norm, name, dev):
    import robustmvd_amd as R
    g, gr = load_golden("g13_warp_only"), load_golden("g15_sweep_grads")
    fk = T(gc.rng_array(1501, (1, 16, 12, 18)), dev)
    srcs = [T(gc.rng_array(1502, (1, 16, 12, 18)), dev, True), T(gc.rng_array(1503, (1, 16, 12, 18)), dev, True)]
    kw = dict(num_sampling_points=6, min_depth=0.4, max_depth=1000.0)
    blk = R.PlanesweepCorrelation(warp_only=True, normalize=norm, differentiable=True)
    warped, masks, _ = blk(fk, T(g["K"], dev), srcs, [T(g["T0"], dev), T(g["T1"], dev)], **kw)
    assert all(x.requires_grad for x in warped) and not any(m.requires_grad for m in masks)
    with torch.no_grad():
        w0, m0, _ = blk(fk, T(g["K"], dev), srcs, [T(g["T0"], dev), T(g["T1"], dev)], **kw)
    for a, b, ma, mb in zip(warped, w0, masks, m0):
        assert torch.equal(a, b) and torch.equal(ma, mb)
    seed = int(gr[f"warp_{name}_seed"])
    got = backward(warped, [gc.rng_array(seed + v, tuple(o.shape)) for v, o in enumerate(warped)], srcs, dev)
    for v in range(2):
        close(got[v], gr[f"warp_{name}_dsrc{v}"], f"warp_{name}_dsrc{v}", GOLD)


# ------------------------------------------------------------------------------------------------ other shapes, vs the restatement
def reduce_case(shape, seed, dev, modes=None, edit=None):
    """Runs sweep_reduce with grad on `shape` in each mode and compares every gradient with the restatement's."""
    from robustmvd_amd import _lib as L, sweep_modes as SM
    B, C, h, w, D, V, G = shape
    feats, projs, key_inv, depth = mvs_inputs(B, C, h, w, D, V, seed=seed)
    Ms = [np.ascontiguousarray((p @ key_inv)[:, :3, :4].astype(np.float32)) for p in projs]
    if edit is not None:
        edit(Ms)
    rng = np.random.default_rng(seed + 1)
    dpp = (depth[:, :, None, None] * (1 + 0.05 * rng.uniform(-1, 1, (B, D, h, w)))).astype(np.float32)
    cases = [("variance", L.REDUCE_VARIANCE, depth, {}), ("keysq", L.REDUCE_VARIANCE_KEYSQ, dpp, {})]
    if G:
        cases.append(("groupcorr", L.REDUCE_GROUPCORR, depth, dict(groups=G, pix_offset=0.5, stretch=False)))
    result = {}
    for mname, mode, dep, kw in cases:
        if modes and mname not in modes:
            continue
        ft = [T(f, dev, True) for f in feats]
        out = SM.sweep_reduce(ft[0], ft[1:], [T(m, dev) for m in Ms], T(dep, dev), mode, **kw)
        outs = out if isinstance(out, list) else [out]
        with torch.no_grad():
            ref = SM.sweep_reduce(ft[0], ft[1:], [T(m, dev) for m in Ms], T(dep, dev), mode, **kw)
        for a, b in zip(outs, ref if isinstance(ref, list) else [ref]):
            assert torch.equal(a, b)
        cots = [rng.standard_normal(tuple(o.shape)).astype(np.float32) for o in outs]
        got = backward(outs, cots, ft, dev)
        f64 = [RS.leaf64(f) for f in feats]
        want_out = RS.sweep_reduce_restated(f64[0], f64[1:], Ms, dep, mname, **kw)
        want = RS.grads_of(want_out if isinstance(want_out, list) else [want_out], cots, f64)
        for i, (a, b) in enumerate(zip(got, want)):
            close(a, b, f"{shape} {mname} d feat{i}", RAGGED)
        result[mname] = [x.cpu().numpy() for x in got]
    return result


@pytest.mark.parametrize("shape", [(1, 32, 21, 37, 4, 3, 4), (1, 16, 9, 14, 3, 1, 2), (2, 8, 5, 7, 2, 2, 0)])
def test_sweep_reduce_gradients_ragged_vs_restatement(shape, dev):
    """C/groups = 8 (two quads per group), one source, two batch elements with fewer pixels than a wave; odd sizes; per-plane and
    per-pixel depths"""
    reduce_case(shape, 11, dev)


def test_view_out_of_frame_has_zero_gradient(dev):
    """a source translated wholly out of frame: every tap is on the zero padding, its gradient is exactly zero"""
    def edit(Ms):
        Ms[1][:, 0, 3] += 1e6
    res = reduce_case((1, 16, 9, 14, 3, 2, 2), 12, dev, edit=edit)
    for grads in res.values():
        assert np.count_nonzero(grads[2]) == 0 and np.count_nonzero(grads[1]) > 0


def test_plane_behind_the_source_camera(dev):
    """Z <= 0 on the left part of the image (Z = 0 exactly on one column: X/Z is inf or NaN there): finite gradients that agree
    with the restatement"""
    def edit(Ms):
        Ms[0][:, 2, :] = np.array([0.1, 0.0, -0.7, 0.0], np.float32)  # Z = (0.1 x - 0.7) d: zero at x = 7, negative left of it
    reduce_case((1, 16, 9, 14, 3, 1, 2), 13, dev, modes=("variance", "keysq"), edit=edit)


def test_key_gradient_is_bit_reproducible(dev):
    """d key is a gather written once per element (no atomics): two calls give the same bits"""
    a = reduce_case((1, 32, 21, 37, 4, 3, 4), 14, dev)
    b = reduce_case((1, 32, 21, 37, 4, 3, 4), 14, dev)
    for m in a:
        assert np.array_equal(a[m][0], b[m][0]), m


def test_partial_grads_and_accumulation(dev):
    """only the key, or only one source, requires grad; a second backward accumulates into .grad"""
    from robustmvd_amd import _lib as L, sweep_modes as SM
    B, C, h, w, D, V = 1, 16, 9, 14, 3, 2
    feats, projs, key_inv, depth = mvs_inputs(B, C, h, w, D, V, seed=15)
    Ms = [T((p @ key_inv)[:, :3, :4].astype(np.float32), dev) for p in projs]
    cot = T(gc.rng_array(16, (B, C, D, h, w)), dev)
    full = [T(f, dev, True) for f in feats]
    want = torch.autograd.grad((SM.sweep_reduce(full[0], full[1:], Ms, T(depth, dev), L.REDUCE_VARIANCE) * cot).sum(), full)
    for only in range(V + 1):
        ft = [T(f, dev, i == only) for i, f in enumerate(feats)]
        out = SM.sweep_reduce(ft[0], ft[1:], Ms, T(depth, dev), L.REDUCE_VARIANCE)
        (out * cot).sum().backward()
        assert [f.grad is not None for f in ft] == [i == only for i in range(V + 1)]
        np.testing.assert_allclose(ft[only].grad.cpu().numpy(), want[only].cpu().numpy(), atol=1e-5, rtol=1e-5)
        first = ft[only].grad.clone()
        (SM.sweep_reduce(ft[0], ft[1:], Ms, T(depth, dev), L.REDUCE_VARIANCE) * cot).sum().backward()
        np.testing.assert_allclose(ft[only].grad.cpu().numpy(), 2 * first.cpu().numpy(), atol=2e-5, rtol=1e-5)


def test_warp_only_block_end_to_end(dev):
    """PlanesweepCorrelation(warp_only=True, differentiable=True) with sources of two different sizes (one launch per size), two
    batch elements with their own inverse depths: gradients reach both sources and agree with the restatement"""
    import robustmvd_amd as R
    g = load_golden("g13_warp_only")
    rng = np.random.default_rng(17)
    fs = [rng.standard_normal((2, 16, 12, 18)).astype(np.float32), rng.standard_normal((2, 16, 10, 14)).astype(np.float32)]
    K2, Ts = np.repeat(g["K"], 2, 0), [np.repeat(g["T0"], 2, 0), np.repeat(g["T1"], 2, 0)]
    inv2 = np.stack([g["invdepths"].reshape(-1), g["invdepths"].reshape(-1) * 0.7]).astype(np.float32)
    for norm in ("after", "before"):
        srcs = [T(f, dev, True) for f in fs]
        blk = R.PlanesweepCorrelation(warp_only=True, normalize=norm, differentiable=True)
        warped, masks, _ = blk(T(np.zeros((2, 16, 12, 18), np.float32), dev), T(K2, dev), srcs, [T(t, dev) for t in Ts],
                               sampling_invdepths=T(inv2, dev))
        cots = [rng.standard_normal(tuple(x.shape)).astype(np.float32) for x in warped]
        loss = sum((x * T(c, dev)).sum() for x, c in zip(warped, cots))
        loss.backward()
        f64 = [RS.leaf64(f) for f in fs]
        w_r, m_r = RS.sweep_warp_restated(f64, K2, [K2, K2], Ts, inv2, (12, 18), norm)
        want = RS.grads_of(w_r, cots, f64)
        for v in range(2):
            assert np.array_equal(masks[v].cpu().numpy(), m_r[v])
            assert srcs[v].grad is not None and tuple(srcs[v].grad.shape) == fs[v].shape
            close(srcs[v].grad, want[v], f"warp-only {norm} d src{v}", RAGGED)
