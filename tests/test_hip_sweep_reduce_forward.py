"""The generic plane-sweep reduction's forward on every path of its five kernels (csrc/sweep_modes.hip: sweep_reduce_tile_kernel,
sweep_reduce_kernel, sweep_reduce_nhwc_kernel, sweep_groupcorr_nhwc_kernel<0|1|2>; sampling in csrc/sweep_homography.h), through
the product library, at small shapes, against the float64 restatement.

The cases, their inputs, the reference, the error bound K 2^-24 A and the restated dispatch are in tests/sweep_reduce_cases.py;
tests/test_sweep_reduce_cpu.py checks on the CPU that the cases reach every path, that their inputs cross all four borders and go
behind the camera in both pixel conventions and depth forms, and that the bound holds the reference's own float32 evaluation.

What is asserted:
  1. THE BOUND, per case, convention (pix_offset 0 with the w / (w - 1) stretch; pix_offset 0.5 without) and depth form ((B,D) and
     (B,D,h,w)): sweep_reduce_inference in all three modes, ops.sweep_reduce_nhwc in both variance modes, ops.sweep_groupcorr_nhwc
     without grid_clamp and, on the clamp cases, with 1.1: every element within K 2^-24 A of the float64 reference, every output
     finite.  No atol: where A is 0 (a view out of frame) the output is 0.  C = 260 is refused by both nhwc entries.
  2. WRAPPERS: cvp_proj_cost (both settings of reproduce_alias_bug, both depth forms) and vis_cost_volumes (shared and per-pixel
     depth_start) within the same bound of the restatement fed the matrices the wrapper computed, in the convention the wrapper
     documents; and those matrices within the float32 error of a 4 x 4 inverse and two products of the same formula in float64.
  3. STORES: the (B,C,D,h,w) and (B,G,D,h,w) outputs of mvd_sweep_reduce_f32 written between guard floats, once 16-byte aligned
     and once one float off (the tile kernel then takes its scalar store path: the same bits); the nhwc outputs written into slices
     of sentinel-filled buffers; guards untouched, two calls the same bits, all equal to the entry checked under 1.
  4. ZERO BORDER: a view translated out of frame has a group-correlation volume of exact zeros, and the variance is, bit for bit,
     the variance with that view's features set to zero.

Measured on the MI355X (pytest -s prints every comparison's error / bound; the worst per kernel over all cases):
  sweep_reduce_tile_kernel 0.305   sweep_reduce_kernel 0.260   sweep_reduce_nhwc_kernel 0.182
  sweep_groupcorr_nhwc_kernel<0> 0.056   <1> 0.305   <2> 0.212   cvp_proj_cost 0.142   vis_cost_volumes 0.224
i.e. every kernel sits where the reference's own float32 evaluation sits (0.32 on the CPU), a third of the bound (the 32-view
case: 0.27), with errors of 2e-7 .. 7e-6 on outputs of 0.4 .. 36; the wrappers' matrices are within 0.013 of their tolerance.
The module runs in 4 s.
ops.sweep_groupcorr_nhwc hands the entry consecutive slices of one buffer: with V > 1 and B D h w groups no multiple of 4 ("views32":
90 floats per view) the volumes after the first are only float-aligned, which mvd_sweep_groupcorr_nhwc_f32 accepts for out[v > 0]."""
import numpy as np
import pytest
import torch

import gen_common as gc
import sweep_reduce_cases as S
import test_sweep_grads_cpu as RS

pytestmark = pytest.mark.gpu
GUARD = 64  # floats on either side of an output
WORST = {}  # kernel -> the largest error / bound seen


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst error / bound per kernel: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def T(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def bordered(x):
    """(B,C,h,w) -> zero-bordered channel-last (B,h+3,w+3,C) with the map at (1,1)"""
    B, C, h, w = x.shape
    buf = torch.zeros((B, h + 3, w + 3, C), dtype=torch.float32, device=x.device)
    buf[:, 1:h + 1, 1:w + 1, :] = x.permute(0, 2, 3, 1)
    return buf


def mode_code(mode):
    from robustmvd_amd import _lib as L
    return dict(variance=L.REDUCE_VARIANCE, keysq=L.REDUCE_VARIANCE_KEYSQ, groupcorr=L.REDUCE_GROUPCORR)[mode]


def within(got, want, bound, kernel, what):
    """got (a tensor in the reference's layout) within `bound` of `want`, element by element"""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        ratio = float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print(f"{what} [{kernel}]: error / bound {ratio:.3f}, max |err| {err.max():.2e}, max |want| {np.abs(want).max():.3g}")
    assert (err <= bound).all(), f"{what}: error / bound {ratio:.3f}"


def device_inputs(name, conv, dev):
    c = S.case_inputs(name, conv)
    feats = [T(f, dev) for f in c["feats"]]
    return feats, [T(m, dev) for m in c["Ms"]], dict(shared=T(c["shared"], dev), per_pixel=T(c["per_pixel"], dev))


def reduce_kernel(name, mode):
    return "sweep_reduce_" + ("tile_kernel" if S.reduce_dispatch(*S.CASES[name].shape, mode)["kernel"] == "tile" else "kernel")


# ------------------------------------------------------------------------------------------------ 1. the bound
@pytest.mark.parametrize("conv", list(S.CONVENTIONS))
@pytest.mark.parametrize("name", list(S.CASES))
def test_forward_within_bound(name, conv, dev):
    from robustmvd_amd import ops, sweep_modes as SM
    B, C, D, h, w, V, G = S.CASES[name].shape
    kw = S.CONVENTIONS[conv]
    feats, Ms, depths = device_inputs(name, conv, dev)
    for form in S.DEPTH_FORMS:
        what = f"{name} {conv} {form}"
        for mode in S.MODES:
            want, bound = S.reference(name, conv, form, mode)
            got = SM.sweep_reduce_inference(feats[0], feats[1:], Ms, depths[form], mode_code(mode), groups=G, **kw)
            if mode == "groupcorr":
                assert len(got) == V
                for v in range(V):
                    within(got[v], want[v], bound[v], reduce_kernel(name, mode), f"{what} sweep_reduce {mode} view {v}")
            else:
                within(got, want, bound, reduce_kernel(name, mode), f"{what} sweep_reduce {mode}")
        if name not in S.NHWC_CASES:
            continue
        key, srcs = nhwc(feats[0]), [bordered(f) for f in feats[1:]]
        for mode in ("variance", "keysq"):
            want, bound = S.reference(name, conv, form, mode)
            got = ops.sweep_reduce_nhwc(key, srcs, Ms, depths[form], mode_code(mode), **kw)
            assert tuple(got.shape) == (B, D, h, w, C)
            within(got.permute(0, 4, 1, 2, 3), want, bound, "sweep_reduce_nhwc_kernel", f"{what} sweep_reduce_nhwc {mode}")
        qpu = S.nhwc_dispatch(C, D, h, w, G)["QPU"]
        for clamp in (False, True) if S.CASES[name].clamp else (False,):
            want, bound = S.reference(name, conv, form, "groupcorr", clamp)
            got = ops.sweep_groupcorr_nhwc(key, srcs, Ms, depths[form], G, grid_clamp=1.1 if clamp else 0.0, **kw)
            assert len(got) == V
            for v in range(V):
                assert tuple(got[v].shape) == (B, D, h, w, G)
                within(got[v].permute(0, 4, 1, 2, 3), want[v], bound[v], f"sweep_groupcorr_nhwc_kernel<{qpu}>",
                       f"{what} sweep_groupcorr_nhwc{' grid_clamp' if clamp else ''} view {v}")


def test_nhwc_entries_refuse_more_than_64_channels(dev):
    from robustmvd_amd import _lib as L, ops
    B, C, D, h, w, V, G = S.CASES["wide"].shape
    assert C > S.NHWC_MAX_C and S.nhwc_dispatch(C, D, h, w)["refused"]
    feats, Ms, depths = device_inputs("wide", "half", dev)
    key, srcs = nhwc(feats[0]), [bordered(f) for f in feats[1:]]
    with pytest.raises(ValueError):
        ops.sweep_reduce_nhwc(key, srcs, Ms, depths["shared"], L.REDUCE_VARIANCE)
    with pytest.raises(ValueError):
        ops.sweep_groupcorr_nhwc(key, srcs, Ms, depths["shared"], G)
    with pytest.raises(RuntimeError, match=r"status 1"):  # MVD_ERR_INVALID_ARG
        ops.call("mvd_sweep_reduce_nhwc_f32", dev, key, srcs, Ms, depths["shared"], 0, 0.5, 1.0, 1.0, -0.5, L.REDUCE_VARIANCE, B, C, D, h, w, V,
                 torch.empty((B, D, h, w, C), device=dev))
    with pytest.raises(RuntimeError, match=r"status 1"):
        ops.call("mvd_sweep_groupcorr_nhwc_f32", dev, key, srcs, Ms, depths["shared"], 0, 0.5, 1.0, 1.0, -0.5, 0.0, G, B, C, D, h, w, V,
                 [torch.empty((B, D, h, w, G), device=dev)])


# ------------------------------------------------------------------------------------------------ 2. the wrappers
def _cameras(B, V, h, w, seed):
    """float32 calibration: key intrinsics, source intrinsics (3 x the focal length), key extrinsics, source extrinsics (B,V,..)"""
    rng = np.random.default_rng(seed)
    K = gc.synthetic_intrinsics(h, w)
    Ks = K.copy()
    Ks[0, 0] *= 3.0
    Ks[1, 1] *= 3.0
    ref_ex = np.stack([gc.synthetic_pose(rng, 0.05, 0.1) for _ in range(B)])
    src_ex = np.zeros((B, V, 4, 4), np.float32)
    for b in range(B):
        for v in range(V):
            P = gc.synthetic_pose(rng, 0.1, 0.3).astype(np.float64)
            P[:3, 3] *= np.array([1, -1, 1]) * (-1) ** (v + b)
            src_ex[b, v] = (P @ ref_ex[b].astype(np.float64)).astype(np.float32)
    return np.stack([K] * B), np.stack([np.stack([Ks] * V)] * B), ref_ex, src_ex


def _matrices_agree(got, want, terms, cond, what):
    """the wrapper's float32 matrices against the float64 formula: an inverse (relative error <= n u cond, n = 4) and two matrix
    products (4 u each of the absolute products `terms`) -> 16 u (cond + 1) terms, element by element"""
    tol = 16 * S.U * (cond + 1) * terms
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max matrix error / tolerance {float((err / tol).max()):.3f}, condition number {cond:.1f}")
    assert (err <= tol).all(), what


def test_cvp_proj_cost_passes_its_convention(dev):
    """the "ragged" case's features and depths (two batch elements, 7 x 9) with cameras in CVP-MVSNet's form"""
    import robustmvd_amd as R
    from robustmvd_amd import sweep_modes as SM
    B, C, D, h, w, V, G = S.CASES["ragged"].shape
    c = S.case_inputs("ragged", "stretch")
    ref_in, src_in, ref_ex, src_ex = _cameras(B, V, h, w, 21)
    last = np.array([[0, 0, 0, 1.0]])
    Ms = []
    for v in range(V):
        got = SM._cvp_transform(T(ref_in, dev), T(src_in[:, v], dev), T(ref_ex, dev), T(src_ex[:, v], dev)).cpu().numpy()
        for b in range(B):
            sp = np.vstack((src_in[b, v].astype(np.float64) @ src_ex[b, v, :3].astype(np.float64), last))
            rp = np.vstack((ref_in[b].astype(np.float64) @ ref_ex[b, :3].astype(np.float64), last))
            inv = np.linalg.inv(rp)
            _matrices_agree(got[b], (sp @ inv)[:3], (np.abs(sp) @ np.abs(inv))[:3], np.linalg.cond(rp), f"_cvp_transform view {v} batch {b}")
        Ms.append(got)
    feats = [T(f, dev) for f in c["feats"]]
    for alias, mode in ((True, "keysq"), (False, "variance")):
        for form in S.DEPTH_FORMS:
            got = R.cvp_proj_cost(feats[0], feats[1:], T(ref_in, dev), T(src_in, dev), T(ref_ex, dev), T(src_ex, dev), T(c[form], dev),
                                  reproduce_alias_bug=alias)
            args = (c["feats"], Ms, c[form], mode, G, "stretch")
            within(got, S.evaluate(*args), S.bound_of(S.magnitude(*args), mode, C, G, V), "cvp_proj_cost", f"cvp_proj_cost alias={alias} {form}")


def test_vis_cost_volumes_passes_its_convention(dev):
    """the "units3" case's features (9 x 13, three groups, three views) with cameras in Vis-MVSNet's form; shared and per-pixel depth_start"""
    import robustmvd_amd as R
    from robustmvd_amd import sweep_modes as SM
    B, C, D, h, w, V, G = S.CASES["units3"].shape
    c = S.case_inputs("units3", "half")
    ref_in, src_in, ref_ex, src_ex = _cameras(B, V, h, w, 22)

    def cam(ex, K):
        m = np.zeros((B, 2, 4, 4), np.float32)
        m[:, 0] = ex
        m[:, 1, :3, :3] = K
        m[:, 1, 3, 3] = 1
        return m

    ref_cam, srcs_cam = cam(ref_ex, ref_in), [cam(src_ex[:, v], src_in[:, v]) for v in range(V)]
    Ms = []
    for v in range(V):
        got = SM._vis_transform(T(ref_cam, dev), T(srcs_cam[v], dev)).cpu().numpy()
        for b in range(B):
            Rl, tl, Kl = (x.astype(np.float64) for x in (ref_ex[b, :3, :3], ref_ex[b, :3, 3], ref_in[b]))
            Rr, tr, Kr = (x.astype(np.float64) for x in (src_ex[b, v, :3, :3], src_ex[b, v, :3, 3], src_in[b, v]))
            Kl_inv = np.linalg.inv(Kl)
            A, b3 = Kr @ Rr @ Rl.T @ Kl_inv, -(Kr @ Rr @ ((-Rr.T @ tr) - (-Rl.T @ tl)))
            terms = np.hstack((np.abs(Kr) @ np.abs(Rr) @ np.abs(Rl.T) @ np.abs(Kl_inv),
                               (np.abs(Kr) @ np.abs(Rr) @ (np.abs(Rr.T) @ np.abs(tr) + np.abs(Rl.T) @ np.abs(tl)))[:, None]))
            _matrices_agree(got[b], np.hstack((A, b3[:, None])), 2 * terms, np.linalg.cond(Kl), f"_vis_transform view {v} batch {b}")
        Ms.append(got)
    feats = [T(f, dev) for f in c["feats"]]
    rng = np.random.default_rng(23)
    interval = np.full((B, 1, 1, 1), 2.0, np.float32)
    starts = dict(shared=np.full((B, 1, 1, 1), 1.5, np.float32), per_pixel=(1.5 * (0.5 + rng.random((B, 1, h, w)))).astype(np.float32))
    for form, start in starts.items():
        got = R.vis_cost_volumes(feats[0], T(ref_cam, dev), feats[1:], [T(sc, dev) for sc in srcs_cam], D, T(start, dev), T(interval, dev), groups=G)
        depth = RS.vis_depth(start, interval, D, h, w)
        assert depth.shape == ((B, D) if form == "shared" else (B, D, h, w))
        args = (c["feats"], Ms, depth, "groupcorr", G, "half")
        want, bound = S.evaluate(*args), S.bound_of(S.magnitude(*args), "groupcorr", C, G, V)
        assert len(got) == V
        for v in range(V):
            within(got[v], want[v], bound[v], "vis_cost_volumes", f"vis_cost_volumes {form} view {v}")
            assert np.abs(want[v]).max() > 1  # samples land in the map


# ------------------------------------------------------------------------------------------------ 3. the stores
def guarded(shapes, offset, dev, fill=-3.0):
    """outputs of `shapes`, each between GUARD floats of `fill`, the first `offset` floats into a 16-byte aligned buffer
    -> (buffer, outputs, mask of the buffer's guard floats)"""
    sizes = [int(np.prod(s)) for s in shapes]
    total = offset + GUARD + sum(n + GUARD + 3 for n in sizes)
    buf = torch.full((total,), fill, device=dev)
    assert buf.data_ptr() % 16 == 0
    guard = torch.ones(total, dtype=torch.bool, device=dev)
    outs, at = [], offset + GUARD
    for n, s in zip(sizes, shapes):
        pad = (-n) % 4 if offset == 0 else 0  # keeps every aligned output aligned
        outs.append(buf[at:at + n].view(s))
        guard[at:at + n] = False
        at += n + GUARD + pad
    return buf, outs, guard


@pytest.mark.parametrize("name", list(S.CASES))
def test_stores_stay_inside_their_output(name, dev):
    from robustmvd_amd import _lib as L, ops, sweep_modes as SM
    B, C, D, h, w, V, G = S.CASES[name].shape
    kw = S.CONVENTIONS["half"]
    feats, Ms, depths = device_inputs(name, "half", dev)
    wsb = L.load().mvd_sweep_reduce_workspace_bytes(B, C, h, w, V)
    for form in S.DEPTH_FORMS:
        per_pixel = int(form == "per_pixel")
        for mode in S.MODES:
            want = SM.sweep_reduce_inference(feats[0], feats[1:], Ms, depths[form], mode_code(mode), groups=G, **kw)
            want = want if mode == "groupcorr" else [want]
            for offset in (0, 1):  # 16-byte aligned, and one float off: the tile kernel's float4 stores need the alignment
                buf, outs, guard = guarded([tuple(x.shape) for x in want], offset, dev)
                assert all(o.data_ptr() % 16 == 0 for o in outs) if offset == 0 else outs[0].data_ptr() % 16 == 4
                for _ in range(2):
                    ops.call("mvd_sweep_reduce_f32", dev, feats[0], feats[1:], Ms, depths[form], per_pixel, kw["pix_offset"], 1.0, 1.0, -0.5,
                             mode_code(mode), G, B, C, D, h, w, V, outs, ops.workspace(wsb, dev), wsb)
                    assert all(torch.equal(o, x) for o, x in zip(outs, want)), (form, mode, offset)
                    assert bool((buf[guard] == -3.0).all()), (form, mode, offset)
        if name not in S.NHWC_CASES:
            continue
        key, srcs = nhwc(feats[0]), [bordered(f) for f in feats[1:]]
        for mode in ("variance", "keysq"):
            want = ops.sweep_reduce_nhwc(key, srcs, Ms, depths[form], mode_code(mode), **kw)
            buf, (out,), guard = guarded([(B, D, h, w, C)], 0, dev)
            for _ in range(2):
                ops.call("mvd_sweep_reduce_nhwc_f32", dev, key, srcs, Ms, depths[form], per_pixel, kw["pix_offset"], 1.0, 1.0, -0.5, mode_code(mode),
                         B, C, D, h, w, V, out)
                assert torch.equal(out, want) and bool((buf[guard] == -3.0).all()), (form, mode)
        for clamp in (0.0, 1.1) if S.CASES[name].clamp else (0.0,):
            want = ops.sweep_groupcorr_nhwc(key, srcs, Ms, depths[form], G, grid_clamp=clamp, **kw)
            buf, (out,), guard = guarded([(V * B, D, h, w, G)], 0, dev)
            for _ in range(2):
                got = ops.sweep_groupcorr_nhwc(key, srcs, Ms, depths[form], G, grid_clamp=clamp, out=out, **kw)
                assert all(g.data_ptr() == out.data_ptr() + v * g.numel() * 4 for v, g in enumerate(got))
                assert all(torch.equal(g, x) for g, x in zip(got, want)) and bool((buf[guard] == -3.0).all()), (form, clamp)


# ------------------------------------------------------------------------------------------------ 4. the zero border
@pytest.mark.parametrize("conv", list(S.CONVENTIONS))
def test_view_out_of_frame_is_the_zero_border(conv, dev):
    from robustmvd_amd import ops, sweep_modes as SM
    B, C, D, h, w, V, G = S.CASES["out_of_frame"].shape
    kw = S.CONVENTIONS[conv]
    feats, Ms, depths = device_inputs("out_of_frame", conv, dev)
    blank = [feats[0], feats[1], torch.zeros_like(feats[2])]
    for form in S.DEPTH_FORMS:
        got = SM.sweep_reduce_inference(feats[0], feats[1:], Ms, depths[form], mode_code("groupcorr"), groups=G, **kw)
        assert int(torch.count_nonzero(got[1])) == 0 and int(torch.count_nonzero(got[0])) > 0
        key = nhwc(feats[0])
        for clamp in (0.0, 1.1):
            got = ops.sweep_groupcorr_nhwc(key, [bordered(f) for f in feats[1:]], Ms, depths[form], G, grid_clamp=clamp, **kw)
            assert int(torch.count_nonzero(got[1])) == 0 and int(torch.count_nonzero(got[0])) > 0
        for mode in ("variance", "keysq"):
            a = SM.sweep_reduce_inference(feats[0], feats[1:], Ms, depths[form], mode_code(mode), **kw)
            b = SM.sweep_reduce_inference(blank[0], blank[1:], Ms, depths[form], mode_code(mode), **kw)
            assert torch.equal(a, b), (form, mode)
            a = ops.sweep_reduce_nhwc(key, [bordered(f) for f in feats[1:]], Ms, depths[form], mode_code(mode), **kw)
            b = ops.sweep_reduce_nhwc(key, [bordered(f) for f in blank[1:]], Ms, depths[form], mode_code(mode), **kw)
            assert torch.equal(a, b), (form, mode)
