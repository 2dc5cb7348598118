"""CPU pins of tests/sweep_reduce_cases.py, the case table, reference and bound of tests/test_hip_sweep_reduce_forward.py: the cases
reach every path of the five kernels and each case is needed for one; their inputs cross all four borders, go behind the camera
and stay inside often enough in both pixel conventions and both depth forms; the "z0" case divides by an exact zero; the bound
K 2^-24 A holds the restatement's own float32 evaluation and is at least ten times tighter than the 1e-4 it replaces; the
grid_clamp reference agrees with test_vis_mvsnet_cpu.groupcorr_reference.

Measured here (pytest -s prints them): the share of samples inside the map is 2.8 to 12 % per case, convention and depth form (the
2 x 2 map: 0 to 8 %, exempt: two or three of its 16 samples touch the map); the float32 evaluation's worst error / bound is 0.32;
the worst bound / (1e-5 x the output's largest magnitude) is 0.94 ("views32": K = 79 on a variance of 33 samples, 0.35 .. 0.45)."""
import numpy as np
import pytest
import torch

import sweep_reduce_cases as S
import test_sweep_grads_cpu as RS
from test_vis_mvsnet_cpu import groupcorr_reference

f32 = np.float32
INSIDE_EXEMPT = ("smallest",)  # a 2 x 2 map: its interior is one cell, [0, 1] x [0, 1], and the source's focal length is 3 x the key's


# ------------------------------------------------------------------------------------------------ coverage
def test_cases_cover_every_path_and_each_is_needed():
    claimed = {}
    for name, case in S.CASES.items():
        reached = S.predict(name)
        print(name, case.shape, sorted(reached))
        for path in case.paths:
            assert path in reached, f"{name} does not reach {path}"
            claimed.setdefault(path, []).append(name)
    assert set(claimed) == set(S.REQUIRED_PATHS) and len(set(S.REQUIRED_PATHS)) == len(S.REQUIRED_PATHS)
    for name, case in S.CASES.items():  # without the case, a path it was added for has no case left
        assert any(claimed[path] == [name] for path in case.paths), f"{name} is needed for no path of its own"


def test_dispatch_details():
    """the numbers behind the labels"""
    d = S.reduce_dispatch(*S.CASES["ragged"].shape, "variance")
    assert d == dict(kernel="tile", units=4, ppw=64, workgroups=1, partial=True, batch=2, vec4=False)
    d = S.reduce_dispatch(*S.CASES["vec4"].shape, "variance")
    # 60 pixels in a workgroup of 64: 15 lanes per channel store a float4, 1 lies past the map.  With h w % 4 == 0 a lane's four
    # pixels are all inside or all outside the map: no lane stores part of a float4.
    assert (d["kernel"], d["ppw"], d["vec4"], d["lanes_float4"], d["lanes_else"], d["tail_stores"]) == ("tile", 64, True, 15, 1, 0)
    assert not S.reduce_dispatch(*S.CASES["vec4"].shape, "variance", out_aligned=False)["vec4"]
    for name, mode, units, why in (("smallest", "variance", 1, "units=1"), ("smallest", "groupcorr", 1, "units=1"),
                                   ("units3", "variance", 3, "not-a-power-of-two"), ("units6", "groupcorr", 6, "not-a-power-of-two"),
                                   ("one_group", "variance", 12, "not-a-power-of-two"), ("wide", "variance", 65, "units>64"),
                                   ("wide", "groupcorr", 5, "not-a-power-of-two")):
        d = S.reduce_dispatch(*S.CASES[name].shape, mode)
        assert (d["kernel"], d["units"], d["why"]) == ("plain", units, why), (name, mode, d)
    B, C, D, h, w, V, G = S.CASES["units3"].shape
    assert S.nhwc_dispatch(C, D, h, w)["idle"] == 1 and S.nhwc_dispatch(C, D, h, w, G)["idle"] == 1
    B, C, D, h, w, V, G = S.CASES["units6"].shape
    assert S.nhwc_dispatch(C, D, h, w, G) == dict(refused=False, units=6, ppw=42, idle=4, partial=True, chunks="8+1", QPU=1)
    assert S.nhwc_dispatch(C, D, h, w)["chunks"] == "8+1"
    assert [S.nhwc_dispatch(*S.CASES[n].shape[1:5], S.CASES[n].shape[6])["QPU"] for n in ("one_group", "chunks", "two_quads")] == [0, 1, 2]
    assert S.nhwc_dispatch(*S.CASES["chunks"].shape[1:5])["chunks"] == "8+8+3"
    assert S.nhwc_dispatch(*S.CASES["wide"].shape[1:5])["refused"]
    from robustmvd_amd import _lib as L
    assert S.CASES["views32"].shape[5] == L.MVD_MAX_VIEWS
    # grid_clamp: inside [-1, n] on a side below 10 pixels, the identity from 10 pixels on
    for name in S.CLAMP_CASES:
        B, C, D, h, w, V, G = S.CASES[name].shape
        xlo, xhi, ylo, yhi = S.host_bounds(h, w)
        assert (xlo > -1 and xhi < w) == (w < 10) and (ylo > -1 and yhi < h) == (h < 10), name
        assert (xlo, xhi) == (-1, w) or w < 10
        for n, lo, hi in ((w, xlo, xhi), (h, ylo, yhi)):  # 1.0f - 1.1f is exact, 1.0f + 1.1f is rounded: the upper bound is off the
            if n < 10:                                   # float64 formula by up to n / 2 ulp of 2.1f
                assert float(lo) == ((1 - S.GRID_CLAMP) * n - 1) / 2 and 0 < abs(float(hi) - ((1 + S.GRID_CLAMP) * n - 1) / 2) <= n * 2.0 ** -23


# ------------------------------------------------------------------------------------------------ the inputs
def test_generator_is_the_one_the_gpu_tests_had():
    """the values at the head of the streams of seed 7, shape (2, 16, 8, 12, 20, 2) of test_sweep_reduce_nhwc_is_sweep_reduce_permuted,
    drawn from numpy's generator in the order the two copies drew them: features, poses, per-pixel spread"""
    feats, Ms, shared, per_pixel = S.sweep_inputs_np(2, 16, 12, 20, 8, 2, 7)
    rng = np.random.default_rng(7)
    assert np.array_equal(feats[0], rng.standard_normal((2, 16, 12, 20)).astype(f32))
    assert [f.shape for f in feats] == [(2, 16, 12, 20)] * 3 and [m.shape for m in Ms] == [(2, 3, 4)] * 2
    assert shared.shape == (2, 8) and shared[0, 0] == f32(-0.7) and shared[0, 1] == f32(1.5) and shared[1, 7] == f32(22.0)
    assert per_pixel.shape == (2, 8, 12, 20) and per_pixel.dtype == f32
    ratio = per_pixel / shared[:, :, None, None]
    assert 0.5 <= ratio.min() < 0.51 and 1.49 < ratio.max() <= 1.5
    assert all(a.dtype == f32 for a in feats + Ms + [shared])


@pytest.mark.parametrize("conv", list(S.CONVENTIONS))
@pytest.mark.parametrize("name", list(S.CASES))
def test_inputs_exercise_the_edges(name, conv):
    B, C, D, h, w, V, G = S.CASES[name].shape
    c = S.case_inputs(name, conv)
    for form in S.DEPTH_FORMS:
        left = right = top = bottom = behind = False
        inside, total = 0, 0
        for M in c["Ms"]:
            ix, iy = RS.reduce_positions(M, c[form], h, w, **S.CONVENTIONS[conv])
            Z = S.source_depth(M, c[form], h, w, S.CONVENTIONS[conv]["pix_offset"])
            front = Z > 0
            left, right = left or bool(((ix == -1) & front).any()), right or bool(((ix == w) & front).any())
            top, bottom = top or bool(((iy == -1) & front).any()), bottom or bool(((iy == h) & front).any())
            behind = behind or bool((Z < 0).all(axis=(2, 3)).any())
            inside += int(((ix >= 0) & (ix <= w - 1) & (iy >= 0) & (iy <= h - 1)).sum())
            total += ix.size
        print(f"{name} {conv} {form}: inside {inside / total:.3f}, clamped in front of the camera l r t b {left} {right} {top} {bottom}, "
              f"a plane behind {behind}")
        assert left and right and top and bottom, "a border has no clamped sample in front of the camera"
        assert behind, "no plane lies behind the camera"
        assert name in INSIDE_EXEMPT or inside >= 0.02 * total


@pytest.mark.parametrize("conv", list(S.CONVENTIONS))
def test_z0_case_divides_by_zero(conv):
    B, C, D, h, w, V, G = S.CASES["z0"].shape
    c = S.case_inputs("z0", conv)
    for form in S.DEPTH_FORMS:
        Z = S.source_depth(c["Ms"][0], c[form], h, w, S.CONVENTIONS[conv]["pix_offset"])
        assert (Z[:, :, :, 7] == 0).all() and (Z[:, 1:, :, :7] < 0).all() and (Z[:, 1:, :, 8:] > 0).all()
        # X / Z there, before the clamp: +-inf, or NaN; after it -1 or w
        M = c["Ms"][0]
        X = S.source_depth(M, c[form], h, w, S.CONVENTIONS[conv]["pix_offset"], row=0)
        with np.errstate(all="ignore"):
            q = X[:, :, :, 7] / Z[:, :, :, 7]
        assert not np.isfinite(q).any()
        ix, _ = RS.reduce_positions(M, c[form], h, w, **S.CONVENTIONS[conv])
        assert np.isin(ix[:, :, :, 7], (-1, w)).all()
    # the constants of test_hip_sweep_grads.test_plane_behind_the_source_camera do NOT give a zero under the kernels' fmaf
    assert RS._fma(f32(0.1), f32(7), f32(-0.7)) != 0 and f32(0.1) * f32(7) + f32(-0.7) == 0


def test_out_of_frame_view_is_all_border():
    for conv in S.CONVENTIONS:
        B, C, D, h, w, V, G = S.CASES["out_of_frame"].shape
        c = S.case_inputs("out_of_frame", conv)
        for form in S.DEPTH_FORMS:
            ix, iy = RS.reduce_positions(c["Ms"][1], c[form], h, w, **S.CONVENTIONS[conv])
            assert np.isin(ix, (-1, w)).all()
            want, bound = S.reference("out_of_frame", conv, form, "groupcorr")
            assert not want[1].any() and not bound[1].any() and want[0].any()


def test_fma_rounds_once():
    """_fma against exact rational arithmetic, on random operands and on constructed half-way cases"""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(4000).astype(f32), rng.standard_normal(4000).astype(f32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 3, 4000)).astype(f32)
    # half-way cases: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 exactly, half-way between two float32; c = +-2^-60 is lost in the float64 sum
    a[:4], b[:4] = [1 + 2.0 ** -12, 1 + 2.0 ** -12, -(1 + 2.0 ** -12), -(1 + 2.0 ** -12)], f32(1 + 2.0 ** -12)
    c[:4] = [2.0 ** -60, -2.0 ** -60, 2.0 ** -60, -2.0 ** -60]
    got = RS._fma(a, b, c)

    def nearest(x):  # the float32 nearest to the rational x (ties to even cannot occur for the constructed cases)
        r = f32(float(x))
        cands = [r, np.nextafter(r, f32(np.inf)), np.nextafter(r, f32(-np.inf))]
        return min(cands, key=lambda v: abs(Fraction(float(v)) - x))

    for i in list(range(200)) + [int(j) for j in rng.integers(0, 4000, 200)]:
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert got[i] == nearest(exact), i
    naive = (a[:4].astype(np.float64) * b[:4].astype(np.float64) + c[:4].astype(np.float64)).astype(f32)
    assert (naive != got[:4]).any()  # the double rounding that _fma avoids


# ------------------------------------------------------------------------------------------------ the bound
@pytest.mark.parametrize("conv", list(S.CONVENTIONS))
@pytest.mark.parametrize("name", list(S.CASES))
def test_bound_holds_float32_evaluation_and_is_tight(name, conv):
    B, C, D, h, w, V, G = S.CASES[name].shape
    c = S.case_inputs(name, conv)
    for form in S.DEPTH_FORMS:
        for mode, clamp in [(m, False) for m in S.MODES] + ([("groupcorr", True)] if S.CASES[name].clamp else []):
            want, bound = S.reference(name, conv, form, mode, clamp)
            low = S.evaluate(c["feats"], c["Ms"], c[form], mode, G, conv, S.host_bounds(h, w) if clamp else None, dtype=f32)
            want, bound, low = (np.stack(x) if mode == "groupcorr" else x for x in (want, bound, low))
            assert np.isfinite(want).all() and np.isfinite(bound).all() and (bound >= 0).all()
            err = np.abs(low - want)
            with np.errstate(all="ignore"):
                ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max()
            scale = np.abs(want).max()
            print(f"{name} {conv} {form} {mode}{' clamp' if clamp else ''}: float32 error / bound {ratio:.3f}, max |err| {err.max():.2e}, "
                  f"max bound {bound.max():.2e}, max |want| {scale:.3g}, bound / (1e-5 scale) {bound.max() / (1e-5 * scale):.3f}")
            assert ratio <= 1.0
            assert S.K_VARIANCE(V) * S.U < 1e-5 and S.K_GROUPCORR(C // G // 4) * S.U < 1e-5
            assert bound.max() < 1e-5 * scale


# ------------------------------------------------------------------------------------------------ grid_clamp
EXACT_CLAMP = 1.0625  # bounds ((1 -+ g) n - 1) / 2 that are exact in float32 and float64, inside [-1, n] for n < 16


@pytest.mark.parametrize("grid_clamp", [EXACT_CLAMP, S.GRID_CLAMP])
@pytest.mark.parametrize("name", S.CLAMP_CASES)
def test_grid_clamp_reference_agrees_with_groupcorr_reference(name, grid_clamp):
    """On the clamp cases' shapes and features with matrices and planes whose positions are exact in float32 and float64
    (dyadic_inputs; on the cases' own poses the float32 positions differ from float64 ones by 1e-6 pixel, and the two references
    with them): 1e-12 with a grid_clamp of 1.0625, whose bounds are exact too.  With 1.1f the host's float32 upper bound is not
    the float64 formula's (test_dispatch_details): then 1e-12 holds for every sample the second clamp leaves alone, and the others
    are within the bounds' difference times the steepest slope of the blend, 2 max |src| per axis."""
    B, C, D, h, w, V, G = S.CASES[name].shape
    feats, Ms, shared = S.dyadic_inputs(name)
    xlo, xhi, ylo, yhi = bounds = S.host_bounds(h, w, grid_clamp)
    exact = [((1 - grid_clamp) * w - 1) / 2, ((1 + grid_clamp) * w - 1) / 2, ((1 - grid_clamp) * h - 1) / 2, ((1 + grid_clamp) * h - 1) / 2]
    delta = max(abs(float(a) - max(-1.0, min(float(n), b))) for a, b, n in zip(bounds, exact, (w, w, h, h)))
    assert delta == 0 if grid_clamp == EXACT_CLAMP else 0 < delta < 1e-6 or min(h, w) >= 10
    got = S.evaluate(feats, Ms, shared, "groupcorr", G, "half", bounds)
    want = groupcorr_reference([torch.from_numpy(np.array(f)) for f in feats], [torch.from_numpy(m) for m in Ms], torch.from_numpy(shared), G, grid_clamp)
    plain = S.evaluate(feats, Ms, shared, "groupcorr", G, "half")
    for v in range(V):
        ix, iy = RS.reduce_positions(Ms[v], shared, h, w, **S.CONVENTIONS["half"])
        if name not in INSIDE_EXEMPT:
            assert (ix == -1).any() and (ix == w).any() and (iy == -1).any() and (iy == h).any()
            assert ((ix >= 0) & (ix <= w - 1) & (iy >= 0) & (iy <= h - 1)).mean() > 0.02
        hit = np.broadcast_to(((ix < xlo) | (ix > xhi) | (iy < ylo) | (iy > yhi))[:, None], got[v].shape)
        diff = np.abs(got[v] - want[v].permute(0, 4, 1, 2, 3).numpy())
        slope = 4 * np.abs(feats[v + 1]).max() * np.abs(feats[0]).astype(np.float64).reshape(B, G, C // G, 1, h, w).sum(2)
        moved = np.abs(got[v] - plain[v]).max()
        print(f"{name} grid_clamp {grid_clamp} view {v}: max |diff| {diff.max():.2e} (samples the clamp leaves alone {diff[~hit].max():.2e}), "
              f"bounds off by {delta:.2e}, clamped {hit.mean():.2f}, the clamp moves the result by {moved:.2e}")
        assert diff[~hit].max() <= 1e-12 and (delta > 0 or diff.max() <= 1e-12)
        assert (diff <= 1e-12 + delta * np.broadcast_to(slope, diff.shape)).all()
        assert (moved > 1e-2) == (xlo > -1 or ylo > -1)
