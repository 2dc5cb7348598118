"""CPU checks of the registration's definition (robustmvd_amd/cloud_register.py), which is also the yardstick of the GPU tests:
transform_numpy against a long-double evaluation, pair_sums_numpy against math.fsum, the solvers on exact synthetic sums,
register_numpy on scene R (register_cases.py), the stop rules and PointCloudEvaluation(align=...) on host arrays."""
import math

import numpy as np
import pytest

import cloud_cases as CC
import register_cases as RC
from robustmvd_amd import cloud_eval as CE
from robustmvd_amd import cloud_register as CR


def random_transform(rng, scale=1.0, shift=1.0):
    T = np.eye(4)
    T[:3, :3] = scale * RC.rotation(rng.normal(size=3), rng.uniform(-40, 40))
    T[:3, 3] = rng.normal(size=3) * shift
    return T


@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_transform_against_long_double(offset):
    """One rounding to float32 of a float64 chain of five roundings: within half a float32 ulp plus 4 float64 roundings of the
    long-double value, i.e. at most 1 float32 ulp off and equal wherever the long-double value is not within 2^-50 relative of a tie."""
    rng = np.random.default_rng(3)
    p = (rng.uniform(-1, 1, (500, 3)) + offset).astype(np.float32)
    T = random_transform(rng, 1.03, offset + 1)
    q = CR.transform_numpy(p, T)
    L = np.longdouble
    want = (p.astype(L) @ T[:3, :3].astype(L).T + T[:3, 3].astype(L))
    got = q.astype(L)
    assert q.dtype == np.float32 and q.shape == p.shape
    assert (np.abs(got - want) <= 0.5 * np.spacing(np.abs(q)).astype(L) * (1 + 2.0 ** -20)).all()
    assert (q == want.astype(np.float32)).mean() > 0.999


def test_transform_invalid_rows_and_normals():
    rng = np.random.default_rng(4)
    p = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    p[3, 1], p[7, 0], p[9, 2] = np.nan, np.inf, -np.inf
    p[11] = 3e38
    T = random_transform(rng, 2.0)
    n = rng.normal(size=(40, 3)).astype(np.float32)
    n[5], n[6, 0] = 0, np.nan
    q, m = CR.transform_numpy(p, T, n)
    bad = [3, 7, 9, 11]  # 11 overflows float32 under the scale
    assert (q[bad].view(np.uint32) == 0x7fc00000).all() and np.isfinite(np.delete(q, bad, axis=0)).all()
    assert (m[[5, 6]] == 0).all()
    good = np.delete(np.arange(40), [5, 6])
    want = n[good].astype(np.float64) @ T[:3, :3].T
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert np.abs(m[good] - want).max() <= 2.0 ** -24 and np.abs(np.linalg.norm(m[good].astype(np.float64), axis=1) - 1).max() < 1e-7
    assert CR.transform_numpy(np.zeros((0, 3)), T).shape == (0, 3)
    with pytest.raises(ValueError, match="last row"):
        CR.transform_numpy(p, np.ones((4, 4)))
    with pytest.raises(ValueError, match="finite"):
        CR.transform_numpy(p, np.full((3, 4), np.nan))


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_pair_sums_against_fsum(offset, plane):
    """numpy's pairwise sum of N float64 terms is within N 2^-53 sum |term| of the exact sum (any order is); N and the pairs exact."""
    sc = RC.scene_r(offset)
    T = np.eye(4)
    q = CR.transform_numpy(sc["source"], T)
    _, index = CE.nearest_numpy(q, sc["target"], RC.R_RADIUS)
    pivot = np.full(3, offset)
    normals = sc["normals"].copy()
    normals[::7] = 0
    normals[3::11, 1] = np.nan
    nrm = normals if plane else None
    terms = CR.pair_terms_numpy(sc["source"], T, index, sc["target"], pivot, nrm)
    N, sums = CR.pair_sums_numpy(sc["source"], T, index, sc["target"], pivot, nrm)
    pair = index >= 0
    if plane:
        pair &= np.isfinite(normals[index]).all(axis=1) & (normals[index] != 0).any(axis=1)
    assert N == pair.sum() == len(terms) and (0 < N < RC.R_TRUE if plane else N == RC.R_TRUE)
    assert not pair[sc["far"]].any() and not pair[sc["nan"]].any()
    assert terms.shape[1] == (CR.PLANE_SUMS if plane else CR.POINT_SUMS) == len(sums)
    for k in range(terms.shape[1]):
        assert abs(sums[k] - math.fsum(terms[:, k])) <= N * 2.0 ** -53 * math.fsum(np.abs(terms[:, k]))
    # the terms themselves, from an independent float64 evaluation
    a = q[pair].astype(np.float64) - pivot
    b = sc["target"][index[pair]].astype(np.float64) - pivot
    if not plane:
        np.testing.assert_array_equal(terms[:, :3], a)
        np.testing.assert_array_equal(terms[:, 3:6], b)
        np.testing.assert_allclose(terms[:, 6:15], np.einsum("nr,nc->nrc", a, b).reshape(-1, 9), rtol=0, atol=0)
        np.testing.assert_allclose(terms[:, 17], ((a - b) ** 2).sum(axis=1), rtol=1e-15)
    else:
        u = normals[index[pair]].astype(np.float64)
        J = np.concatenate([np.cross(a, u), u], axis=1)
        r = ((a - b) * u).sum(axis=1)
        iu = np.triu_indices(6)
        np.testing.assert_allclose(terms[:, :21], J[:, iu[0]] * J[:, iu[1]], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(terms[:, 21:27], J * r[:, None], rtol=1e-9, atol=1e-18)
        np.testing.assert_allclose(terms[:, 27], r * r, rtol=1e-9, atol=1e-24)
    # no pair at all
    N0, s0 = CR.pair_sums_numpy(sc["source"], T, np.full(len(index), -1), sc["target"], pivot, nrm)
    assert N0 == 0 and (s0 == 0).all() and len(s0) == len(sums)


def exact_sums(a, b, pivot, normals=None):
    """The sums of given pairs (a in the moved source's frame, b the targets) through pair_sums_numpy with the identity"""
    return CR.pair_sums_numpy(a.astype(np.float32), np.eye(4), np.arange(len(a)), b.astype(np.float32), pivot, normals)


@pytest.mark.parametrize("similarity", [False, True])
def test_solve_point_recovers_a_known_map(similarity):
    rng = np.random.default_rng(11)
    a = np.round(rng.uniform(-1, 1, (50, 3)) * 1024) / 1024  # exact in float32
    T = random_transform(rng, 1.25 if similarity else 1.0)
    b = RC.apply64(T, a)
    pivot = np.array([0.25, -0.5, 0.125])
    # float64 sums of float64 pairs, formed here (pair_sums_numpy would round b to float32)
    A, B = a - pivot, b - pivot
    sums = np.concatenate([A.sum(0), B.sum(0), np.einsum("nr,nc->rc", A, B).reshape(-1), [(A * A).sum(), (B * B).sum(), ((A - B) ** 2).sum()]])
    M, t = CR.solve_point(len(a), sums, pivot, similarity)
    np.testing.assert_allclose(M, T[:3, :3], atol=1e-13)
    np.testing.assert_allclose(t, T[:3, 3], atol=1e-13)
    if similarity:  # the rigid solver on the same sums keeps the scale at one
        Mr, _ = CR.solve_point(len(a), sums, pivot, False)
        np.testing.assert_allclose(Mr @ Mr.T, np.eye(3), atol=1e-13)


def test_solve_point_reflection_case():
    """Targets that are a MIRROR image of the source: the unconstrained optimum is a reflection; the fix returns a proper rotation."""
    rng = np.random.default_rng(12)
    a = rng.uniform(-1, 1, (60, 3)) * [1, 1, 0.01]
    b = a * [1, 1, -1]
    pivot = np.zeros(3)
    sums = np.concatenate([a.sum(0), b.sum(0), np.einsum("nr,nc->rc", a, b).reshape(-1), [(a * a).sum(), (b * b).sum(), ((a - b) ** 2).sum()]])
    M, t = CR.solve_point(len(a), sums, pivot)
    assert abs(np.linalg.det(M) - 1) < 1e-12
    np.testing.assert_allclose(M @ M.T, np.eye(3), atol=1e-12)
    with pytest.raises(ValueError, match="at least 3"):
        CR.solve_point(2, sums, pivot)


def test_solve_plane_single_plane_keeps_the_sliding_directions():
    """Every target on the plane z = 0 with normal +z: only the height, the tilt about x and the tilt about y are observable; the
    in-plane translation and the rotation about z get a zero update."""
    rng = np.random.default_rng(13)
    b = np.column_stack([rng.uniform(-1, 1, (200, 2)), np.zeros(200)])
    tilt = RC.rotation((1, 0.5, 0), 0.2)
    a = b @ tilt.T + [0.0, 0.0, 0.01]
    normals = np.tile(np.float32([0, 0, 1]), (200, 1))
    N, sums = exact_sums(a, b, np.zeros(3), normals)
    assert N == 200
    M, t = CR.solve_plane(N, sums, np.zeros(3))
    assert abs(t[0]) < 1e-12 and abs(t[1]) < 1e-12 and abs(t[2] + 0.01) < 1e-4
    assert abs(M[1, 0] - M[0, 1]) < 1e-12  # no rotation about z
    moved = a @ M.T + t
    assert np.abs(moved[:, 2]).max() < 1e-4 < np.abs(a[:, 2]).max()
    with pytest.raises(ValueError, match="at least 6"):
        CR.solve_plane(5, sums, np.zeros(3))


@pytest.mark.parametrize("mode", RC.R_MODES)
@pytest.mark.parametrize("offset", RC.R_OFFSETS)
def test_register_numpy_recovers_t_star(offset, mode):
    """Within 1e-8 of T* at offset 0 and a tenth of a float32 ulp of the coordinates (6e-5) at offset 1000, on every source point."""
    ref = RC.reference(offset, mode)
    reg, sc = ref["reg"], ref["scene"]
    print(f"\nR +{int(offset)} {mode}: {reg.iterations} iterations, pairs {reg.pairs}, rmse {reg.rmse:.3g}, error {ref['err']:.3g}")
    assert reg.converged and reg.reason == "converged" and 2 <= reg.iterations <= 16 and len(reg.history) == reg.iterations
    assert reg.pairs == RC.R_TRUE  # the far and the NaN rows never pair
    assert ref["err"] <= (1e-8 if offset == 0 else 6e-6)
    assert abs(reg.scale - (RC.R_SCALE if mode == "similarity" else 1.0)) < 1e-6
    assert reg.transform.shape == (4, 4) and reg.transform.dtype == np.float64
    moved = reg.apply(sc["source"])
    assert moved.dtype == np.float32 and np.isnan(moved[sc["nan"]]).all()
    assert np.abs(moved[sc["true"]] - sc["target"][sc["chosen"]]).max() <= 2 * np.spacing(np.float32(offset + 1))


def test_stop_rules_stages_and_too_few_pairs():
    sc = RC.scene_r(0.0)
    s, p = sc["source"], sc["target"]
    one = CR.register_numpy(s, p, RC.R_RADIUS, iterations=1)
    assert not one.converged and one.reason == "iterations" and one.iterations == 1 and len(one.history) == 1
    loose = CR.register_numpy(s, p, RC.R_RADIUS, tol=1.0)
    assert loose.converged and loose.iterations == 1
    # stages: each has its own budget and the radius of every iteration is in the history
    staged = CR.register_numpy(s, p, (0.2, 0.1, 0.05), iterations=3)
    radii = [h[0] for h in staged.history]
    assert radii == sorted(radii, reverse=True) and set(np.float32(radii)) == set(np.float32([0.2, 0.1, 0.05]))
    assert all(radii.count(r) <= 3 for r in set(radii)) and staged.iterations == len(radii)
    # the result's pairs and rmse are the last iteration's
    assert (staged.pairs, staged.rmse) == (staged.history[-1][1], staged.history[-1][2])
    with pytest.raises(ValueError, match="descend"):
        CR.register_numpy(s, p, (0.05, 0.1))
    with pytest.raises(ValueError, match="radii"):
        CR.register_numpy(s, p, -1.0)
    with pytest.raises(ValueError, match="target_normals"):
        CR.register_numpy(s, p, 0.1, mode="plane")
    with pytest.raises(ValueError, match="mode"):
        CR.register_numpy(s, p, 0.1, mode="affine")
    # too few pairs: a source far from every target, two pairs, and an empty target
    far = CR.register_numpy(s[sc["far"]], p, RC.R_RADIUS)
    assert not far.converged and far.reason == "too few pairs" and far.pairs == 0 and far.iterations == 0
    assert np.array_equal(far.transform, np.eye(4)) and math.isnan(far.rmse)
    two = CR.register_numpy(p[:2], p, RC.R_RADIUS)
    assert two.reason == "too few pairs" and two.pairs == 2
    none = CR.register_numpy(s, np.zeros((0, 3)), RC.R_RADIUS)
    assert none.reason == "too few pairs"
    # an init that is already T*: one step that does not move
    exact = CR.register_numpy(s, p, RC.R_RADIUS, init=sc["t_star"])
    assert exact.converged and exact.iterations == 1 and exact.history[0][3] < 1e-6


def test_register_clouds_dispatch_and_default_tol():
    sc = RC.scene_r(1000.0)
    ref = RC.reference(1000.0, "rigid")["reg"]
    reg = CR.register_clouds(sc["source"], sc["target"], RC.R_RADIUS)
    assert np.array_equal(reg.transform, ref.transform)
    # the default tol at offset 1000 is the ulp term, 2^-21 x 1001, above 1e-3 x the radius
    assert reg.history[-1][3] <= 2.0 ** -21 * 1001.0 and reg.history[-2][3] > 2.0 ** -21 * 1001.0


def test_evaluation_with_alignment_on_host_arrays():
    sc = RC.scene_r(0.0)
    good = sc["target"][sc["chosen"]]
    displaced = sc["source"][sc["true"]]
    th = (0.005, 0.01, 0.03)
    plain = CE.PointCloudEvaluation(th, 0.03)
    base, off = plain(good, sc["target"]), plain(displaced, sc["target"])
    assert base.registration is None and off.precision[0] < 0.5 < base.precision[0] == 1.0
    for align in ("rigid", "plane"):
        ev = CE.PointCloudEvaluation(th, 0.03, align=align, gt_normals=sc["normals"] if align == "plane" else None)
        assert ev.align_max_dist == [float(np.float32(v)) for v in (0.12, 0.06, 0.03)]
        score = ev(displaced, sc["target"])
        assert score.registration.converged and score.precision[0] == 1.0 and abs(score.accuracy - base.accuracy) < 1e-6
        assert np.abs(score.pred_points - good).max() < 1e-6
    with pytest.raises(ValueError, match="gt_normals"):
        CE.PointCloudEvaluation(th, 0.03, align="plane")(displaced, sc["target"])
    with pytest.raises(ValueError, match="align must be"):
        CE.PointCloudEvaluation(th, align="affine")
    with pytest.raises(ValueError, match="belong to align"):
        CE.PointCloudEvaluation(th, align_max_dist=0.1)
