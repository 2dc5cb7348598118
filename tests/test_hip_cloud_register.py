"""GPU checks of the registration kernels (csrc/cloud_register.hip), of register_clouds on GPU tensors and of
PointCloudEvaluation(align=...) / evaluate_scene(align=...), on the clouds of register_cases.py.  The reference project has no
counterpart: the yardstick is cloud_register.py's float64 numpy (itself checked in test_cloud_register_cpu.py).

Registration on scene R (test_registration_on_scene_r).  Every valid source point must land within
    4 x (the error register_numpy itself leaves against T*) + 2^-23 x (the largest |coordinate| of the target)
of where T* puts it: the factor 4 covers the float32 distance chain choosing another equal-distance neighbour and the other order of
the sums, the ulp term is one float32 rounding of q.  Measured on an MI355X (numpy's error from the numpy side alone):
    case              numpy: error   iterations   bound       device: error   iterations   error / bound
    R +0    rigid     1.01e-09       8            1.23e-07    1.01e-09        8            0.008
    R +0    simil.    1.19e-09       11           1.24e-07    1.19e-09        11           0.010
    R +0    plane     3.50e-09       3            1.33e-07    3.50e-09        3            0.026
    R +1000 rigid     1.09e-06       8            1.24e-04    1.09e-06        8            0.009
    R +1000 simil.    3.83e-06       10           1.35e-04    3.83e-06        10           0.028
    R +1000 plane     2.46e-06       3            1.29e-04    2.46e-06        3            0.019
The pair sums (test_pair_sums_against_fsum) stay below 0.02 of their bound N 2^-52 sum |term| at every size; the evaluation's counts
(test_evaluation_with_alignment) equal the undisplaced prediction's, with no distance within delta = 7e-7 of a threshold.
"""
import math

import numpy as np
import pytest
import torch

import cloud_cases as CC
import fusion_cases as FC
import register_cases as RC
from robustmvd_amd import cloud_eval as CE
from robustmvd_amd import cloud_register as CR
from robustmvd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = ops.CLOUD_PAIR_SUMS_PER_WG


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def some_transform(offset, seed=0, scale=1.02):
    """A few degrees and centimetres about the cloud's centre, scale 1.02: M and t with every bit of a double in use"""
    rng = np.random.default_rng(seed)
    c = np.full(3, float(offset))
    M = scale * RC.rotation(rng.normal(size=3), 4.0)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = M, c - M @ c + rng.normal(size=3) * 0.03
    return T


# ---- 1. transform ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_transform_equals_numpy_bit_for_bit(n, offset):
    rng = np.random.default_rng(100 + n)
    p = (rng.uniform(-1, 1, (n, 3)) + offset).astype(np.float32)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    if n >= 63:
        p[2, 0], p[9, 1], p[17, 2], p[30] = np.nan, np.inf, -np.inf, 3.3e38
        nrm[4], nrm[5, 2] = 0, np.nan
    T = some_transform(offset, n)
    want_q, want_n = CR.transform_numpy(p, T, nrm)
    q = ops.cloud_transform(up(p), T)
    assert q.dtype == torch.float32 and q.shape == (n, 3) and np.array_equal(bits(q), bits(want_q))
    q2, m = ops.cloud_transform(up(p), T, up(nrm))
    assert np.array_equal(bits(q2), bits(want_q)) and m.shape == (n, 3)
    assert (np.abs(m.cpu().numpy() - want_n) <= np.spacing(np.abs(want_n))).all()
    if n >= 63:
        assert (m.cpu().numpy()[[4, 5]] == 0).all() and (bits(q)[[2, 9, 17, 30]] == 0x7fc00000).all()
    # the records: a permuted perm, position i = T(p[perm[i]]) and perm[i]
    perm = rng.permutation(n).astype(np.int64)
    rec = ops.cloud_transform_records(up(p), up(perm), T)
    assert rec.shape == (n, 4)
    assert np.array_equal(bits(rec[:, :3]), bits(want_q[perm])) and np.array_equal(bits(rec[:, 3]), perm.astype(np.uint32))
    # Registration.apply on tensors is the same kernel
    reg = CR.Registration(T, 1.02, 0.0, 0, 0, True, "converged")
    assert np.array_equal(bits(reg.apply(up(p))), bits(want_q))


# ---- 2. pair sums ---------------------------------------------------------------------------------------------------------------------
def sums_case(n, offset, kind="mixed", seed=0):
    """n source points near scene R's targets (about a tenth far from all of them) through the inverse of a transform T
    -> (source, T, target, normals with zero and NaN rows)"""
    sc = RC.scene_r(offset)
    rng = np.random.default_rng(1000 + n + seed)
    T = some_transform(offset, seed)
    near = sc["target"][rng.integers(0, 4000, n)].astype(np.float64) + rng.normal(0, 0.01, (n, 3))
    if kind == "mixed":
        near[rng.uniform(size=n) < 0.1] += 5.0
        if n > 10:
            near[3] = np.nan
    elif kind == "none":
        near += 5.0
    src = RC.apply64(np.linalg.inv(T), near).astype(np.float32)
    normals = sc["normals"].copy()
    if kind != "every":
        normals[::7] = 0
        normals[3::11, 1] = np.nan
    return src, T, sc["target"], normals


def device_sums(src, T, target, normals, pivot, plane, radius=RC.R_RADIUS):
    """-> (index numpy, block tensor): the device's own nearest neighbours of the moved source, and its sums over them"""
    grid = ops.cloud_grid(up(target), target.min(0).astype(np.float64) - 0.5, float(np.float32(radius)) * ops.CLOUD_CELL_MARGIN)
    _, index = ops.cloud_nearest(ops.cloud_transform(up(src), T), grid, radius)
    block = ops.cloud_pair_sums(up(src), T, index, up(target), pivot, up(normals) if plane else None)
    assert block.dtype == torch.int64 and block.shape == (32,)
    return index.cpu().numpy(), block


def check_sums(src, T, target, normals, pivot, plane, index, block):
    """N exact; every sum within N 2^-52 sum |term| of math.fsum over pair_sums_numpy's terms (the any-order bound, times 2)."""
    nrm = normals if plane else None
    terms = CR.pair_terms_numpy(src, T, index, target, pivot, nrm)
    N, sums = ops.cloud_pair_sums_read(block, plane)
    assert N == len(terms) and sums.shape == (terms.shape[1],) and sums.dtype == np.float64
    assert (block[1 + len(sums):].cpu().numpy() == 0).all()
    worst = 0.0
    for k in range(terms.shape[1]):
        bound = N * 2.0 ** -52 * math.fsum(np.abs(terms[:, k]))
        err = abs(sums[k] - math.fsum(terms[:, k]))
        worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
        assert err <= bound, (k, err, bound)
    return N, worst


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1])
def test_pair_sums_against_fsum(n, plane):
    offset = 1000.0 if n % 2 else 0.0  # both offsets over the sizes; the pivot at the cloud's centre
    src, T, target, normals = sums_case(n, offset)
    pivot = np.full(3, offset)
    index, block = device_sums(src, T, target, normals, pivot, plane)
    N, worst = check_sums(src, T, target, normals, pivot, plane, index, block)
    print(f"\nn {n} {'plane' if plane else 'point'} +{int(offset)}: N {N}, worst error / bound {worst:.3f}")
    if n > 100:
        assert 0.5 * n < N < n  # paired and unpaired points in every workgroup
    # two calls, the same bits
    assert torch.equal(block, device_sums(src, T, target, normals, pivot, plane)[1])


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_pair_sums_no_pair_every_pair_and_the_pivot(plane):
    n = W + 65
    src, T, target, normals = sums_case(n, 1000.0, "none")
    index, block = device_sums(src, T, target, normals, np.zeros(3), plane)
    assert (index == -1).all() and (block.cpu().numpy() == 0).all()
    src, T, target, normals = sums_case(n, 1000.0, "every")
    for pivot in (np.zeros(3), np.full(3, 1000.0)):  # at 0 the terms are 10^6 times larger, and so is the bound
        index, block = device_sums(src, T, target, normals, pivot, plane)
        N, _ = check_sums(src, T, target, normals, pivot, plane, index, block)
        assert N == n and (index >= 0).all()
    # every normal zero or NaN: plane mode pairs nothing, point mode does not look at them
    bad = np.zeros_like(normals)
    bad[::2] = np.nan
    index, block = device_sums(src, T, target, bad, np.full(3, 1000.0), plane)
    assert ops.cloud_pair_sums_read(block, plane)[0] == (0 if plane else n)
    # an empty source and an empty target write zeros
    empty = ops.cloud_pair_sums(up(np.zeros((0, 3), np.float32)), T, torch.zeros(0, dtype=torch.int32, device=DEV), up(target),
                                np.zeros(3), up(normals) if plane else None)
    assert (empty.cpu().numpy() == 0).all()
    none = ops.cloud_pair_sums(up(src), T, torch.full((n,), -1, dtype=torch.int32, device=DEV), up(np.zeros((0, 3), np.float32)),
                               np.zeros(3), up(np.zeros((0, 3), np.float32)) if plane else None)
    assert (none.cpu().numpy() == 0).all()
    # an index that is no target's pairs with nothing
    wild = torch.full((n,), 4000, dtype=torch.int32, device=DEV)
    assert (ops.cloud_pair_sums(up(src), T, wild, up(target), np.zeros(3), up(normals) if plane else None).cpu().numpy() == 0).all()


# ---- 3. one step ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", RC.R_MODES)
def test_one_step_is_the_solver_on_the_device_sums(mode):
    """From the same T_0 the loop's first update equals solve_* on the sums of the kernels called by hand: the same host code, so
    exactly; this checks the wiring (pivot, radius, normals, composition)."""
    sc = RC.scene_r(1000.0, mode == "similarity")
    plane = mode == "plane"
    T0 = some_transform(1000.0, 7, scale=1.0)
    s, p, nrm = sc["source"], sc["target"], sc["normals"]
    reg = CR.register_clouds(up(s), up(p), RC.R_RADIUS, mode=mode, init=T0, target_normals=up(nrm) if plane else None, iterations=1,
                             tol=0.0)
    assert reg.iterations == 1 and not reg.converged and reg.reason == "iterations"
    box = np.stack([p.min(0), p.max(0)]).astype(np.float64)
    pivot = 0.5 * (box[0] + box[1])
    index, block = device_sums(s, T0, p, nrm, pivot, plane)
    N, sums = ops.cloud_pair_sums_read(block, plane)
    dM, dt = CR.solve_plane(N, sums, pivot) if plane else CR.solve_point(N, sums, pivot, mode == "similarity")
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = dM @ T0[:3, :3], dM @ T0[:3, 3] + dt
    assert np.array_equal(reg.transform, want)
    assert reg.pairs == N and reg.history[0][:2] == (float(np.float32(RC.R_RADIUS)), N)
    assert reg.rmse == math.sqrt(sums[-1] / N)


# ---- 4. registration ------------------------------------------------------------------------------------------------------------------
R_CASES = [(o, m) for o in RC.R_OFFSETS for m in RC.R_MODES]


@pytest.mark.parametrize("offset,mode", R_CASES, ids=[f"R+{int(o)}-{m}" for o, m in R_CASES])
def test_registration_on_scene_r(offset, mode):
    ref = RC.reference(offset, mode)
    sc = ref["scene"]
    s, p = up(sc["source"]), up(sc["target"])
    nrm = up(sc["normals"]) if mode == "plane" else None
    reg = CR.register_clouds(s, p, RC.R_RADIUS, mode=mode, target_normals=nrm)
    err = RC.landing_error(sc, reg.transform)
    bound = 4.0 * ref["err"] + 2.0 ** -23 * float(np.abs(sc["target"]).max())
    print(f"\nR +{int(offset)} {mode}: numpy error {ref['err']:.2e} in {ref['reg'].iterations} iterations, bound {bound:.2e}; device error "
          f"{err:.2e} in {reg.iterations} iterations, error / bound {err / bound:.3f}")
    assert reg.converged and reg.reason == "converged" and reg.iterations <= 50
    # the far and the NaN rows never pair: no iteration has more pairs than true points, and under the final T none of them has a neighbour
    assert all(h[1] <= RC.R_TRUE for h in reg.history) and reg.pairs == RC.R_TRUE
    index, _ = device_sums(sc["source"], reg.transform, sc["target"], sc["normals"], np.zeros(3), False)
    assert (index[sc["far"]] == -1).all() and (index[sc["nan"]] == -1).all() and (index[sc["true"]] >= 0).all()
    assert err <= bound
    assert abs(reg.scale - (RC.R_SCALE if mode == "similarity" else 1.0)) < 1e-5
    # the queries' order decides nothing: sorted once per stage instead of before every iteration, the same bits; and twice the same bits
    again = CR.register_clouds(s, p, RC.R_RADIUS, mode=mode, target_normals=nrm)
    once = CR._register_device(s, p, RC.R_RADIUS, mode, None, nrm, 50, None, resort=False)
    for other in (again, once):
        assert np.array_equal(bits(other.transform), bits(reg.transform)) and other.history == reg.history
    # apply: the aligned cloud is the numpy transform of the source, bit for bit
    assert np.array_equal(bits(reg.apply(s)), bits(CR.transform_numpy(sc["source"], reg.transform)))


# ---- 5. evaluation --------------------------------------------------------------------------------------------------------------------
def nearest_band(q, p):
    """cloud_cases.reference's band for any pair of clouds: 4 x the largest gap between nearest_numpy's float64 and float32 chains"""
    raw64, _ = CE.nearest_numpy(q, p, np.inf)
    raw32, _ = CE.nearest_numpy(q, p, np.inf, dtype=np.float32)
    both = np.isfinite(raw64) & np.isfinite(raw32)  # an invalid query is at inf in both
    return raw64, 4.0 * float(np.abs(raw32.astype(np.float64)[both] - raw64[both]).max())


@pytest.mark.parametrize("align", [None, "rigid", "similarity"])
def test_evaluation_with_alignment(align):
    """gt: scene R's 4000 targets; the undisplaced prediction: where T* puts scene R's source (2000 of the targets, the 200 far
    points, 5 NaN rows); displaced: the source itself, i.e. the prediction through the inverse of T*.  delta = test 4's bound on the
    displacement (with the error register_numpy itself leaves on this pair, register_cases.reference) + the nearest band, both from
    the numpy side alone.  2000 of the 4000 ground-truth points have no prediction on them, so the recall counts are decided by
    distances of every size."""
    mode = align or "rigid"
    ref = RC.reference(0.0, mode)
    sc = ref["scene"]
    gt, displaced = sc["target"], sc["source"]
    good = displaced.copy()
    good[sc["true"]] = gt[sc["chosen"]]
    good[sc["far"]] = RC.apply64(sc["t_star"], displaced[sc["far"]]).astype(np.float32)
    th, md = CC.S_THRESHOLDS, CC.S_MAX_DIST
    base = CE.cloud_scores_numpy(good, gt, th, md)
    assert base.n_pred == RC.R_TRUE + RC.R_FAR and base.precision[0] == RC.R_TRUE / base.n_pred and 0.4 < base.recall[0] < base.recall[2] < 1
    if align is None:
        off = CE.PointCloudEvaluation(th, md)(up(displaced), up(gt))
        assert off.registration is None and off.fscore[0] < base.fscore[0] and off.precision[0] < 0.5 * base.precision[0]
        return
    (raw_p, band_p), (raw_g, band_g) = nearest_band(good, gt), nearest_band(gt, good)
    delta = 4.0 * ref["err"] + 2.0 ** -23 * float(np.abs(gt).max()) + max(band_p, band_g)
    score = CE.PointCloudEvaluation(th, md, align=align, align_max_dist=RC.R_RADIUS)(up(displaced), up(gt))
    reg = score.registration
    assert reg.converged and score.pred_points.is_cuda and score.dist_pred.is_cuda and score.n_pred == base.n_pred
    ok = np.isfinite(good).all(axis=1)
    moved = np.linalg.norm(score.pred_points.cpu().numpy().astype(np.float64)[ok] - good[ok], axis=1).max()
    print(f"\nalign {align}: numpy's own error {ref['err']:.2e}, delta {delta:.2e}; device: the aligned points within {moved:.2e} of the undisplaced")
    for share, share0, raw, n in ((score.precision, base.precision, raw_p, base.n_pred), (score.recall, base.recall, raw_g, base.n_gt)):
        near = np.array([(np.abs(raw - np.float64(np.float32(t))) <= delta).sum() for t in th])
        print(f"  counts {np.round(share * n).astype(int).tolist()} against {np.round(share0 * n).astype(int).tolist()}, within delta of a threshold {near.tolist()}")
        assert (np.abs(share - share0) * n <= near + 1e-6).all()


def test_evaluate_scene_with_alignment():
    H, W_ = FC.SIZES[0]
    sc = FC.scene("B", H, W_)
    g = np.linspace(-2.5, 2.5, 126)
    gx, gy = np.meshgrid(g, g)
    gt = np.stack([gx.ravel(), gy.ravel(), (FC.PLANE_D - FC.PLANE_N[0] * gx.ravel() - FC.PLANE_N[1] * gy.ravel()) / FC.PLANE_N[2]],
                  axis=1).astype(np.float32)
    score = CE.evaluate_scene(FC.StubModel(H, W_), sc["images"], sc["Ks"], sc["Ts"], up(gt), thresholds=(0.02, 0.05), align="rigid")
    reg = score.registration
    assert isinstance(reg, CR.Registration) and reg.pairs > 500 and np.isfinite(reg.transform).all() and len(reg.history) >= 1
    assert score.pred_points.is_cuda and score.n_pred > 500 and np.isfinite(score.fscore).all()
    assert [h[0] for h in reg.history][0] == float(np.float32(4 * score.max_dist))  # the default radii start at 4 x max_dist


# ---- 6. arguments ---------------------------------------------------------------------------------------------------------------------
def test_arguments():
    sc = RC.scene_r(0.0)
    s, p, nrm = up(sc["source"]), up(sc["target"]), up(sc["normals"])
    with pytest.raises(ValueError, match="different places"):
        CR.register_clouds(s, sc["target"], 0.1)
    with pytest.raises(ValueError, match="target_normals"):
        CR.register_clouds(s, p, 0.1, mode="plane")
    with pytest.raises(ValueError, match="descend"):
        CR.register_clouds(s, p, (0.05, 0.1))
    with pytest.raises(ValueError, match="mode"):
        CR.register_clouds(s, p, 0.1, mode="affine")
    big = torch.zeros((1, 3), device=DEV).expand(2 ** 31, 3)  # no memory behind it
    with pytest.raises(ValueError, match=r"below 2\^31"):
        CR.register_clouds(big, p, 0.1)
    with pytest.raises(ValueError, match=r"below 2\^31"):
        CR.register_clouds(s, big, 0.1)
    with pytest.raises(ValueError, match=r"\(n,3\)"):
        ops.cloud_transform(s[:, :2], np.eye(4))
    with pytest.raises(ValueError, match="cuda"):
        ops.cloud_transform(s.cpu(), np.eye(4))
    with pytest.raises(ValueError, match="finite"):
        ops.cloud_transform(s, np.full((3, 4), np.inf))
    with pytest.raises(ValueError, match="last row"):
        ops.cloud_transform(s, np.ones((4, 4)))
    with pytest.raises(ValueError, match="shape"):
        ops.cloud_transform(s, np.eye(4), nrm)
    index = torch.zeros(s.shape[0], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="dtype"):
        ops.cloud_pair_sums(s, np.eye(4), index.long(), p, np.zeros(3))
    with pytest.raises(ValueError, match="shape"):
        ops.cloud_pair_sums(s, np.eye(4), index[:-1], p, np.zeros(3))
    with pytest.raises(ValueError, match="pivot"):
        ops.cloud_pair_sums(s, np.eye(4), index, p, (0.0, np.nan, 0.0))
    with pytest.raises(ValueError, match="shape"):
        ops.cloud_pair_sums(s, np.eye(4), index, p, np.zeros(3), nrm[:-1])
    with pytest.raises(ValueError, match="shape"):
        ops.cloud_transform_records(s, torch.zeros(3, dtype=torch.int64, device=DEV), np.eye(4))
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.cloud_transform(s.clone().requires_grad_(), np.eye(4))
