"""CPU checks of the point-cloud clean-up's definition (robustmvd_amd/cloud_clean.py): the numpy forms against an independent brute
force, the conditions of the scene `noisy` that the GPU tests rest on, the degenerate cases and the host path of the front ends."""
import math

import numpy as np
import pytest

import cloud_cases as CC
import cloud_clean_cases as C
import robustmvd_amd as R
from robustmvd_amd import cloud_clean as CL
from robustmvd_amd import cloud_eval as CE


def small_clouds():
    rng = np.random.default_rng(3)
    p = rng.uniform(0, 1, (150, 3)).astype(np.float32)
    p[[20, 31, 77]] = p[5]  # duplicates: neighbours of one another at distance 0
    p[9] = [np.nan, 0.5, 0.5]
    q = rng.uniform(0, 1, (40, 3)).astype(np.float32)
    q[3] = [0.5, np.inf, 0.5]
    q[4] = p[5]
    return q, p


@pytest.mark.parametrize("self_query", [True, False])
def test_numpy_forms_against_an_independent_brute_force(self_query):
    q, p = small_clouds()
    q = p if self_query else q
    r = 0.21
    lists = C.brute_neighbours(q, p, r, self_query)
    nb = CL.neighbourhood_numpy(q, r, None if self_query else p)
    assert nb.count.dtype == np.int32 and nb.sum_dist.dtype == nb.moments.dtype == np.float64 and nb.moments.shape == (len(q), 9)
    assert np.array_equal(nb.count, [len(row) for row in lists]) and nb.count.max() > 8 and nb.count.min() == 0
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    for i, row in enumerate(lists):
        v = [p[j].astype(np.float64) - q[i].astype(np.float64) for _, j in row]
        terms = [[float(np.sqrt(d2)) for d2, _ in row]] + [[x[a] for x in v] for a in range(3)] + [[x[a] * x[b] for x in v] for a, b in pairs]
        got = [nb.sum_dist[i]] + nb.moments[i].tolist()
        for g, t in zip(got, terms):
            assert abs(g - math.fsum(t)) <= (len(row) + 16) * C.SUM_BOUND * math.fsum(abs(x) for x in t)
    for k in (1, 5, 16):
        kn = CL.knn_numpy(q, k, r, None if self_query else p)
        for i, row in enumerate(lists):
            want = sorted(row, key=lambda e: (int(e[0].view(np.uint32)), e[1]))[:k]
            assert kn.count[i] == len(want) and kn.index[i, :len(want)].tolist() == [j for _, j in want]
            assert (kn.index[i, len(want):] == -1).all() and (kn.dist[i, len(want):] == np.float32(r)).all()
            assert np.array_equal(kn.dist[i, :len(want)], np.sqrt(np.array([d2 for d2, _ in want], np.float32)))
    if self_query:
        kn = CL.knn_numpy(p, 4, r)
        assert kn.index[5, :3].tolist() == [20, 31, 77] and (kn.dist[5, :3] == 0).all() and kn.count[9] == 0  # ties by index; the NaN point


def test_list_moments_equal_the_radius_moments_of_the_same_neighbours():
    """With k above every count the list holds the radius neighbourhood: equal counts, sums within the bound (another order)."""
    _, p = small_clouds()
    r = 0.12
    nb, kn = CL.neighbourhood_numpy(p, r), CL.knn_numpy(p, 16, r)
    assert nb.count.max() <= 16
    lm = CL.list_moments_numpy(p, None, kn.index, kn.dist)
    assert np.array_equal(lm.count, nb.count)
    scale = 2 * (nb.count[:, None] + 16) * C.SUM_BOUND * nb.count[:, None] * r * r  # each side within the bound of the exact sum
    assert (np.abs(lm.moments[:, 3:] - nb.moments[:, 3:]) <= scale).all() and (np.abs(lm.sum_dist - nb.sum_dist) <= scale[:, 0] / r).all()


@pytest.mark.parametrize("offset", C.OFFSETS)
def test_scene_conditions(offset):
    p, nb = C.noisy(offset), C.neighbourhood(offset)
    surface, floaters = nb.count[:C.N_SURFACE], nb.count[C.N_SURFACE:]
    print(f"\noffset {offset}: surface counts {surface.min()} / {np.median(surface):.0f} / {surface.max()}, floaters max {floaters.max()}")
    assert floaters.max() < 2 <= surface.min()
    kept = C.outliers(offset, "density")
    assert np.array_equal(kept.kept, np.arange(C.N_SURFACE)) and kept.threshold is None
    assert np.array_equal(kept.points, p[:C.N_SURFACE]) and np.array_equal(kept.colors, p[:C.N_SURFACE])
    assert np.array_equal(kept.normals, -p[:C.N_SURFACE]) and kept.keep.sum() == C.N_SURFACE
    # float32 membership against float64: no pair differs
    d = p[:, None, :].astype(np.float64) - p[None, :, :].astype(np.float64)
    inside = (d * d).sum(axis=2) < np.float64(np.float32(C.RADIUS)) ** 2
    np.fill_diagonal(inside, False)
    d32 = CL._pair_d2(p, p) < np.float32(C.RADIUS) * np.float32(C.RADIUS)
    np.fill_diagonal(d32, False)
    assert (inside != d32).sum() == 0 and np.array_equal(inside.sum(axis=1), nb.count)
    # the eigenvalue gap wherever a normal is estimated
    ok = nb.count >= 5
    N = nb.count[ok] + 1.0
    mean = nb.moments[ok, :3] / N[:, None]
    Cm = np.empty((ok.sum(), 3, 3))
    for t, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        Cm[:, a, b] = Cm[:, b, a] = nb.moments[ok, 3 + t] / N - mean[:, a] * mean[:, b]
    lam = np.linalg.eigvalsh(Cm)
    gap = ((lam[:, 1] - lam[:, 0]) / lam[:, 2]).min()
    print(f"smallest (l1 - l0) / l2: {gap:.3f}")
    assert gap >= 1e-2
    # normals against the analytic surface, oriented towards a viewpoint above it
    normals, curvature = CL.estimate_normals_numpy(p, radius=C.RADIUS, toward=np.array([0.0, 0.0, 5.0]) + offset)
    assert np.array_equal(np.isnan(curvature), ~ok) and np.array_equal((normals == 0).all(axis=1), ~ok)
    assert (normals[ok][:, 2] > 0).all() and (np.abs(np.linalg.norm(normals[ok].astype(np.float64), axis=1) - 1) < 2.0 ** -22).all()
    on = ok[:C.N_SURFACE]
    cos = (normals[:C.N_SURFACE].astype(np.float64) * C.analytic_normals(p[:C.N_SURFACE], offset)).sum(axis=1)[on]
    angle = np.degrees(np.arccos(np.clip(cos, -1, 1)))
    print(f"normals against the analytic surface: median {np.median(angle):.2f}, max {angle.max():.2f} degrees")
    assert np.median(angle) < 1.0 and angle.max() < 8.0
    assert (curvature[ok] >= 0).all() and (curvature[ok] < 1 / 3 + 1e-6).all()
    # no orientation: the largest component is positive; reference normals: the sign follows them
    free, _ = CL.estimate_normals_numpy(p, radius=C.RADIUS)
    assert (np.take_along_axis(free, np.abs(free).argmax(axis=1)[:, None], axis=1)[ok, 0] > 0).all()
    down, _ = CL.estimate_normals_numpy(p, radius=C.RADIUS, like=-normals)
    assert np.array_equal(down, -normals)
    # k nearest instead of the radius: the same surface, within the same sanity margin
    byk, _ = CL.estimate_normals_numpy(p, k=16, max_dist=0.3, toward=np.array([0.0, 0.0, 5.0]) + offset)
    cosk = (byk[:C.N_SURFACE].astype(np.float64) * C.analytic_normals(p[:C.N_SURFACE], offset)).sum(axis=1)
    assert np.median(np.degrees(np.arccos(np.clip(cosk, -1, 1)))) < 1.0


@pytest.mark.parametrize("offset", C.OFFSETS)
def test_both_statistical_branches_occur(offset):
    far = C.knn(offset, C.K, C.MAX_DIST_LONG)
    assert (far.count == C.K).all()
    eighth = far.dist[:, C.K - 1]
    assert eighth[:C.N_SURFACE].max() < C.MAX_DIST_SHORT < eighth[C.N_SURFACE:].min()
    short, long_ = C.outliers(offset, "short"), C.outliers(offset, "long")
    near = C.knn(offset, C.K, C.MAX_DIST_SHORT)
    # short: every floater lacks a full list, every surface point has one
    assert (near.count[C.N_SURFACE:] < C.K).all() and (near.count[:C.N_SURFACE] == C.K).all() and not short.keep[C.N_SURFACE:].any()
    # long: every floater has a full list and is above the threshold; no surface point is
    mean = CL.knn_means_numpy(far.dist, far.count)
    print(f"\noffset {offset}: threshold {long_.threshold:.4f}, smallest floater mean {mean[C.N_SURFACE:].min():.4f}, largest surface mean "
          f"{mean[:C.N_SURFACE].max():.4f}")
    assert not np.isnan(mean).any() and (mean[C.N_SURFACE:] > long_.threshold).all() and (mean[:C.N_SURFACE] <= long_.threshold).all()
    assert np.array_equal(long_.kept, np.arange(C.N_SURFACE)) and abs(long_.threshold - 0.1448) < 1e-3
    # the threshold is mean + 2 sigma of the means, in any order of summation
    assert abs(long_.threshold - (mean.mean() + C.STD_RATIO * mean.std(ddof=1))) < 1e-12
    assert abs(CL.fixed_sum_numpy(mean) - math.fsum(mean)) <= (len(mean) + 16) * C.SUM_BOUND * math.fsum(mean)


def test_fixed_sum_order():
    """fixed_sum_numpy against a literal replay of the two-level order on 5000 terms (three workgroups, the last one part full)."""
    a = np.random.default_rng(1).uniform(0, 1, 5000)
    pad = np.zeros(3 * 2048)
    pad[:5000] = a

    def workgroup(thread):
        waves = []
        for w in range(4):
            v = thread[64 * w:64 * w + 64]
            for s in (32, 16, 8, 4, 2, 1):
                v = [v[lane] + v[lane ^ s] for lane in range(64)]
            waves.append(v[0])
        return ((waves[0] + waves[1]) + waves[2]) + waves[3]

    partial = []
    for g in range(3):
        thread = [0.0] * 256
        for j in range(8):
            for t in range(256):
                thread[t] += pad[2048 * g + 256 * j + t]
        partial.append(workgroup(thread))
    want = workgroup([0.0 + x for x in partial] + [0.0] * 253)  # the final workgroup: thread t holds record t
    assert CL.fixed_sum_numpy(a) == want and CL.fixed_sum_numpy([]) == 0.0 and CL.fixed_sum_numpy([0.25]) == 0.25


def test_degenerate_normals():
    f = np.float32
    line = np.stack([np.linspace(0, 0.05, 8), np.zeros(8), np.zeros(8)], axis=1).astype(f)   # collinear
    dup = np.tile(np.array([[0.3, 0.3, 0.3]], f), (8, 1))                                       # all duplicates
    few = np.array([[0.6, 0.6, 0.6], [0.61, 0.6, 0.6], [0.6, 0.61, 0.6], [0.6, 0.6, 0.61]], f)  # 3 neighbours each
    rng = np.random.default_rng(2)
    plane = np.column_stack([rng.uniform(0.8, 0.9, (12, 2)), np.full(12, 0.5)]).astype(f)       # a patch of z = 0.5
    bad = np.array([[np.nan, 0.85, 0.5]], f)
    p = np.concatenate([line, dup, few, plane, bad])
    n, c = CL.estimate_normals_numpy(p, radius=0.2)
    assert (n[:20] == 0).all() and np.isnan(c[:20]).all() and (n[32] == 0).all() and np.isnan(c[32])
    assert np.array_equal(n[20:32], np.tile(np.array([[0, 0, 1]], f), (12, 1))) and (np.abs(c[20:32]) < 1e-12).all()
    nb = CL.neighbourhood_numpy(p, 0.2)
    assert (nb.count[:8] == 7).all() and (nb.count[8:16] == 7).all() and (nb.sum_dist[8:16] == 0).all() and (nb.count[16:20] == 3).all()
    assert nb.count[32] == 0 and (nb.count[20:32] == 11).all()  # the NaN point neither asks nor answers
    n3, _ = CL.estimate_normals_numpy(p, radius=0.2, min_neighbours=3)
    assert (np.abs(n3[16:20]) > 0).any(axis=1).all() and (n3[:16] == 0).all()
    # the orientation tie: a viewpoint in the plane, reference normals in it or invalid -> the largest component decides
    for kw in (dict(toward=np.array([0.85, 0.85, 0.5])), dict(like=np.tile(np.array([[1, 0, 0]], f), (len(p), 1))),
               dict(like=np.full((len(p), 3), np.nan, f)), dict(toward=np.tile(np.array([[0.85, 0.85, 0.5]], f), (len(p), 1)))):
        tie, _ = CL.estimate_normals_numpy(p, radius=0.2, **kw)
        assert np.array_equal(tie[20:32], n[20:32])
    below, _ = CL.estimate_normals_numpy(p, radius=0.2, toward=np.array([0.85, 0.85, -3.0]))
    assert np.array_equal(below[20:32], -n[20:32])
    # equal magnitudes: the first component decides the sign
    m = np.zeros((1, 9))
    m[0, 3:] = [2, -1, 0, 2, 0, 5]  # sum v v^T with the eigenvector (1, 1, 0) / sqrt 2 of the smallest eigenvalue
    first, _ = CL.normals_from_moments_numpy(np.zeros((1, 3), f), np.array([9]), m)
    assert first[0, 0] > 0 and first[0, 1] > 0 and abs(first[0, 0] - first[0, 1]) < 1e-7


def test_argument_errors():
    p = C.noisy(0.0)[:50]
    with pytest.raises(ValueError, match="exactly one of radius and k"):
        CL.estimate_normals(p)
    with pytest.raises(ValueError, match="exactly one of radius and k"):
        CL.estimate_normals(p, radius=0.1, k=4, max_dist=0.1)
    with pytest.raises(ValueError, match="k needs max_dist"):
        CL.estimate_normals(p, k=4)
    with pytest.raises(ValueError, match="at least 2"):
        CL.estimate_normals(p, radius=0.1, min_neighbours=1)
    with pytest.raises(ValueError, match="at most one"):
        CL.estimate_normals(p, radius=0.1, toward=(0, 0, 1), like=p)
    with pytest.raises(ValueError, match=r"expected \(3,\) or \(50, 3\)"):
        CL.estimate_normals(p, radius=0.1, toward=np.zeros((4, 3)))
    for k in (0, 17, 2.5):
        with pytest.raises(ValueError, match=r"supported 1\.\.16"):
            CL.cloud_knn(p, k, 0.1)
    with pytest.raises(ValueError, match="finite and > 0"):
        CL.cloud_knn(p, 4, 0.0)
    with pytest.raises(ValueError, match="finite and > 0"):
        CL.cloud_neighbourhood(p, np.inf)
    with pytest.raises(ValueError, match=r"\(n,3\)"):
        CL.cloud_neighbourhood(p[:, :2], 0.1)
    with pytest.raises(ValueError, match=r"each must be in \[0, 2097151\)"):
        CL.cloud_neighbourhood(p, 1e-7)
    with pytest.raises(ValueError, match="below radius"):
        CL.neighbourhood_numpy(p, 0.1, cell=0.1)
    with pytest.raises(ValueError, match=r"\['max_dist', 'radius'\]"):
        CL.remove_outliers(p, radius=0.1, max_dist=0.2)
    with pytest.raises(ValueError, match=r"\['k', 'min_neighbours', 'radius'\]"):
        CL.remove_outliers(p, radius=0.1, min_neighbours=2, k=3)
    with pytest.raises(ValueError, match=r"got \[\]"):
        CL.remove_outliers(p)
    with pytest.raises(ValueError, match="colors: shape"):
        CL.remove_outliers(p, p[:-1], radius=0.1, min_neighbours=2)
    with pytest.raises(ValueError, match="clean: unexpected"):
        CE.PointCloudEvaluation((0.01,), clean=dict(voxel=0.1))
    with pytest.raises(ValueError, match="remove_outliers takes"):
        CE.PointCloudEvaluation((0.01,), clean=dict(radius=0.1))
    with pytest.raises(ValueError, match="belong to align"):
        CE.PointCloudEvaluation((0.01,), gt_normals="estimate")
    with pytest.raises(ValueError, match="'estimate'"):
        CE.PointCloudEvaluation((0.01,), align="plane", gt_normals="guess")
    with pytest.raises(ValueError, match="normal_radius"):
        CE.PointCloudEvaluation((0.01,), align="plane", normal_radius=0.1)
    with pytest.raises(ValueError, match="align='plane' needs gt_normals"):
        CE.PointCloudEvaluation((0.01,), align="plane")(p, p)


def test_small_and_empty_clouds():
    empty = np.zeros((0, 3), np.float32)
    one = np.array([[0.5, 0.5, 0.5]], np.float32)
    for pts in (empty, one):
        nb, kn = CL.cloud_neighbourhood(pts, 0.1), CL.cloud_knn(pts, 3, 0.1)
        assert nb.count.tolist() == [0] * len(pts) and nb.moments.shape == (len(pts), 9) and kn.index.shape == (len(pts), 3)
        assert (kn.index == -1).all() and (kn.dist == np.float32(0.1)).all()
        out = CL.remove_outliers(pts, radius=0.1, min_neighbours=0)
        assert len(out.kept) == len(pts) and out.colors is None
        out = CL.remove_outliers(pts, k=1, std_ratio=1.0, max_dist=0.1)
        assert len(out.kept) == 0 and out.threshold == float("-inf") and out.points.shape == (0, 3)
        assert math.isnan(CL.cloud_spacing(pts, 0.1))
    q = C.noisy(0.0)[:30]
    assert CL.cloud_neighbourhood(q, 0.1, target=empty).count.sum() == 0 and CL.cloud_knn(empty, 2, 0.1, target=q).index.shape == (0, 2)
    two = np.array([[0, 0, 0], [0.03, 0.04, 0], [np.nan, 0, 0]], np.float32)
    assert abs(CL.cloud_spacing(two, 0.1) - 0.05) < 1e-8
    assert R.cloud_spacing is CL.cloud_spacing and R.remove_outliers is CL.remove_outliers and R.estimate_normals is CL.estimate_normals


def test_evaluation_with_clean_and_estimated_normals_on_the_host():
    q, gt = CC.scene_s(0.0)
    pred = np.concatenate([q[:1500], C.noisy(0.0)[C.N_SURFACE:]])
    plain = CE.PointCloudEvaluation(CC.S_THRESHOLDS, CC.S_MAX_DIST)(pred, gt)
    assert plain.n_removed == 0 and plain.n_pred == 1560
    rule = dict(radius=0.12, min_neighbours=2)
    cleaned = CE.PointCloudEvaluation(CC.S_THRESHOLDS, CC.S_MAX_DIST, clean=rule)(pred, gt, pred)
    direct = CL.remove_outliers_numpy(pred, **rule)
    assert 50 <= cleaned.n_removed == 1560 - len(direct.kept) < 100 and not direct.keep[1500:].any()
    assert cleaned.n_pred == len(direct.kept) and np.array_equal(cleaned.pred_points, direct.points)
    assert np.array_equal(cleaned.pred_colors, direct.points) and cleaned.accuracy < plain.accuracy
    # align="plane" on a ground truth without normals: estimated, and the registration recovers a small shift
    moved = (q[:600].astype(np.float64) + [0.004, -0.003, 0.005]).astype(np.float32)
    ev = CE.PointCloudEvaluation(CC.S_THRESHOLDS, CC.S_MAX_DIST, align="plane", gt_normals="estimate")
    assert ev.normal_radius == pytest.approx(0.12)
    a = ev(moved, gt)
    normals, _ = CL.estimate_normals(gt, radius=ev.normal_radius)
    b = CE.PointCloudEvaluation(CC.S_THRESHOLDS, CC.S_MAX_DIST, align="plane")(moved, gt, gt_normals=normals)
    assert a.registration is not None and a.accuracy == b.accuracy and np.array_equal(a.fscore, b.fscore)
    assert a.accuracy < CE.PointCloudEvaluation(CC.S_THRESHOLDS, CC.S_MAX_DIST)(moved, gt).accuracy
    assert CE.PointCloudEvaluation(CC.S_THRESHOLDS, CC.S_MAX_DIST, align="plane", normal_radius=0.1, gt_normals="estimate").normal_radius \
        == float(np.float32(0.1))
    scene = CE.evaluate_scene  # the keyword reaches PointCloudEvaluation
    with pytest.raises(ValueError, match="clean: unexpected"):
        scene(None, None, None, None, gt, thresholds=(0.01,), clean=dict(bad=1))
