"""GPU checks of the point-cloud clean-up kernels (csrc/cloud_clean.hip) and of cloud_clean's front ends on GPU tensors, against the
numpy forms of robustmvd_amd/cloud_clean.py (themselves checked against an independent brute force in test_cloud_clean_cpu.py) on the
clouds of cloud_clean_cases.py and cloud_cases.py.  The pair distance is float32 numpy's chain bit for bit, so counts, indices,
distances and verdicts are compared for equality, and the float64 sums bit for bit once numpy adds in the device grid's order.

Normals (test_normals): the device's Jacobi against numpy.linalg.eigh on the device's own moments, before orientation
min(|n_dev - n_ref|, |n_dev + n_ref|) <= 2^-22 (the float32 rounding of a unit vector is sqrt(3) 2^-24; the float64 solve error at an
eigenvalue gap >= 1e-2 is far below it), the signs after orientation, and the curvature within 2^-23 c + 1e-12.  The measured maxima
are in profiles/cloud_clean.txt.
"""
import numpy as np
import pytest
import torch

import cloud_cases as CC
import cloud_clean_cases as C
from robustmvd_amd import cloud_clean as CL
from robustmvd_amd import cloud_eval as CE
from robustmvd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def grid_of(p, r, origin=None):
    p = np.asarray(p, dtype=np.float32).reshape(-1, 3)
    if origin is None:
        ok = np.isfinite(p).all(axis=1)
        origin = p[ok].min(axis=0).astype(np.float64) if ok.any() else np.zeros(3)
    return ops.cloud_grid(up(p), origin, float(np.float32(r)) * ops.CLOUD_CELL_MARGIN)


def check_moments(dev, ref):
    """count equal, sum_dist and the nine moments bit-equal"""
    count, sum_dist, moments = dev
    assert count.dtype == torch.int32 and sum_dist.dtype == moments.dtype == torch.float64 and moments.shape == (len(ref.count), 9)
    assert np.array_equal(count.cpu().numpy(), ref.count)
    assert same_bits(sum_dist, ref.sum_dist) and same_bits(moments, ref.moments)


def check_knn(dev, ref):
    index, dist, count = dev
    assert index.dtype == torch.int32 and dist.dtype == torch.float32 and count.dtype == torch.int32 and index.shape == ref.index.shape
    assert np.array_equal(index.cpu().numpy(), ref.index) and np.array_equal(count.cpu().numpy(), ref.count) and same_bits(dist, ref.dist)


@pytest.mark.parametrize("offset", C.OFFSETS)
def test_radius_moments_on_the_scene(offset):
    p = C.noisy(offset)
    grid = grid_of(p, C.RADIUS)
    dev = ops.cloud_radius_moments(None, grid, C.RADIUS)
    check_moments(dev, CL.neighbourhood_numpy(p, C.RADIUS, origin=grid.origin, cell=grid.cell))
    check_moments(dev, C.neighbourhood(offset))  # the front end's default grid is this one
    # against the sums in plain index order: within the bound of any order
    plain, total = C.index_order(offset)
    got = np.column_stack([dev[1].cpu().numpy(), dev[2].cpu().numpy()])
    want = np.column_stack([plain.sum_dist, plain.moments])
    bound = (plain.count[:, None] + 16) * C.SUM_BOUND * total
    print(f"\noffset {offset}: largest |device - index order| / bound {np.max(np.abs(got - want) / np.maximum(bound, 1e-300)):.3f}")
    assert np.array_equal(plain.count, dev[0].cpu().numpy()) and (np.abs(got - want) <= bound).all()
    front = CL.cloud_neighbourhood(up(p), C.RADIUS)
    assert torch.equal(front.count, dev[0]) and same_bits(front.moments, dev[2]) and same_bits(front.sum_dist, dev[1])


@pytest.mark.parametrize("base", CC.B_BASES)
def test_boundary(base):
    """One target a hair inside the radius across a cell corner in each of the 26 directions is counted; a hair outside, not."""
    for sign in "-+":
        q, p = CC.boundary(base, sign)
        grid = grid_of(p, CC.B_MAX_DIST, origin=np.full(3, base))  # the queries ON cell corners
        ref = CL.neighbourhood_numpy(q, CC.B_MAX_DIST, p, origin=grid.origin, cell=grid.cell)
        assert (ref.count == (1 if sign == "-" else 0)).all()
        check_moments(ops.cloud_radius_moments(up(q), grid, CC.B_MAX_DIST), ref)
        check_knn(ops.cloud_knn(up(q), grid, 2, CC.B_MAX_DIST), CL.knn_numpy(q, 2, CC.B_MAX_DIST, p))


def test_clustered():
    """5000 targets in one cell: the staging is chunked, not sized by the cell; the far queries find nothing."""
    q, p = CC.clustered()
    grid = grid_of(p, CC.C_MAX_DIST, origin=np.zeros(3))
    ref = CL.neighbourhood_numpy(q, CC.C_MAX_DIST, p, origin=grid.origin, cell=grid.cell)
    assert ref.count[:70].min() > 64 and (ref.count[70:] == 0).all()
    check_moments(ops.cloud_radius_moments(up(q), grid, CC.C_MAX_DIST), ref)
    check_knn(ops.cloud_knn(up(q), grid, 16, CC.C_MAX_DIST), CL.knn_numpy(q, 16, CC.C_MAX_DIST, p))


@pytest.mark.parametrize("m", [1, 2, 1000])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes(n, m):
    rng = np.random.default_rng(1000 * n + m)
    q, p = rng.uniform(0, 1, (n, 3)).astype(np.float32), rng.uniform(0, 1, (m, 3)).astype(np.float32)
    r = 0.15
    grid = grid_of(p, r)
    check_moments(ops.cloud_radius_moments(up(q), grid, r), CL.neighbourhood_numpy(q, r, p, origin=grid.origin, cell=grid.cell))
    check_knn(ops.cloud_knn(up(q), grid, 5, r), CL.knn_numpy(q, 5, r, p))


def test_empty_inputs():
    q = np.random.default_rng(0).uniform(0, 1, (70, 3)).astype(np.float32)
    empty = np.zeros((0, 3), np.float32)
    for target in (q, empty):
        nb, kn = CL.cloud_neighbourhood(up(empty), 0.1, up(target)), CL.cloud_knn(up(empty), 3, 0.1, up(target))
        assert nb.count.shape == (0,) and nb.moments.shape == (0, 9) and kn.index.shape == (0, 3) and kn.count.shape == (0,)
    nb, kn = CL.cloud_neighbourhood(up(q), 0.1, up(empty)), CL.cloud_knn(up(q), 3, 0.1, up(empty))
    assert (nb.count == 0).all() and (nb.moments == 0).all() and (nb.sum_dist == 0).all()
    assert (kn.index == -1).all() and (kn.dist == float(np.float32(0.1))).all() and (kn.count == 0).all()
    n, c = CL.estimate_normals(up(empty), radius=0.1)
    assert n.shape == (0, 3) and c.shape == (0,)
    out = CL.remove_outliers(up(empty), radius=0.1, min_neighbours=1)
    assert out.points.shape == (0, 3) and out.kept.shape == (0,) and out.keep.shape == (0,)


@pytest.mark.parametrize("k", [1, 4, 5, 8, 9, 16])
def test_knn_on_the_scene(k):
    """Every list capacity (4, 8, 16) and a k just above the one before; the floaters find fewer than k within the radius."""
    p = C.noisy(1000.0)
    full = C.knn(1000.0, 16, C.MAX_DIST_SHORT)  # a list of k is the head of the list of 16
    ref = CL.KNN(full.index[:, :k], full.dist[:, :k], np.minimum(full.count, k))
    assert (ref.count[C.N_SURFACE:] < k).any() or k == 1
    dev = CL.cloud_knn(up(p), k, C.MAX_DIST_SHORT)
    check_knn((dev.index, dev.dist, dev.count), ref)
    if k in (5, 16):
        lm = ops.cloud_list_moments(up(p), up(p), dev.index, dev.dist)
        check_moments(lm, CL.list_moments_numpy(p, None, ref.index, ref.dist))
        assert torch.equal(lm[0], dev.count)


def test_knn_ties_self_query_and_order():
    rng = np.random.default_rng(4)
    p = rng.uniform(0, 1, (300, 3)).astype(np.float32)
    p[[250, 17, 99, 180]] = p[40]  # exact duplicates: equal d2, the index decides
    p[5] = [np.nan, 0.5, 0.5]
    p[6] = [0.5, np.inf, 0.5]
    md = 0.2
    dev = CL.cloud_knn(up(p), 9, md)
    check_knn((dev.index, dev.dist, dev.count), CL.knn_numpy(p, 9, md))
    assert dev.index[40, :4].tolist() == [17, 99, 180, 250] and dev.index[17, :4].tolist() == [40, 99, 180, 250]
    assert (dev.dist[40, :4] == 0).all() and dev.count[5] == 0 and dev.count[6] == 0 and not np.isin(dev.index.cpu().numpy(), [5, 6]).any()
    # the same cloud given as target=: a point finds itself (or a duplicate of a smaller index) first
    twice = CL.cloud_knn(up(p), 9, md, target=up(p))
    check_knn((twice.index, twice.dist, twice.count), CL.knn_numpy(p, 9, md, p))
    assert twice.index[41, 0] == 41 and twice.index[250, 0] == 17
    # a shuffled query order gives the same rows
    order = rng.permutation(len(p))
    grid = grid_of(p, md)
    a, b = ops.cloud_knn(up(p), grid, 9, md), ops.cloud_knn(up(p[order]), grid, 9, md)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x)[order], bits(y))
    ra, rb = ops.cloud_radius_moments(up(p), grid, md), ops.cloud_radius_moments(up(p[order]), grid, md)
    for x, y in zip(ra, rb):
        assert np.array_equal(bits(x)[order], bits(y))


@pytest.mark.parametrize("offset", C.OFFSETS)
def test_normals(offset):
    p = C.noisy(offset)
    P = up(p)
    count, _, moments = ops.cloud_radius_moments(None, grid_of(p, C.RADIUS), C.RADIUS)
    cnt, mom = count.cpu().numpy(), moments.cpu().numpy()
    view = np.array([0.0, 0.0, 5.0]) + offset
    views = (p.astype(np.float64) + [0.3, -0.2, 2.0]).astype(np.float32)
    likes = np.tile(np.array([[0.1, 0.2, -1.0]], np.float32), (len(p), 1))
    ok = cnt >= 5
    assert 0 < (~ok).sum() < 100
    worst = {"normal": 0.0, "curvature": 0.0, "ratio": 0.0}
    for name, kw in (("none", {}), ("viewpoint", dict(toward=view)), ("viewpoints", dict(toward=views)), ("like", dict(like=likes))):
        dkw = {k: (up(v) if v.ndim == 2 else v) for k, v in kw.items()}
        n_dev, c_dev = (a.cpu().numpy() for a in ops.cloud_normals(P, count, moments, 5, **dkw))
        n_ref, c_ref = CL.normals_from_moments_numpy(p, cnt, mom, 5, **kw)
        assert np.array_equal((n_dev == 0).all(axis=1), ~ok) and np.array_equal(np.isnan(c_dev), ~ok)
        assert np.array_equal((n_ref == 0).all(axis=1), ~ok) and np.array_equal(np.isnan(c_ref), ~ok)
        a, b = n_dev[ok].astype(np.float64), n_ref[ok].astype(np.float64)
        err = np.minimum(np.linalg.norm(a - b, axis=1), np.linalg.norm(a + b, axis=1))  # before orientation: up to the sign
        cerr = np.abs(c_dev[ok].astype(np.float64) - c_ref[ok])
        worst = {"normal": max(worst["normal"], err.max()), "curvature": max(worst["curvature"], cerr.max()),
                 "ratio": max(worst["ratio"], (cerr / (2.0 ** -23 * c_ref[ok] + 1e-12)).max())}
        assert (err <= 2.0 ** -22).all() and (cerr <= 2.0 ** -23 * c_ref[ok] + 1e-12).all()
        # after orientation: the signs agree, except where the deciding dot is within 2^-22 (times the norms) of zero: nowhere here
        if name == "none":
            w = np.zeros_like(b)
            w[np.arange(len(b)), np.abs(b).argmax(axis=1)] = 1.0
            top = np.sort(np.abs(b), axis=1)
            unclear = top[:, 2] - top[:, 1] <= 2.0 ** -22  # two components of equal magnitude: either may lead
        else:
            w = view - p[ok].astype(np.float64) if name == "viewpoint" else (views[ok].astype(np.float64) - p[ok].astype(np.float64)
                                                                           if name == "viewpoints" else likes[ok].astype(np.float64))
            unclear = np.abs((b * w).sum(axis=1)) <= 2.0 ** -22 * np.linalg.norm(w, axis=1)
        assert not unclear.any()
        assert ((a * b).sum(axis=1) > 0).all() and ((b * w).sum(axis=1) > 0).all()
    print(f"\noffset {offset}: largest |n_dev -+ n_ref| {worst['normal']:.3e} (bound {2.0 ** -22:.3e}), largest curvature error "
          f"{worst['curvature']:.3e} = {worst['ratio']:.4f} of its bound")
    # the front end: radius and k paths against the host's, under the same comparison
    for kw in (dict(radius=C.RADIUS), dict(k=16, max_dist=0.3)):
        n_dev, c_dev = (a.cpu().numpy() for a in CL.estimate_normals(P, toward=up(view.astype(np.float32)) if "k" in kw else view, **kw))
        n_ref, c_ref = CL.estimate_normals_numpy(p, toward=view.astype(np.float32) if "k" in kw else view, **kw)
        good = ~np.isnan(c_ref)
        assert np.array_equal(np.isnan(c_dev), ~good) and np.array_equal((n_dev == 0).all(axis=1), ~good)
        assert (np.linalg.norm(n_dev[good].astype(np.float64) - n_ref[good], axis=1) <= 2.0 ** -22).all()
        assert (np.abs(c_dev[good].astype(np.float64) - c_ref[good]) <= 2.0 ** -23 * c_ref[good] + 1e-12).all()


def test_degenerate_normals():
    f = np.float32
    line = np.stack([np.linspace(0, 0.05, 8), np.zeros(8), np.zeros(8)], axis=1).astype(f)
    dup = np.tile(np.array([[0.3, 0.3, 0.3]], f), (8, 1))
    few = np.array([[0.6, 0.6, 0.6], [0.61, 0.6, 0.6], [0.6, 0.61, 0.6], [0.6, 0.6, 0.61]], f)
    rng = np.random.default_rng(2)
    plane = np.column_stack([rng.uniform(0.8, 0.9, (12, 2)), np.full(12, 0.5)]).astype(f)
    p = np.concatenate([line, dup, few, plane, np.array([[np.nan, 0.85, 0.5]], f)])
    n, c = (a.cpu().numpy() for a in CL.estimate_normals(up(p), radius=0.2))
    assert (n[:20] == 0).all() and np.isnan(c[:20]).all() and (n[32] == 0).all() and np.isnan(c[32])
    assert np.array_equal(n[20:32], np.tile(np.array([[0, 0, 1]], f), (12, 1))) and (np.abs(c[20:32]) < 1e-12).all()
    # the orientation tie (a viewpoint in the plane, reference normals in it or invalid): the largest component decides
    like = np.tile(np.array([[1, 0, 0]], f), (len(p), 1))
    for kw in (dict(toward=(0.85, 0.85, 0.5)), dict(like=up(like)), dict(like=up(np.full_like(like, np.nan)))):
        tie, _ = CL.estimate_normals(up(p), radius=0.2, **kw)
        assert np.array_equal(tie.cpu().numpy()[20:32], n[20:32])
    below, _ = CL.estimate_normals(up(p), radius=0.2, toward=(0.85, 0.85, -3.0))
    assert np.array_equal(below.cpu().numpy()[20:32], -n[20:32])


def check_outliers(dev, ref):
    assert dev.keep.dtype == torch.bool and dev.kept.dtype == torch.int32
    assert np.array_equal(dev.keep.cpu().numpy(), ref.keep) and np.array_equal(dev.kept.cpu().numpy(), ref.kept)
    assert dev.threshold == ref.threshold
    for got, want in ((dev.points, ref.points), (dev.colors, ref.colors), (dev.normals, ref.normals)):
        assert (got is None) == (want is None) and (got is None or (got.shape == want.shape and same_bits(got, want)))


@pytest.mark.parametrize("rule", ["density", "short", "long"])
@pytest.mark.parametrize("offset", C.OFFSETS)
def test_outliers_on_the_scene(offset, rule):
    p = C.noisy(offset)
    ref = C.outliers(offset, rule)
    dev = CL.remove_outliers(up(p), up(p), up(-p), **C.arguments(rule))
    check_outliers(dev, ref)
    assert not ref.keep[C.N_SURFACE:].any() and (rule == "short" or ref.keep[:C.N_SURFACE].all())
    if rule == "long":
        assert abs(dev.threshold - 0.1448) < 1e-3
    if offset == 0.0:  # without the attributes: the same points
        bare = CL.remove_outliers(up(p), **C.arguments(rule))
        assert bare.colors is None and bare.normals is None and same_bits(bare.points, ref.points)


def test_outliers_all_none_one_and_invalid():
    p = C.noisy(0.0)[:700].copy()
    p[13] = [np.nan, 0, 0]
    p[500] = [0, 0, np.inf]
    for kw in (dict(radius=0.08, min_neighbours=0), dict(radius=0.08, min_neighbours=10 ** 6), dict(radius=0.08, min_neighbours=3),
               dict(k=1, std_ratio=1e9, max_dist=3.0), dict(k=16, std_ratio=0.0, max_dist=0.05), dict(k=4, std_ratio=-1.0, max_dist=0.5)):
        ref = CL.remove_outliers_numpy(p, p, **kw)
        check_outliers(CL.remove_outliers(up(p), up(p), **kw), ref)
        assert not ref.keep[13] and not ref.keep[500]
    assert CL.remove_outliers_numpy(p, radius=0.08, min_neighbours=0).keep.sum() == 698 == CL.remove_outliers_numpy(p, k=1, std_ratio=1e9, max_dist=3.0).keep.sum()
    assert CL.remove_outliers_numpy(p, radius=0.08, min_neighbours=10 ** 6).keep.sum() == 0
    one = p[:1]
    for kw in (dict(radius=0.08, min_neighbours=0), dict(radius=0.08, min_neighbours=1), dict(k=1, std_ratio=1.0, max_dist=0.1)):
        check_outliers(CL.remove_outliers(up(one), **kw), CL.remove_outliers_numpy(one, **kw))
    # a keep mask across many chunks of the compaction: 70000 points, every third kept
    keep = (torch.arange(70000, device=DEV) % 3 == 0).to(torch.uint8)
    kept, remap, K = ops.cloud_select(keep)
    assert K == 23334 and torch.equal(kept, torch.arange(0, 70000, 3, device=DEV, dtype=torch.int32))
    assert torch.equal(remap[::3], torch.arange(K, device=DEV, dtype=torch.int32)) and (remap[1::3] == -1).all() and (remap[2::3] == -1).all()


def test_spacing():
    p = C.noisy(1000.0)
    host, dev = CL.cloud_spacing(p, 0.5), CL.cloud_spacing(up(p), 0.5)
    assert abs(dev - host) <= len(p) * 2.0 ** -53 * host and 0.015 < host < 0.025
    few = np.array([[0, 0, 0], [0.03, 0.04, 0], [np.nan, 0, 0], [5, 5, 5]], np.float32)
    assert abs(CL.cloud_spacing(up(few), 0.1) - 0.05) < 1e-8 and np.isnan(CL.cloud_spacing(up(few[2:]), 0.1))


def test_two_calls_give_the_same_bits():
    p = up(C.noisy(1000.0))
    grid = grid_of(C.noisy(1000.0), C.RADIUS)
    def run():
        nb = ops.cloud_radius_moments(None, grid, C.RADIUS)
        kn = ops.cloud_knn(None, grid, 8, C.RADIUS)
        lm = ops.cloud_list_moments(p, p, kn[0], kn[1])
        nr = ops.cloud_normals(p, nb[0], nb[2], 5, toward=(0.0, 0.0, 1005.0))
        mean, block = ops.cloud_knn_mean_sums(kn[1], kn[2])
        keep = ops.cloud_keep_density(p, nb[0], 9)
        kept, remap, _ = ops.cloud_select(keep)
        return nb + kn + lm + nr + (mean, block, keep, ops.cloud_keep_threshold(mean, 0.05), kept, remap)
    for a, b in zip(run(), run()):
        assert same_bits(a, b)


def test_evaluation_on_the_device_equals_the_host_path():
    """PointCloudEvaluation(clean=..., align="plane", gt_normals="estimate") on GPU tensors against the host path, compared as
    test_hip_cloud_eval.py compares the two: the band 4 x |d32 - d64| of the distance chain, here widened by twice the registration's
    stopping tolerance (each path stops when its step is at most tol, so each aligned cloud is within about a step of the fixed point
    both iterate towards); a query whose distance is within that of max_dist or of a threshold may fall on either side."""
    q, gt = CC.scene_s(0.0)
    pred = np.concatenate([(q[:600].astype(np.float64) + [0.004, -0.003, 0.005]).astype(np.float32), C.noisy(0.0)[C.N_SURFACE:]])
    ev = CE.PointCloudEvaluation(CC.S_THRESHOLDS, CC.S_MAX_DIST, align="plane", gt_normals="estimate", clean=dict(radius=0.2, min_neighbours=3))
    host, dev = ev(pred, gt, pred), ev(up(pred), up(gt), up(pred))
    assert dev.dist_pred.is_cuda and dev.pred_points.is_cuda and dev.pred_colors.is_cuda
    assert host.n_removed == dev.n_removed and 40 <= host.n_removed < 100 and (dev.n_pred, dev.n_gt) == (host.n_pred, host.n_gt)
    assert same_bits(dev.pred_colors, host.pred_colors)  # the same points survive the filter
    assert host.registration.converged and dev.registration.converged
    tol = max(1e-3 * ev.align_max_dist[-1], 2.0 ** -21 * float(np.abs(gt).max()))
    moved = np.abs(dev.pred_points.cpu().numpy().astype(np.float64) - host.pred_points).max()
    print(f"\naligned clouds differ by at most {moved:.2e}; the registration's tolerance {tol:.2e}")
    assert moved <= 2 * tol
    for a, b, got_d, got_h, mean_d, mean_h, share_d, share_h in (
            (host.pred_points, gt, dev.dist_pred, host.dist_pred, dev.accuracy, host.accuracy, dev.precision, host.precision),
            (gt, host.pred_points, dev.dist_gt, host.dist_gt, dev.completeness, host.completeness, dev.recall, host.recall)):
        raw64, _ = CE.nearest_numpy(a, b, np.inf)
        raw32, _ = CE.nearest_numpy(a, b, np.inf, dtype=np.float32)
        both = (raw64 < CC.S_MAX_DIST) & (raw32 < CC.S_MAX_DIST)
        band = 4.0 * float(np.abs(raw32.astype(np.float64) - raw64)[both].max()) + 2 * tol
        excluded = np.zeros(len(a), dtype=bool)
        for edge in (CC.S_MAX_DIST,) + CC.S_THRESHOLDS:
            excluded |= np.abs(raw64 - np.float64(np.float32(edge))) <= band
        assert excluded.mean() < 0.05
        assert np.abs(got_d.cpu().numpy().astype(np.float64) - got_h)[~excluded].max() <= band
        assert abs(mean_d - mean_h) <= band + excluded.mean() * CC.S_MAX_DIST
        assert (np.abs(share_d - share_h) * len(a) <= excluded.sum() + 1e-9).all()


def test_wrapper_errors():
    p = up(C.noisy(0.0))
    grid = ops.cloud_grid(p, (-1, -1, -1), 0.08)
    with pytest.raises(ValueError, match=r"below radius \* \(1 \+ 2\^-10\)"):
        ops.cloud_radius_moments(None, grid, 0.08)
    with pytest.raises(ValueError, match=r"below max_dist \* \(1 \+ 2\^-10\)"):
        ops.cloud_knn(None, grid, 4, 0.08)
    for k in (0, 17):
        with pytest.raises(ValueError, match=r"supported 1\.\.16"):
            ops.cloud_knn(None, grid, k, 0.05)
        with pytest.raises(ValueError, match=r"supported 1\.\.16"):
            CL.cloud_knn(p, k, 0.05)
    with pytest.raises(ValueError, match="CloudGrid"):
        ops.cloud_radius_moments(p, p, 0.05)
    with pytest.raises(ValueError, match="cuda"):
        ops.cloud_radius_moments(p.cpu(), grid, 0.05)
    with pytest.raises(ValueError, match="different places"):
        CL.cloud_knn(p, 4, 0.05, target=p.cpu())
    with pytest.raises(ValueError, match="different places"):
        CL.remove_outliers(p, p.cpu(), radius=0.05, min_neighbours=1)
    with pytest.raises(ValueError, match="finite and > 0"):
        ops.cloud_knn(None, grid, 4, -1.0)
    with pytest.raises(ValueError, match="shape"):
        ops.cloud_normals(p, torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros((4, 9), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="at least 2"):
        ops.cloud_normals(p[:4], torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros((4, 9), dtype=torch.float64, device=DEV), 1)
    with pytest.raises(ValueError, match="dtype"):
        ops.cloud_select(torch.zeros(4, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match=r"each must be in \[0, 2097151\)"):
        CL.cloud_neighbourhood(p, 1e-7)
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.cloud_radius_moments(p.clone().requires_grad_(), grid, 0.05)
    lib = ops.L.load()  # the C entries check for themselves
    assert lib.mvd_cloud_knn_f32(None, 0, None, None, 0, 0.0, 0.0, 0.0, 1.0, 0.5, 17, 0, None, None, None, None) != 0
    assert b"supported 1..16" in lib.mvd_last_error()
    assert lib.mvd_cloud_radius_moments_f32(None, 0, None, None, 0, 0.0, 0.0, 0.0, 1.0, 1.0, 0, None, None, None, None) != 0
    assert b"below radius" in lib.mvd_last_error()
