"""GPU checks of the point-cloud evaluation kernels (csrc/cloud_eval.hip) and of PointCloudEvaluation / evaluate_scene on GPU tensors,
on the clouds of cloud_cases.py.  The reference project has no counterpart: the yardstick is cloud_eval.nearest_numpy in float64
(itself checked against a k-d tree in test_cloud_eval_cpu.py).

Nearest kernel against the definition (scene S at both offsets, both directions).  The band comes from the reference side alone
(cloud_cases.reference): the largest |d32 - d64| between nearest_numpy in float64 and the same chain in float32, over the queries
untruncated in both, times four: the kernel may contract to FMAs, add the three squares in another order and use a 1-ulp sqrt, each
about one more float32 rounding of the same chain.  A query whose float64 untruncated distance is within the band of max_dist or of a
threshold is left out of the verdict comparisons; at most 0.5 % of a case may be left out.  On the rest: |dist - d64| <= band, the
truncation agrees, the float64 distance to P[index] is <= d64 + band, and dist == max_dist exactly where index == -1.

Measured (gap, band and excluded share from the two numpy chains alone; the kernel's column on an MI355X):
    case               gap        band       excluded  kernel: max |dist - d64|   wrong verdicts
    S +0    q -> t     2.00e-09   8.01e-09   0.000 %   1.88e-09                   0
    S +0    t -> q     2.33e-09   9.33e-09   0.000 %   1.84e-09                   0
    S +1000 q -> t     9.30e-10   3.72e-09   0.000 %   9.30e-10                   0
    S +1000 t -> q     9.30e-10   3.72e-09   0.000 %   9.30e-10                   0
    clustered          1.43e-10   5.74e-10   0.000 %   1.43e-10                   0
9-17 % of a case's queries are truncated and 15-20 % are under 0.01, so both verdicts are decided in every case.
"""
import numpy as np
import pytest
import torch

import cloud_cases as CC
import fusion_cases as FC
from robustmvd_amd import cloud_eval as CE
from robustmvd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_EXCLUDED_SHARE = 0.005


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_nearest(q, p, max_dist, origin=None):
    """nearest_numpy's arguments -> (dist, index) numpy, from the kernels: a grid over the targets from the clouds' common minimum"""
    q, p = np.asarray(q, dtype=np.float32).reshape(-1, 3), np.asarray(p, dtype=np.float32).reshape(-1, 3)
    if origin is None:
        both = np.concatenate([q, p])
        both = both[np.isfinite(both).all(axis=1)]
        origin = both.min(axis=0).astype(np.float64) if len(both) else np.zeros(3)
    grid = ops.cloud_grid(up(p), origin, float(np.float32(max_dist)) * ops.CLOUD_CELL_MARGIN)
    dist, index = ops.cloud_nearest(up(q), grid, max_dist)
    assert dist.dtype == torch.float32 and index.dtype == torch.int32 and dist.shape == index.shape == (len(q),)
    return dist.cpu().numpy(), index.cpu().numpy()


def check_against(ref, dist, index, label):
    """The issue's four assertions on the queries that are not excluded; prints the figures first."""
    q, p, md, band, keep = ref["q"], ref["p"], ref["max_dist"], ref["band"], ~ref["excluded"]
    diff = np.abs(dist.astype(np.float64) - ref["d64"])
    wrong = int(((index >= 0) != (ref["i64"] >= 0))[keep].sum())
    print(f"\n{label}: gap {ref['gap']:.2e}, band {band:.2e}, excluded {100 * ref['share']:.3f} %; kernel: max |dist - d64| "
          f"{diff[keep].max():.2e}, wrong verdicts {wrong}, found {100 * (index >= 0).mean():.1f} %")
    assert ref["share"] <= MAX_EXCLUDED_SHARE
    assert (diff[keep] <= band).all()
    assert wrong == 0
    found = index >= 0
    assert (index[found] < len(p)).all()
    own = np.linalg.norm(q[found].astype(np.float64) - p[index[found]].astype(np.float64), axis=1)
    assert (own <= ref["raw64"][found] + band).all()
    assert (dist[~found] == md).all() and (dist[found] < md).all()


def check_small(q, p, md, d64, raw, dist, index):
    """For the small random clouds in the unit cube: distances below 0.2 from coordinate differences with at most half an ulp of 0.2
    (7.5e-9) of error each, and some eight float32 roundings of the chain, stay within 1e-7 of the float64 value.  Queries within
    that of max_dist are left to either verdict."""
    tol = 1e-7
    clear = np.abs(raw - np.float64(np.float32(md))) > tol
    assert clear.mean() > 0.95 or len(q) < 64
    assert np.array_equal((index >= 0)[clear], (d64 < np.float32(md))[clear])
    assert (np.abs(dist - d64)[clear] <= tol).all()
    found = index >= 0
    own = np.linalg.norm(q[found].astype(np.float64) - p[index[found]].astype(np.float64), axis=1)
    assert (own <= raw[found] + tol).all() and (dist[~found] == np.float32(md)).all()


S_CASES = [(o, d) for o in CC.S_OFFSETS for d in ("qt", "tq")]


@pytest.mark.parametrize("offset,direction", S_CASES, ids=[f"S+{int(o)}-{d}" for o, d in S_CASES])
def test_nearest_kernel_against_the_definition(offset, direction):
    ref = CC.reference(("S", offset, direction), CC.S_MAX_DIST, CC.S_THRESHOLDS)
    dist, index = device_nearest(ref["q"], ref["p"], CC.S_MAX_DIST)
    check_against(ref, dist, index, f"S +{int(offset)} {direction}")
    assert 0.03 < (index < 0).mean() < 0.5  # both outcomes occur
    # the verdicts at the thresholds, on the queries that are not excluded
    keep = ~ref["excluded"]
    for tau in np.float32(CC.S_THRESHOLDS):
        assert np.array_equal((dist < tau)[keep], (ref["d64"] < tau)[keep])


@pytest.mark.parametrize("base", CC.B_BASES)
def test_boundary(base):
    """A target a hair inside max_dist, on a cell corner's far side in every one of the 26 directions, is found; a hair outside, truncated."""
    for sign in "-+":
        ref = CC.reference(("B", base, sign), CC.B_MAX_DIST)
        assert not ref["excluded"].any() and ((ref["i64"] >= 0) == (sign == "-")).all()  # the reference decides all 26
        dist, index = device_nearest(ref["q"], ref["p"], CC.B_MAX_DIST, origin=np.full(3, base))  # the queries ON cell corners
        if sign == "-":
            assert np.array_equal(index, np.arange(26))
            assert (dist < np.float32(CC.B_MAX_DIST)).all() and (dist > np.float32(CC.B_MAX_DIST) * (1 - 2.0 ** -10)).all()
        else:
            assert (index == -1).all() and (dist == np.float32(CC.B_MAX_DIST)).all()


def test_clustered():
    """5000 targets in one cell: the staging is chunked, not sized by the cell; the far queries find nothing."""
    ref = CC.reference(("C",), CC.C_MAX_DIST)
    dist, index = device_nearest(ref["q"], ref["p"], CC.C_MAX_DIST, origin=np.zeros(3))
    check_against(ref, dist, index, "clustered")
    assert (index[:70] >= 0).all() and (index[70:] == -1).all()


@pytest.mark.parametrize("m", [1, 2, 1000])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes(n, m):
    rng = np.random.default_rng(1000 * n + m)
    q, p = rng.uniform(0, 1, (n, 3)).astype(np.float32), rng.uniform(0, 1, (m, 3)).astype(np.float32)
    md = 0.15
    d64, i64 = CE.nearest_numpy(q, p, md)
    raw, _ = CE.nearest_numpy(q, p, np.inf)
    dist, index = device_nearest(q, p, md)
    check_small(q, p, md, d64, raw, dist, index)


def test_empty_inputs():
    q = np.random.default_rng(0).uniform(0, 1, (70, 3)).astype(np.float32)
    dist, index = device_nearest(np.zeros((0, 3)), q, 0.1)
    assert dist.shape == (0,) and index.shape == (0,)
    dist, index = device_nearest(q, np.zeros((0, 3)), 0.1)
    assert (dist == np.float32(0.1)).all() and (index == -1).all()


def test_duplicates_and_invalid_points():
    rng = np.random.default_rng(4)
    p = rng.uniform(0, 1, (300, 3)).astype(np.float32)
    p[[250, 17, 99, 180]] = p[40]  # exact duplicates of one target: the smallest index, 17, wins
    p[5] = [np.nan, 0.5, 0.5]
    p[6] = [0.5, np.inf, 0.5]
    p[7] = [0.5, 0.5, -np.inf]
    q = rng.uniform(0, 1, (200, 3)).astype(np.float32)
    q[0] = p[40]
    q[1] = [np.nan, 0.1, 0.1]
    q[2] = [0.1, np.inf, 0.1]
    q[3] = [0.5, 0.5, 0.5]
    md = 0.2
    d64, i64 = CE.nearest_numpy(q, p, md)
    raw, _ = CE.nearest_numpy(q, p, np.inf)
    assert i64[0] == 17 and (i64[1:3] == -1).all()
    dist, index = device_nearest(q, p, md)
    assert index[0] == 17 and dist[0] == 0
    assert (index[1:3] == -1).all() and (dist[1:3] == np.float32(md)).all()
    assert not np.isin(index, [5, 6, 7]).any()
    check_small(q, p, md, d64, raw, dist, index)
    only_bad = p[5:8]
    dist, index = device_nearest(q, only_bad, md, origin=np.zeros(3))
    assert (index == -1).all() and (dist == np.float32(md)).all()


def test_nearest_is_deterministic_and_order_free():
    q, p = CC.scene_s(1000.0)
    a, b = device_nearest(q, p, CC.S_MAX_DIST), device_nearest(q, p, CC.S_MAX_DIST)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    # both clouds as grids of one origin, as PointCloudEvaluation runs them: the same bits
    origin = np.minimum(q.min(0), p.min(0)).astype(np.float64)
    cell = float(np.float32(CC.S_MAX_DIST)) * ops.CLOUD_CELL_MARGIN
    gq, gp = ops.cloud_grid(up(q), origin, cell), ops.cloud_grid(up(p), origin, cell)
    d, i = ops.cloud_nearest(gq, gp, CC.S_MAX_DIST)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), a[0].view(np.uint32)) and np.array_equal(i.cpu().numpy(), a[1])
    keys = gp.keys.cpu().numpy()
    assert (np.diff(keys) >= 0).all() and gp.records.shape == (4000, 4)
    perm = gp.records[:, 3].contiguous().view(torch.int32).cpu().numpy()
    assert np.array_equal(np.sort(perm), np.arange(4000)) and np.array_equal(gp.records[:, :3].cpu().numpy(), p[perm])


def test_wrapper_errors():
    p = up(CC.scene_s(0.0)[1])
    with pytest.raises(ValueError, match=r"each must be in \[0, 2097151\)"):
        ops.cloud_grid(p, (-1, -1, -1), 1e-7)
    with pytest.raises(ValueError, match="indices -"):
        ops.cloud_grid(p, (0, 0, 0), 0.1)
    grid = ops.cloud_grid(p, (-1, -1, -1), 0.03)
    with pytest.raises(ValueError, match="below max_dist"):
        ops.cloud_nearest(p, grid, 0.03)
    with pytest.raises(ValueError, match=r"\(n,3\)"):
        ops.cloud_nearest(p[:, :2], grid, 0.01)
    with pytest.raises(ValueError, match="cuda"):
        ops.cloud_nearest(p.cpu(), grid, 0.01)
    with pytest.raises(ValueError, match="CloudGrid"):
        ops.cloud_nearest(p, p, 0.01)
    with pytest.raises(ValueError, match="9 thresholds"):
        ops.cloud_scores(torch.zeros(4, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV), np.linspace(0.1, 0.9, 9))
    with pytest.raises(ValueError, match="dtype"):
        ops.cloud_scores(torch.zeros(4, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), (0.1,))
    with pytest.raises(ValueError, match=r"each must be in \[0, 2097151\)"):
        ops.voxel_downsample(p, 1e-7)
    with pytest.raises(ValueError, match="shape"):
        ops.voxel_downsample(p, 0.1, colors=p[:-1])
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.voxel_downsample(p.clone().requires_grad_(), 0.1)


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("n", [1, 65, 3000])
def test_scores_kernel(n, T):
    """Against numpy on the device's own dist array: the counts exactly, the sum within n 2^-53 relative (any order of non-negative
    float64 terms is within that of any other)."""
    q, p = CC.scene_s(0.0)
    q = q[:n].copy()
    if n > 10:
        q[3] = [np.nan, 0, 0]  # an invalid query: truncated and not counted
        q[n - 1] = [0, np.inf, 0]
    th = np.float32(np.linspace(0.004, CC.S_MAX_DIST, T))
    grid = ops.cloud_grid(up(p), p.min(0).astype(np.float64) - 0.1, float(np.float32(CC.S_MAX_DIST)) * ops.CLOUD_CELL_MARGIN)
    dist, index = ops.cloud_nearest(up(q), grid, CC.S_MAX_DIST)
    block = ops.cloud_scores(dist, index, th, up(q))
    total, valid, counts = ops.cloud_scores_read(block, T)
    ok = np.isfinite(q).all(axis=1)
    d = dist.cpu().numpy()[ok]
    assert valid == ok.sum() == (n if n <= 10 else n - 2)
    assert np.array_equal(counts, [(d < t).sum() for t in th]) and counts.dtype == np.int64
    assert (block[2 + T:].cpu().numpy() == 0).all()
    want = d.astype(np.float64).sum()
    assert abs(total - want) <= n * 2.0 ** -53 * want
    if n == 3000 and T == 8:
        assert 0 < counts[0] < counts[-1] < valid
    # without the points every query counts; twice the same bits
    every = ops.cloud_scores_read(ops.cloud_scores(dist, index, th), T)
    assert every[1] == n
    assert torch.equal(block, ops.cloud_scores(dist, index, th, up(q)))


def voxel_points(case):
    rng = np.random.default_rng(12)
    if case[0] == "n" and case[1:].isdigit():
        return rng.uniform(-1, 1, (int(case[1:]), 3)).astype(np.float32), 0.25, None
    if case == "n70000-fine":  # nearly every point its own voxel: every one of the 274 chunks of 256 keys adds to the scan
        return rng.uniform(-1, 1, (70000, 3)).astype(np.float32), 0.02, None
    if case == "one-voxel":
        return rng.uniform(0.01, 0.99, (5000, 3)).astype(np.float32), 1.0, (0, 0, 0)
    if case == "own-voxel":
        g = np.stack(np.meshgrid(*[np.arange(17)] * 3, indexing="ij"), -1).reshape(-1, 3)
        return rng.permutation((g + 0.5).astype(np.float32) * np.float32(0.5)), 0.5, (0, 0, 0)
    if case == "faces-pow2":
        return CC.voxel_faces(2.0 ** -4), 2.0 ** -4, (0, 0, 0)
    if case == "faces-0.01":
        return CC.voxel_faces(0.01), 0.01, (0, 0, 0)
    if case == "negative":
        return CC.voxel_faces(0.01, negative=True), 0.01, None
    if case == "negative-origin":
        return CC.voxel_faces(2.0 ** -4, negative=True), 2.0 ** -4, (-1.5, -1, -2)
    assert case == "invalid"
    pts = CC.voxel_faces(0.125).copy()
    pts[::7, 0] = np.nan
    pts[3::11, 2] = np.inf
    return pts, 0.125, (0, 0, 0)


@pytest.mark.parametrize("case", ["n1", "n64", "n65", "n5000", "n70000", "n70000-fine", "one-voxel", "own-voxel", "faces-pow2",
                                  "faces-0.01", "negative", "negative-origin", "invalid"])
def test_voxel_kernel(case):
    """Voxel order and counts exactly; coordinates and colours within 1 float32 ulp of the float64 mean rounded to float32.
    n70000 (274 chunks of 256 keys) is the smallest round size at which a lane of the one-workgroup scan (csrc/compact.h) takes two
    counts; its 512 voxels of about 137 points also take the wave-wide sum."""
    pts, voxel, origin = voxel_points(case)
    col = np.random.default_rng(8).uniform(0, 255, pts.shape).astype(np.float32)
    wx, wr, wc = CE.voxel_downsample_numpy(pts, voxel, col, origin)
    xyz, rgb, counts = ops.voxel_downsample(up(pts), voxel, up(col), origin)
    assert xyz.dtype == torch.float32 and counts.dtype == torch.int32 and xyz.shape == (len(wc), 3) == rgb.shape
    assert np.array_equal(counts.cpu().numpy(), wc)
    if case == "one-voxel":
        assert wc.tolist() == [5000]
    if case == "own-voxel":
        assert (wc == 1).all() and len(wc) == 17 ** 3
    if case == "invalid":
        assert wc.sum() == np.isfinite(pts).all(1).sum() < len(pts)
    for got, want in ((xyz, wx), (rgb, wr)):
        got = got.cpu().numpy()
        assert (np.abs(got - want) <= np.spacing(np.abs(want))).all()
    # twice the same bits, and the same voxels without colours
    again = ops.voxel_downsample(up(pts), voxel, up(col), origin)
    for a, b in zip((xyz, rgb, counts), again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    x2, r2, c2 = ops.voxel_downsample(up(pts), voxel, None, origin)
    assert r2 is None and torch.equal(x2.view(torch.int32), xyz.view(torch.int32)) and torch.equal(c2, counts)


def test_evaluation_on_the_device_equals_the_host_path():
    q, p = CC.scene_s(1000.0)
    ev = CE.PointCloudEvaluation(CC.S_THRESHOLDS, CC.S_MAX_DIST)
    host, dev = ev(q, p), ev(up(q), up(p))
    assert dev.dist_pred.is_cuda and dev.dist_gt.is_cuda and dev.pred_points.is_cuda
    fwd = CC.reference(("S", 1000.0, "qt"), CC.S_MAX_DIST, CC.S_THRESHOLDS)
    back = CC.reference(("S", 1000.0, "tq"), CC.S_MAX_DIST, CC.S_THRESHOLDS)
    assert (dev.n_pred, dev.n_gt) == (host.n_pred, host.n_gt) == (3000, 4000)
    for ref, got, n, mean_dev, mean_host, share_dev, share_host in (
            (fwd, dev.dist_pred, 3000, dev.accuracy, host.accuracy, dev.precision, host.precision),
            (back, dev.dist_gt, 4000, dev.completeness, host.completeness, dev.recall, host.recall)):
        assert np.abs(got.cpu().numpy() - ref["d64"])[~ref["excluded"]].max() <= ref["band"]
        assert abs(mean_dev - mean_host) <= ref["band"] + ref["excluded"].mean() * CC.S_MAX_DIST
        assert (np.abs(share_dev - share_host) * n <= ref["excluded"].sum() + 1e-9).all()  # the counts differ only by the excluded
    np.testing.assert_allclose(dev.overall, (dev.accuracy + dev.completeness) / 2, rtol=1e-15)
    P, Rc = dev.precision, dev.recall
    np.testing.assert_allclose(dev.fscore, 2 * P * Rc / (P + Rc), rtol=1e-15)
    # thinned: the device's voxels are the host's, the scores follow
    # (at offset 0: a voxel mean may differ by one float32 ulp, 1.2e-7 there, and the distances with it)
    thin = CE.PointCloudEvaluation(CC.S_THRESHOLDS, CC.S_MAX_DIST, voxel=0.05)
    q0, p0 = CC.scene_s(0.0)
    a, b = thin(q0, p0, q0), thin(up(q0), up(p0), up(q0))
    assert a.n_pred == b.n_pred < 3000 and b.pred_colors.is_cuda
    assert np.abs(b.pred_points.cpu().numpy() - a.pred_points).max() <= 2.0 ** -23
    assert abs(a.accuracy - b.accuracy) < 1e-6 and np.abs(a.precision - b.precision).max() <= 3 / a.n_pred
    with pytest.raises(ValueError, match="different places"):
        ev(up(q), p)


def test_evaluate_scene_on_the_device():
    H, W = FC.SIZES[0]
    sc = FC.scene("B", H, W)
    g = np.linspace(-2.5, 2.5, 126)
    gx, gy = np.meshgrid(g, g)
    gt = np.stack([gx.ravel(), gy.ravel(), (FC.PLANE_D - FC.PLANE_N[0] * gx.ravel() - FC.PLANE_N[1] * gy.ravel()) / FC.PLANE_N[2]],
                  axis=1).astype(np.float32)
    score = CE.evaluate_scene(FC.StubModel(H, W), sc["images"], sc["Ks"], sc["Ts"], up(gt), thresholds=(0.02, 0.05))
    assert score.dist_pred.is_cuda and score.pred_points.is_cuda and score.pred_colors.is_cuda
    host = CE.evaluate_scene(FC.StubModel(H, W), sc["images"], sc["Ks"], sc["Ts"], gt, thresholds=(0.02, 0.05))
    assert score.n_pred > 500 and abs(score.n_pred - host.n_pred) <= 0.01 * host.n_pred  # the fusion's verdicts differ within its bands
    assert score.precision[1] == 1.0 and abs(score.accuracy - host.accuracy) < 1e-3 and np.abs(score.recall - host.recall).max() < 0.01
    # a model on the GPU and a ground truth on the host: the ground truth follows the fused cloud
    moved = CE.evaluate_scene(FC.StubModel(H, W, param=torch.zeros(1, device=DEV)), sc["images"], sc["Ks"], sc["Ts"], gt,
                              thresholds=(0.02, 0.05))
    assert moved.dist_gt.is_cuda and moved.accuracy == score.accuracy and np.array_equal(moved.fscore, score.fscore)
