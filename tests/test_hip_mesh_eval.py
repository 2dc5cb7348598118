"""GPU checks of the mesh-evaluation kernels (csrc/mesh_eval.hip) and of MeshEvaluation / Mesh.distance / Mesh.sample on GPU tensors,
on the meshes of mesh_eval_cases.py.  The reference project has no counterpart: the yardstick is mesh_eval.mesh_distance_numpy in
float64 (itself checked against dense barycentric sampling in test_mesh_eval_cpu.py), mesh_grid_pairs_numpy and sample_mesh_numpy.

Nearest kernel against the definition.  The band comes from the reference side alone (mesh_eval_cases.reference): the largest
|d32 - d64| between mesh_distance_numpy in float64 and the same chain in float32, over the queries untruncated in both, times four:
the kernel may contract to FMAs, add the three-term sums in another order and use a 1-ulp sqrt and division, each about one more
float32 rounding of the same chain.  A query whose float64 untruncated distance is within the band of max_dist or of a threshold is
left out of the verdict comparisons; at most 0.5 % of a case may be left out.  On the rest: |dist - d64| <= band, the truncation
agrees, the float64 distance to triangle `index` is <= d64 + band (the winning triangle may differ at a shared edge), dist == max_dist
exactly where index == -1, and the threshold verdicts agree.  The pair list and the samples are compared bit for bit.

Measured (gap, band and excluded share from the two numpy chains alone; the kernel's column on an MI355X):
    case            gap        band       excluded  kernel: max |dist - d64|   wrong verdicts
    sphere +0       6.38e-09   2.55e-08   0.000 %   5.64e-09                   0
    sphere +1000    5.14e-09   2.06e-08   0.000 %   8.11e-09                   0
    crowded         3.49e-10   1.40e-09   0.000 %   3.49e-10                   0
    quad            3.73e-09   1.49e-08   0.000 %   3.73e-09                   0
    sphere+quad     6.38e-09   2.55e-08   0.000 %   5.64e-09                   0
    degenerate      2.11e-08   8.44e-08   0.000 %   2.38e-08                   0
14 % of the sphere's queries are truncated and 34.5 % are under 0.01, so every verdict is decided in both directions.
"""
import numpy as np
import pytest
import torch

import mesh_eval_cases as MC
import render_cases as RC
import tsdf_cases as TC
import robustmvd_amd as R
from robustmvd_amd import cloud_eval as CE
from robustmvd_amd import mesh_eval as ME
from robustmvd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def common_origin(*clouds):
    both = np.concatenate([np.asarray(c, dtype=np.float32).reshape(-1, 3) for c in clouds])
    both = both[np.isfinite(both).all(axis=1)]
    return both.min(axis=0).astype(np.float64) if len(both) else np.zeros(3)


def device_distance(q, v, t, max_dist, origin=None):
    """mesh_distance_numpy's arguments -> (dist, index) numpy, from the kernels: a grid over the triangles from the common minimum"""
    q, v = np.asarray(q, dtype=np.float32).reshape(-1, 3), np.asarray(v, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(t, dtype=np.int32).reshape(-1, 3)
    if origin is None:
        origin = common_origin(q, v)
    grid = ops.mesh_grid(up(v), up(t), origin, float(np.float32(max_dist)) * ops.CLOUD_CELL_MARGIN)
    dist, index = ops.mesh_nearest(up(q), grid, max_dist)
    assert dist.dtype == torch.float32 and index.dtype == torch.int32 and dist.shape == index.shape == (len(q),)
    return dist.cpu().numpy(), index.cpu().numpy()


def check_against(ref, dist, index, label, rows=None):
    """The issue's assertions on the queries that are not excluded (rows: a subset of the reference's queries); prints the figures first."""
    rows = np.arange(len(ref["q"])) if rows is None else rows
    q, md, band, keep = ref["q"][rows], ref["max_dist"], ref["band"], ~ref["excluded"][rows]
    d64, i64, raw64 = ref["d64"][rows], ref["i64"][rows], ref["raw64"][rows]
    diff = np.abs(dist.astype(np.float64) - d64)
    wrong = int(((index >= 0) != (i64 >= 0))[keep].sum())
    print(f"\n{label}: gap {ref['gap']:.2e}, band {band:.2e}, excluded {100 * ref['share']:.3f} %; kernel: max |dist - d64| "
          f"{diff[keep].max():.2e}, wrong verdicts {wrong}, found {100 * (index >= 0).mean():.1f} %")
    assert ref["share"] <= MC.MAX_EXCLUDED_SHARE
    assert (diff[keep] <= band).all()
    assert wrong == 0
    found = index >= 0
    assert (index[found] < len(ref["t"])).all()
    own = ME.triangle_distance_numpy(q[found], ref["v"], ref["t"], index[found])
    assert (own <= raw64[found] + band).all()
    assert (dist[~found] == md).all() and (dist[found] < md).all()
    for tau in ref["thresholds"]:
        assert np.array_equal((dist < tau)[keep], (d64 < tau)[keep])


@pytest.mark.parametrize("offset", MC.S_OFFSETS, ids=lambda o: f"sphere+{int(o)}")
def test_nearest_kernel_against_the_definition(offset):
    ref = MC.reference(("sphere", offset))
    dist, index = device_distance(ref["q"], ref["v"], ref["t"], MC.S_MAX_DIST)
    check_against(ref, dist, index, f"sphere +{int(offset)}")
    assert 0.05 < (index < 0).mean() < 0.3 and 0.2 < (dist < 0.01).mean() < 0.5  # every verdict occurs


@pytest.mark.parametrize("base", MC.B_BASES)
def test_boundary(base):
    """A triangle whose nearest point is a hair inside max_dist, on a cell corner's far side in every one of the 26 directions, is
    found; a hair outside, truncated."""
    for sign in "-+":
        ref = MC.reference(("boundary", base, sign))
        assert not ref["excluded"].any() and ((ref["i64"] >= 0) == (sign == "-")).all()  # the reference decides all 26
        dist, index = device_distance(ref["q"], ref["v"], ref["t"], MC.B_MAX_DIST, origin=np.full(3, base))  # the queries ON cell corners
        if sign == "-":
            assert np.array_equal(index, np.arange(26))
            assert (dist < np.float32(MC.B_MAX_DIST)).all() and (dist > np.float32(MC.B_MAX_DIST) * (1 - 2.0 ** -10)).all()
        else:
            assert (index == -1).all() and (dist == np.float32(MC.B_MAX_DIST)).all()


@pytest.mark.parametrize("case", ["crowded", "quad", "sphere+quad"])
def test_crowded_cell_and_large_boxes(case):
    """crowded: 700 triangles in one cell are six LDS stages, the staging is chunked and not sized by the cell, and the far queries
    find nothing.  quad, sphere+quad: two triangles of 41 x 41 cells each, alone and among 1280 small ones."""
    ref = MC.reference((case,))
    origin = np.zeros(3) if case == "crowded" else None
    dist, index = device_distance(ref["q"], ref["v"], ref["t"], ref["max_dist"], origin=origin)
    check_against(ref, dist, index, case)
    if case == "crowded":
        assert (index[:70] >= 0).all() and (index[70:] == -1).all()
    else:
        assert np.isin(index, [len(ref["t"]) - 2, len(ref["t"]) - 1]).sum() > 100  # the quad answers its queries


def test_degenerate_and_invalid_triangles():
    ref = MC.reference(("degenerate",))
    dist, index = device_distance(ref["q"], ref["v"], ref["t"], MC.D_MAX_DIST)
    check_against(ref, dist, index, "degenerate")
    assert set(np.unique(index)) == {-1, 0, 1, 2, 3}  # a line, a segment, a point and a triangle answer; an invalid one never
    # the line and the point give the segment's and the point's distance
    q64 = ref["q"].astype(np.float64)
    won = index == 2
    assert won.any() and np.abs(dist[won] - np.linalg.norm(q64[won] - 0.5, axis=1)).max() <= 1e-6
    won = index == 0
    on_line = np.clip(q64[won, 0], 0, 1)
    assert won.any() and np.abs(dist[won] - np.linalg.norm(q64[won] - np.stack([on_line, 0 * on_line, 0 * on_line], 1), axis=1)).max() <= 1e-6
    # only invalid triangles: no pair, everything is truncated
    dist, index = device_distance(ref["q"], ref["v"], ref["t"][4:], MC.D_MAX_DIST, origin=np.full(3, -0.5))
    assert (index == -1).all() and (dist == np.float32(MC.D_MAX_DIST)).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_query_counts(n):
    """A wave's worth of queries and one more and less, on the degenerate case's mesh (its first n queries, the band of all 300)."""
    ref = MC.reference(("degenerate",))
    dist, index = device_distance(ref["q"][:n], ref["v"], ref["t"], MC.D_MAX_DIST, origin=common_origin(ref["q"], ref["v"]))
    check_against(ref, dist, index, f"n = {n}", rows=np.arange(n))


def test_empty_inputs():
    ref = MC.reference(("degenerate",))
    dist, index = device_distance(np.zeros((0, 3)), ref["v"], ref["t"], 0.1)
    assert dist.shape == (0,) and index.shape == (0,)
    dist, index = device_distance(ref["q"], ref["v"], np.zeros((0, 3), np.int32), 0.1)
    assert (dist == np.float32(0.1)).all() and (index == -1).all()
    dist, index = device_distance(ref["q"], np.zeros((0, 3)), ref["t"], 0.1)  # no vertex: every triangle is invalid
    assert (dist == np.float32(0.1)).all() and (index == -1).all()
    pts, tri, attr = ops.mesh_sample(up(ref["v"]), up(np.zeros((0, 3), np.int32)), 0.1, up(ref["v"]))
    assert pts.shape == (0, 3) and tri.shape == (0,) and attr.shape == (0, 3)


def test_query_forms_and_determinism():
    ref = MC.reference(("sphere", 1000.0))
    q, v, t = ref["q"], ref["v"], ref["t"]
    a, b = device_distance(q, v, t, MC.S_MAX_DIST), device_distance(q, v, t, MC.S_MAX_DIST)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    # the queries as a CloudGrid of the same origin and cell, as MeshEvaluation runs them: the same bits
    origin, cell = common_origin(q, v), float(np.float32(MC.S_MAX_DIST)) * ops.CLOUD_CELL_MARGIN
    grid, again = ops.mesh_grid(up(v), up(t), origin, cell), ops.mesh_grid(up(v), up(t), origin, cell)
    assert torch.equal(grid.keys, again.keys) and torch.equal(bits(grid.records), bits(again.records))
    d, i = ops.mesh_nearest(ops.cloud_grid(up(q), origin, cell, check=False), grid, MC.S_MAX_DIST)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), a[0].view(np.uint32)) and np.array_equal(i.cpu().numpy(), a[1])
    # a larger cell than the minimum: fewer pairs, the same answers within the band (another cell order may pick another equal winner)
    coarse = ops.mesh_grid(up(v), up(t), origin, 2 * cell)
    assert coarse.keys.shape[0] < grid.keys.shape[0]
    d2, i2 = ops.mesh_nearest(up(q), coarse, MC.S_MAX_DIST)
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), a[0].view(np.uint32)) and np.array_equal(i2.cpu().numpy(), a[1])
    s1, s2 = ops.mesh_sample(up(v), up(t), 0.03, up(v)), ops.mesh_sample(up(v), up(t), 0.03, up(v))
    for x, y in zip(s1, s2):
        assert torch.equal(bits(x), bits(y))


def test_pair_list_equals_the_definition():
    q, v, t, md, _ = MC.mesh_case(("sphere+quad",))
    origin, cell = common_origin(q, v), float(np.float32(md)) * ops.CLOUD_CELL_MARGIN
    keys, tri = ME.mesh_grid_pairs_numpy(v, t, origin, cell)
    grid = ops.mesh_grid(up(v), up(t), origin, cell)
    assert grid.keys.dtype == torch.int64 and grid.records.shape == (len(keys), 12)
    assert np.array_equal(grid.keys.cpu().numpy(), keys)
    assert np.array_equal(grid.pair_triangles.cpu().numpy(), tri)
    rec = grid.records.cpu().numpy()
    assert np.array_equal(rec[:, :9], v[t[tri]].reshape(-1, 9)) and (rec[:, 10:] == 0).all()
    # with invalid triangles among them
    _, dv, dt, _, _ = MC.mesh_case(("degenerate",))
    keys, tri = ME.mesh_grid_pairs_numpy(dv, dt, [-1, -1, -1], 0.31)
    grid = ops.mesh_grid(up(dv), up(dt), [-1, -1, -1], 0.31)
    assert np.array_equal(grid.keys.cpu().numpy(), keys) and np.array_equal(grid.pair_triangles.cpu().numpy(), tri)


def test_wrapper_errors():
    q, v, t, md, _ = MC.mesh_case(("sphere+quad",))
    origin, cell = common_origin(q, v), float(np.float32(md)) * ops.CLOUD_CELL_MARGIN
    with pytest.raises(ValueError, match=r"3\d\d\d \(cell, triangle\) pairs.*above max_pairs = 1000; the largest triangle's box alone covers 1\d\d\d cells"):
        ops.mesh_grid(up(v[-4:]), up(t[-2:] - (len(v) - 4)), origin, cell, max_pairs=1000)
    with pytest.raises(ValueError, match="max_pairs must be in"):
        ops.mesh_grid(up(v), up(t), origin, cell, max_pairs=2 ** 31)
    with pytest.raises(ValueError, match=r"each must be in \[0, 2097151\)"):
        ops.mesh_grid(up(v), up(t), origin + 1.0, cell)
    grid = ops.mesh_grid(up(v), up(t), origin, cell)
    with pytest.raises(ValueError, match="below max_dist"):
        ops.mesh_nearest(up(q), grid, 2 * md)
    with pytest.raises(ValueError, match="MeshGrid"):
        ops.mesh_nearest(up(q), ops.cloud_grid(up(v), origin, cell), md)
    with pytest.raises(ValueError, match="differ in origin"):
        ops.mesh_nearest(ops.cloud_grid(up(q), origin - 1.0, cell, check=False), grid, md)
    with pytest.raises(ValueError, match="cuda"):
        ops.mesh_nearest(torch.from_numpy(q), grid, md)
    with pytest.raises(ValueError, match="dtype"):
        ops.mesh_grid(up(v), up(t.astype(np.int64)), origin, cell)
    with pytest.raises(ValueError, match="above max_samples = 100"):
        ops.mesh_sample(up(v), up(t), 0.03, max_samples=100)
    with pytest.raises(ValueError, match="attributes must be"):
        ops.mesh_sample(up(v), up(t), 0.03, up(v[:-1]))
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.mesh_sample(up(v).requires_grad_(), up(t), 0.03)


@pytest.mark.parametrize("case", ["sphere", "k50", "degenerate"])
def test_samples_equal_the_definition(case):
    """S, triangle, points and attributes bit for bit: the sphere at s = 0.03 (k = 3 everywhere), one triangle of k = 50 among the
    sphere's small ones at s = 2^-5, and the degenerate case's line, point and invalid triangles."""
    if case == "degenerate":
        _, v, t, _, _ = MC.mesh_case(("degenerate",))
        s = 0.25
    else:
        _, v, t = MC.sphere(0.0)
        s = 0.03
        if case == "k50":
            s = 2.0 ** -5
            big = np.array([[2, 0, 0], [2 + 50 * s, 0, 0], [2.7, 0.5, 0.1]], dtype=np.float32)
            v, t = np.concatenate([v[:300], big, v[300:]]), np.where(t >= 300, t + 3, t)
            t = np.concatenate([t[:700], [[300, 301, 302]], t[700:]]).astype(np.int32)
    attr = np.random.default_rng(11).uniform(-1, 255, (len(v), 5)).astype(np.float32)
    attr[~np.isfinite(v).all(axis=1)] = 7.0
    want = ME.sample_mesh_numpy(v, t, s, attr)
    got = ops.mesh_sample(up(v), up(t), s, up(attr))
    k, _ = ME.sample_counts_numpy(v, t, s)
    assert len(want[0]) == int((k * k).sum()) and got[0].shape == want[0].shape and got[2].shape == want[2].shape
    if case == "k50":
        assert k[700] == 50 and (np.delete(k, 700) == 3).all()
    if case == "degenerate":
        assert (k[4:] == 0).all() and (k[:4] > 0).all()
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32
    assert np.array_equal(got[1].cpu().numpy(), want[1])
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[2].cpu().numpy().view(np.uint32), want[2].view(np.uint32))
    plain = ops.mesh_sample(up(v), up(t), s)
    assert plain[2] is None and torch.equal(bits(plain[0]), bits(got[0])) and torch.equal(plain[1], got[1])


def test_evaluation_on_the_device_equals_the_host_path():
    ref = MC.reference(("sphere", 0.0))
    q, v, t = ref["q"], ref["v"], ref["t"]
    ev = ME.MeshEvaluation(MC.S_THRESHOLDS, MC.S_MAX_DIST, spacing=0.03)
    host, dev = ev((v, t), q), ev(R.Mesh(up(v), up(t)), up(q))
    assert dev.dist_pred.is_cuda and dev.dist_gt.is_cuda and dev.pred_points.is_cuda
    assert (dev.n_pred, dev.n_gt) == (host.n_pred, host.n_gt) == (11520, 2000)
    assert np.array_equal(dev.pred_points.cpu().numpy().view(np.uint32), host.pred_points.view(np.uint32))  # the samples, bit for bit
    # the cloud asks the mesh: mesh_eval_cases' reference
    assert np.abs(dev.dist_gt.cpu().numpy() - ref["d64"])[~ref["excluded"]].max() <= ref["band"]
    assert abs(dev.completeness - host.completeness) <= ref["band"] + ref["excluded"].mean() * MC.S_MAX_DIST
    assert (np.abs(dev.recall - host.recall) * 2000 <= ref["excluded"].sum() + 1e-9).all()  # the counts differ only by the excluded
    # the samples ask the cloud: the band of cloud_eval's two chains on these very points
    s = host.pred_points
    raw64, raw32 = CE.nearest_numpy(s, q, np.inf)[0], CE.nearest_numpy(s, q, np.inf, dtype=np.float32)[0]
    md = np.float32(MC.S_MAX_DIST)
    both = (raw64 < md) & (raw32 < md)
    band = 4 * np.abs(raw32.astype(np.float64) - raw64)[both].max()
    excluded = np.zeros(len(s), dtype=bool)
    for edge in (md,) + tuple(np.float32(x) for x in MC.S_THRESHOLDS):
        excluded |= np.abs(raw64 - np.float64(edge)) <= band
    assert excluded.mean() <= MC.MAX_EXCLUDED_SHARE
    assert np.abs(dev.dist_pred.cpu().numpy() - np.minimum(raw64, md))[~excluded].max() <= band
    assert abs(dev.accuracy - host.accuracy) <= band + excluded.mean() * MC.S_MAX_DIST
    assert (np.abs(dev.precision - host.precision) * len(s) <= excluded.sum() + 1e-9).all()
    np.testing.assert_allclose(dev.overall, (dev.accuracy + dev.completeness) / 2, rtol=1e-15)
    # mesh against mesh with thinning, and the other order of the sides
    thin = ME.MeshEvaluation(MC.S_THRESHOLDS, MC.S_MAX_DIST, spacing=0.03, voxel=0.05)
    a, b = thin((v, t), (v, t)), thin((up(v), up(t)), (up(v), up(t)))
    assert a.n_pred == b.n_pred == b.n_gt < 11520 and abs(a.accuracy - b.accuracy) < 1e-6 and (b.fscore == 1).all()
    swapped = ev(up(q), (up(v), up(t)))
    assert swapped.accuracy == dev.completeness and np.array_equal(swapped.precision, dev.recall)
    with pytest.raises(ValueError, match="different places"):
        ev((up(v), up(t)), q)
    with pytest.raises(ValueError, match="PointCloudEvaluation"):
        ev(up(q), up(q))
    moved = ME.evaluate_mesh(R.Mesh(up(v), up(t)), q, MC.S_THRESHOLDS, max_dist=MC.S_MAX_DIST, spacing=0.03)
    assert moved.dist_gt.is_cuda and moved.completeness == dev.completeness


def test_mesh_methods_on_an_extracted_mesh():
    """Mesh.distance and Mesh.sample on TSDFVolume.extract_mesh() of tsdf_cases' sphere (3000 triangles, voxel 0.1, radius 0.52)."""
    F, Wt = TC.sphere_volume()
    mesh = R.TSDFVolume.from_arrays(up(F), up(Wt), origin=RC.SPHERE_ORIGIN, voxel=RC.SPHERE_VOXEL).extract_mesh()
    v, t = mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy()
    assert len(t) == 3000
    centre = np.array(RC.SPHERE_ORIGIN) + np.array(TC.SPHERE[1]) * RC.SPHERE_VOXEL
    u = np.random.default_rng(13).standard_normal((500, 3))
    pts = (centre + u / np.linalg.norm(u, axis=1, keepdims=True) * TC.SPHERE[2] * RC.SPHERE_VOXEL * np.linspace(0.9, 1.1, 500)[:, None]).astype(np.float32)
    dist, index = mesh.distance(up(pts), 0.04)
    want, _ = ME.mesh_distance_numpy(pts, v, t, 0.04)
    d = dist.cpu().numpy()
    clear = np.abs(ME.mesh_distance_numpy(pts, v, t, np.inf)[0] - np.float64(np.float32(0.04))) > 1e-6
    assert clear.mean() > 0.99 and np.abs(d - want)[clear].max() <= 1e-6  # coordinates of 3: a float32 ulp is 2.4e-7
    assert 0.2 < (index.cpu().numpy() >= 0).mean() < 0.8
    samples, tri, colors = mesh.sample(0.05)
    ws, wt, _ = ME.sample_mesh_numpy(v, t, 0.05)
    assert colors is None and samples.is_cuda and torch.equal(bits(samples), bits(up(ws))) and np.array_equal(tri.cpu().numpy(), wt)
    assert mesh.distance(samples, 0.04)[0].max().item() <= 1e-6  # the samples lie on the surface
