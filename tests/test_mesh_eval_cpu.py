"""CPU checks of the mesh evaluation (robustmvd_amd/mesh_eval.py): the numpy specifications of the point-to-triangle distance, the
triangle grid's pair list and the surface sampler against independent constructions (dense barycentric sampling, brute force, a k-d
tree) and values worked out by hand, and the host path of MeshEvaluation.  The kernels are checked against the same specifications
in test_hip_mesh_eval.py."""
import numpy as np
import pytest

import mesh_eval_cases as MC
import robustmvd_amd as R
from robustmvd_amd import mesh_eval as ME


def lattice(A, B, C, m):
    """the (m + 1)(m + 2) / 2 barycentric lattice points of each triangle -> (n, points, 3) float64"""
    i, j = np.meshgrid(np.arange(m + 1), np.arange(m + 1), indexing="ij")
    keep = i + j <= m
    u, w = i[keep] / m, j[keep] / m
    return A[:, None] + u[None, :, None] * (B - A)[:, None] + w[None, :, None] * (C - A)[:, None]


@pytest.mark.parametrize("offset", MC.S_OFFSETS)
def test_distance_against_dense_barycentric_sampling(offset):
    """On the winning triangle the formula is never above the nearest of a 120-step barycentric lattice, and within the lattice's
    resolution of it: a lattice point lies within one step (edge / 120) of the true nearest point p, and moving by e from p changes
    the distance d by at most e^2 / (2 d) + (the first-order term, zero or positive at a minimum over a convex set) <= e."""
    ref = MC.reference(("sphere", offset))
    q, v, t = ref["q"].astype(np.float64), ref["v"].astype(np.float64), ref["t"]
    pick = np.flatnonzero(ref["i64"] >= 0)[::6]
    assert len(pick) > 250
    tri = t[ref["i64"][pick]]
    A, B, C = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    m = 120
    near = np.linalg.norm(lattice(A, B, C, m) - q[pick, None], axis=2).min(axis=1)
    edge = max(np.linalg.norm(B - A, axis=1).max(), np.linalg.norm(C - B, axis=1).max(), np.linalg.norm(A - C, axis=1).max())
    d = ref["raw64"][pick]
    assert (d <= near + 1e-15).all()
    assert (near - d <= edge / m).all()
    # and never above the distance to any vertex
    to_vertex = np.linalg.norm(q[pick, None] - v[None], axis=2).min(axis=1)
    assert (d <= to_vertex + 1e-15).all()
    # the winner is the minimum over all triangles: no other triangle's lattice comes nearer than the formula's band
    assert (ME.triangle_distance_numpy(q[pick], ref["v"], t, ref["i64"][pick]) == d).all()


@pytest.mark.parametrize("offset", MC.S_OFFSETS)
def test_reference_bands_of_the_sphere(offset):
    """The figures the GPU test relies on, from the two numpy chains alone."""
    ref = MC.reference(("sphere", offset))
    truncated, under = float((ref["i64"] < 0).mean()), float((ref["d64"] < 0.01).mean())
    print(f"\nsphere +{int(offset)}: gap {ref['gap']:.2e}, band {ref['band']:.2e}, excluded {100 * ref['share']:.3f} %, truncated "
          f"{100 * truncated:.1f} %, under 0.01 {100 * under:.1f} %")
    assert ref["share"] <= MC.MAX_EXCLUDED_SHARE and 0 < ref["gap"] < 1e-6
    assert 0.05 < truncated < 0.3 and 0.2 < under < 0.5
    # the mesh lies in the shell between 98.5 % of the radius (an icosphere of 3 subdivisions sags by 0.5 % at most) and the radius,
    # and has a vertex on the sphere within 0.05 of every direction
    r = np.linalg.norm(ref["q"].astype(np.float64) - offset, axis=1)
    inner = MC.S_RADIUS * 0.985
    assert (ref["raw64"] >= np.maximum(np.maximum(r - MC.S_RADIUS, inner - r), 0) - 1e-6).all()
    assert (ref["raw64"] <= np.abs(r - MC.S_RADIUS) + 0.05).all()


def test_every_case_keeps_its_excluded_share():
    for key in [("crowded",), ("quad",), ("sphere+quad",)] + [("boundary", b, s) for b in MC.B_BASES for s in "-+"]:
        ref = MC.reference(key)
        assert ref["share"] <= MC.MAX_EXCLUDED_SHARE, key
    for base in MC.B_BASES:
        assert (MC.reference(("boundary", base, "-"))["i64"] == np.arange(26)).all()
        assert (MC.reference(("boundary", base, "+"))["i64"] == -1).all()
    c = MC.reference(("crowded",))
    assert (c["i64"][:70] >= 0).all() and (c["i64"][70:] == -1).all()


def test_degenerate_and_invalid_triangles():
    q, v, t, md, _ = MC.mesh_case(("degenerate",))
    assert ME.valid_triangles_numpy(v, t).tolist() == [True] * 4 + [False] * 5
    q64 = q.astype(np.float64)

    def segment(a, b):
        a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
        s = np.clip(((q64 - a) @ (b - a)) / ((b - a) @ (b - a)), 0, 1)
        return np.linalg.norm(q64 - (a + s[:, None] * (b - a)), axis=1)

    for k, want in ((0, segment([0, 0, 0], [1, 0, 0])), (1, segment([0, 1, 0], [1, 1, 0])),
                    (2, np.linalg.norm(q64 - [0.5, 0.5, 0.5], axis=1))):
        for dtype, tol in ((np.float64, 1e-15), (np.float32, 1e-6)):
            got = ME.triangle_distance_numpy(q, v, t, np.full(len(q), k), dtype=dtype)
            assert np.abs(got - want).max() <= tol, (k, dtype)
    d, i = ME.mesh_distance_numpy(q, v, t, md)
    assert set(np.unique(i)) == {-1, 0, 1, 2, 3}  # every valid triangle wins somewhere, an invalid one never
    # only invalid triangles: everything is truncated
    d, i = ME.mesh_distance_numpy(q, v, t[4:], md)
    assert (i == -1).all() and (d == np.float32(md)).all()


def test_empty_inputs_ties_and_strictness():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float32)
    t = np.array([[1, 3, 2], [0, 1, 2], [0, 1, 2], [2, 1, 0]], dtype=np.int32)
    q = np.array([[0.25, 0.25, 0.5], [0.5, 0.5, 0.25], [np.nan, 0, 0], [0.25, 0.25, 2.0]], dtype=np.float32)
    d, i = ME.mesh_distance_numpy(q, v, t, 1.0)
    assert i.tolist() == [1, 0, -1, -1] and i.dtype == np.int32  # duplicates: the smallest index; the shared edge: the smallest index
    assert d.tolist() == [0.5, 0.25, 1.0, 1.0]
    d, i = ME.mesh_distance_numpy(q[:1], v, t, 0.5)
    assert i[0] == -1 and d[0] == 0.5  # strict: a triangle at exactly max_dist is truncated
    d, i = ME.mesh_distance_numpy(np.zeros((0, 3)), v, t, 1.0)
    assert d.shape == (0,) and i.shape == (0,)
    d, i = ME.mesh_distance_numpy(q, v, np.zeros((0, 3), np.int32), 1.0)
    assert (i == -1).all() and (d == 1.0).all()
    d, i = ME.mesh_distance_numpy(q, np.zeros((0, 3), np.float32), t, 1.0)
    assert (i == -1).all()
    with pytest.raises(ValueError, match="max_dist"):
        ME.mesh_distance_numpy(q, v, t, 0.0)
    with pytest.raises(ValueError, match=r"\(T,3\)"):
        ME.mesh_distance_numpy(q, v, t[:, :2], 1.0)


def test_grid_pairs_order_and_27_cells():
    q, v, t, md, _ = MC.mesh_case(("sphere+quad",))
    md = np.float32(md)
    cell = float(md) * (1 + 2.0 ** -10)
    origin = np.minimum(q.min(0), v.min(0)).astype(np.float64)
    keys, tri = ME.mesh_grid_pairs_numpy(v, t, origin, cell)
    assert keys.dtype == np.int64 and tri.dtype == np.int32 and (np.diff(keys) >= 0).all()
    # stable: inside a key the triangles ascend (the list is emitted in triangle order)
    same = np.diff(keys) == 0
    assert (np.diff(tri)[same] > 0).all()
    # each triangle's cells are its box, nothing else: the quad's two triangles cover 41 x 41 x 1 cells or so each
    inv = 1.0 / cell
    lo = np.floor((v[t].min(axis=1).astype(np.float64) - origin) * inv).astype(np.int64)
    hi = np.floor((v[t].max(axis=1).astype(np.float64) - origin) * inv).astype(np.int64)
    assert np.array_equal(np.bincount(tri, minlength=len(t)), (hi - lo + 1).prod(axis=1))
    assert np.bincount(tri)[-2:].min() >= 40 * 40
    ix, iy, iz = keys >> 42, (keys >> 21) & (2 ** 21 - 1), keys & (2 ** 21 - 1)
    cells = np.stack([ix, iy, iz], axis=1)
    assert (cells >= lo[tri]).all() and (cells <= hi[tri]).all()
    # the emission order before the sort: x-major, then y, then z
    k1, t1 = ME.mesh_grid_pairs_numpy(v, t[-1:], origin, cell)
    n = (hi - lo + 1)[-1]
    want = [((lo[-1, 0] + a) << 42) | ((lo[-1, 1] + b) << 21) | (lo[-1, 2] + c) for a in range(n[0]) for b in range(n[1]) for c in range(n[2])]
    assert np.array_equal(k1, want) and (t1 == 0).all()  # x-major emission is ascending in the key already
    # every triangle within max_dist of a query (brute force) is listed in one of the query's 27 cells
    qc = np.floor((q.astype(np.float64) - origin) * inv).astype(np.int64)
    listed = set(zip(keys.tolist(), tri.tolist()))
    rng = np.random.default_rng(3)
    checked = 0
    for i in rng.choice(len(q), 150, replace=False):
        d = ME.triangle_distance_numpy(np.repeat(q[i:i + 1], len(t), axis=0), v, t, np.arange(len(t)))
        for j in np.flatnonzero(d < md):
            around = [((qc[i, 0] + a) << 42) | ((qc[i, 1] + b) << 21) | (qc[i, 2] + c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
            assert any((k, j) in listed for k in around), (i, j)
            checked += 1
    assert checked > 300
    with pytest.raises(ValueError, match=r"each must be in \[0, 2097151\)"):
        ME.mesh_grid_pairs_numpy(v, t, origin + 1.0, cell)
    # invalid triangles are not listed
    _, dv, dt, _, _ = MC.mesh_case(("degenerate",))
    _, tri = ME.mesh_grid_pairs_numpy(dv, dt, [-1, -1, -1], 0.31)
    assert set(tri.tolist()) == {0, 1, 2, 3}


def test_sample_counts_at_exact_multiples():
    s = np.float32(0.125)
    for mult, want in ((3, 3), (1, 1), (0.5, 1), (3.0000005, 4), (2.9999998, 3), (50, 50)):
        v = np.array([[0, 0, 0], [float(s) * mult, 0, 0], [float(s) * mult * 0.5, float(s) * mult * 0.25, 0]], dtype=np.float32)  # the x edge is the longest
        k, inv_s2 = ME.sample_counts_numpy(v, np.array([[0, 1, 2]]), s)
        assert k.tolist() == [want], (mult, k)
    # a spacing that is no power of two: the edge is exactly 3 x the float32 spacing
    s = np.float32(0.03)
    v = np.array([[1, 1, 1], [1 + 3 * float(s), 1, 1], [1.045, 1.01, 1]], dtype=np.float64)
    edge = np.float64(np.float32(v[1, 0])) - 1.0
    k, _ = ME.sample_counts_numpy(v.astype(np.float32), np.array([[0, 1, 2]]), s)
    assert k[0] == int(np.ceil(edge / np.float64(s)))
    assert ME._ceil_sqrt(np.array([0.0, 1.0, 1.0000001, 4.0, 8.99, 9.0, 9.01, 2.0 ** 52, 2.0 ** 60, np.inf])).tolist() == \
        [1, 1, 2, 2, 3, 3, 4, 2 ** 26, 2 ** 26, 2 ** 26]


def test_samples_of_the_sphere():
    from scipy.spatial import cKDTree
    _, v, t = MC.sphere(0.0)
    s = 0.03
    colors = np.random.default_rng(5).uniform(0, 255, (len(v), 4)).astype(np.float32)
    pts, tri, col = ME.sample_mesh_numpy(v, t, s, attributes=colors)
    k, _ = ME.sample_counts_numpy(v, t, s)
    assert len(pts) == (k * k).sum() == 11520 and (k == 3).all()  # the icosphere's edges are 0.069 .. 0.082
    assert pts.dtype == np.float32 and tri.dtype == np.int32 and col.shape == (len(pts), 4)
    assert np.array_equal(tri, np.repeat(np.arange(len(t)), 9))
    # on their triangles (a float32 rounding of coordinates of 0.5 away at most), and the first sample by hand
    assert ME.triangle_distance_numpy(pts, v, t, tri).max() <= 3 * 2.0 ** -25
    A, B, C = (v[t[0, c]].astype(np.float64) for c in range(3))
    assert np.array_equal(pts[0], ((7 / 9 * A + 1 / 9 * B) + 1 / 9 * C).astype(np.float32))
    assert np.array_equal(pts[1], ((5 / 9 * A + 2 / 9 * B) + 2 / 9 * C).astype(np.float32))  # the first down sub-triangle
    assert np.array_equal(pts[8], ((1 / 9 * A + 7 / 9 * B) + 1 / 9 * C).astype(np.float32))  # the last row's single sample
    # the samples of a triangle average to its centroid, and the attributes go through the same weights
    np.testing.assert_allclose(pts[:9].astype(np.float64).mean(axis=0), (A + B + C) / 3, atol=1e-7)
    w = np.linalg.solve(np.stack([A, B, C], axis=1), pts[4].astype(np.float64))
    np.testing.assert_allclose(col[4], w @ colors[t[0]].astype(np.float64), rtol=1e-5)
    # covering: every surface point is within 2 s / 3 of a sample
    rng = np.random.default_rng(6)
    pick = rng.integers(0, len(t), 20000)
    b = rng.dirichlet([1, 1, 1], 20000)
    surface = np.einsum("nk,nkc->nc", b, v[t[pick]].astype(np.float64))
    worst = cKDTree(pts.astype(np.float64)).query(surface)[0].max()
    print(f"\ncovering at s = {s}: worst distance {worst:.4f}, bound {2 * s / 3:.4f}")
    assert worst <= 2 * s / 3
    # without attributes the same points
    again = ME.sample_mesh_numpy(v, t, s)
    assert again[2] is None and np.array_equal(again[0], pts)


def test_samples_mixed_sizes_invalid_and_limits():
    q, v, t, _, _ = MC.mesh_case(("degenerate",))
    pts, tri, _ = ME.sample_mesh_numpy(v, t, 0.25)
    k, _ = ME.sample_counts_numpy(v, t, 0.25)
    assert k.tolist() == [4, 4, 1, 3, 0, 0, 0, 0, 0]  # a line and a segment of length 1, a point, edges of 0.6 .. 0.67; invalid: none
    assert np.array_equal(np.bincount(tri, minlength=9), k * k) and np.isfinite(pts).all()
    assert (pts[tri == 2] == np.float32(0.5)).all()
    with pytest.raises(ValueError, match="above max_samples = 10"):
        ME.sample_mesh_numpy(v, t, 0.25, max_samples=10)
    with pytest.raises(ValueError, match="spacing"):
        ME.sample_mesh_numpy(v, t, 0.0)
    with pytest.raises(ValueError, match="attributes"):
        ME.sample_mesh_numpy(v, t, 0.25, attributes=v[:-1])
    empty = ME.sample_mesh_numpy(v, t[4:], 0.25, attributes=v)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,) and empty[2].shape == (0, 3)


def test_mesh_evaluation_on_the_host():
    _, v, t = MC.sphere(0.0)
    mesh = R.Mesh(v, t)
    samples = mesh.sample(0.06)[0]
    assert len(samples) == 4 * 1280
    ev = R.create_evaluation("mesh", thresholds=(0.01, 0.02), spacing=0.06)
    assert isinstance(ev, ME.MeshEvaluation) and ev.max_dist == np.float32(0.08)
    score = ev(mesh, samples)  # the mesh against its own samples
    assert isinstance(score, R.CloudScore) and score.n_pred == score.n_gt == len(samples)
    assert score.accuracy < 1e-7 and score.completeness < 1e-7 and (score.fscore == 1).all()
    assert score.dist_pred.dtype == np.float32 and score.pred_points.shape == samples.shape
    # a cloud on a sphere 1.5 % larger than the mesh's: the offset to the surface is 0.0075 over a vertex and more over a triangle's
    # middle, which sags below the sphere by 0.5 - sqrt(0.5^2 - (0.082 / sqrt(3))^2) = 0.0023 at most: every point is under 0.01
    u = np.random.default_rng(9).standard_normal((1500, 3))
    cloud = (u / np.linalg.norm(u, axis=1, keepdims=True) * (0.5 * 1.015)).astype(np.float32)
    score = ev(cloud, mesh)  # cloud / mesh
    assert 0.0075 - 1e-6 <= score.dist_pred.min() and score.dist_pred.max() <= 0.0075 + 0.0023
    assert abs(score.accuracy - float(score.dist_pred.astype(np.float64).mean())) < 1e-9  # the host sums float64, dist_pred is rounded
    assert score.precision.tolist() == [1.0, 1.0] and score.n_pred == 1500 and score.n_gt == len(samples)
    assert 0.0075 - 1e-6 <= score.completeness <= 0.05  # the samples ask the 1500 points: as far as the cloud is sparse
    back = ev(mesh, cloud)  # mesh / cloud: the directions swap
    assert back.accuracy == score.completeness and back.completeness == score.accuracy
    assert np.array_equal(back.recall, score.precision)
    # mesh / mesh, as a (vertices, triangles) pair, with thinning
    both = ME.MeshEvaluation((0.01, 0.02), spacing=0.06, voxel=0.1)((v, t), mesh)
    assert both.n_pred == both.n_gt < 4 * 1280 and both.accuracy < 0.002 and (both.fscore == 1).all()
    d, i = mesh.distance(cloud, 0.05)
    assert d.dtype == np.float32 and i.dtype == np.int32 and np.array_equal(d, score.dist_pred)
    assert ME.evaluate_mesh(mesh, cloud, (0.01, 0.02), spacing=0.06).accuracy == back.accuracy
    with pytest.raises(ValueError, match="PointCloudEvaluation"):
        ev(cloud, cloud)
    with pytest.raises(ValueError, match="above max_dist"):
        ME.MeshEvaluation((0.01, 0.2), max_dist=0.1)
    with pytest.raises(ValueError, match="spacing"):
        ME.MeshEvaluation((0.01,), spacing=-1)
    with pytest.raises(ValueError, match="colours"):
        mesh.sample(0.06, colors=True)
    assert "mesh" in R.list_evaluations()
