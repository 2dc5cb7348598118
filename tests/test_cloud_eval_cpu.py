"""CPU checks of the point-cloud evaluation (robustmvd_amd/cloud_eval.py): the numpy specifications against an independent k-d tree
and against values worked out by hand, the argument errors, read_ply, and the host path of PointCloudEvaluation / evaluate_scene.
The kernels are checked against the same specifications in test_hip_cloud_eval.py."""
import numpy as np
import pytest

import cloud_cases as CC
import fusion_cases as FC
import robustmvd_amd as R
from robustmvd_amd import cloud_eval as CE
from robustmvd_amd import depth_fusion as DF


@pytest.mark.parametrize("offset", CC.S_OFFSETS)
@pytest.mark.parametrize("direction", ["qt", "tq"])
def test_nearest_numpy_equals_a_kd_tree(offset, direction):
    from scipy.spatial import cKDTree
    ref = CC.reference(("S", offset, direction), CC.S_MAX_DIST, CC.S_THRESHOLDS)
    q, p, md = ref["q"], ref["p"], float(ref["max_dist"])
    d, j = cKDTree(p.astype(np.float64)).query(q.astype(np.float64), distance_upper_bound=md)
    found = np.isfinite(d)
    assert np.array_equal(found, ref["i64"] >= 0)
    assert np.array_equal(j[found], ref["i64"][found])
    assert np.array_equal(d[found], ref["d64"][found])
    assert (ref["d64"][~found] == md).all()
    share = lambda m: float(np.mean(m))
    if direction == "qt":  # the scene decides both outcomes
        assert 0.1 < share(ref["d64"] < 0.01) < 0.4 and 0.03 < share(~found) < 0.3
    assert ref["share"] == 0.0 and 0 < ref["gap"] < 1e-6


def test_nearest_numpy_edge_cases():
    p = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0.5, np.inf, 0]], dtype=np.float32)
    q = np.array([[1, 0, 0], [0.4, 0, 0], [9, 9, 9], [np.nan, 1, 1], [0.5, 0, 0]], dtype=np.float32)
    d, j = CE.nearest_numpy(q, p, 0.45)
    assert j.tolist() == [1, 0, -1, -1, -1] and j.dtype == np.int32  # the duplicate's smaller index; 0.5 is not < 0.45
    np.testing.assert_allclose(d, [0, np.float32(0.4), 0.45, 0.45, 0.45], rtol=1e-7)
    d, j = CE.nearest_numpy(q, p, 0.5)
    assert j[4] == -1 and d[4] == 0.5  # strict: a target at exactly max_dist is truncated
    d, j = CE.nearest_numpy(np.zeros((0, 3)), p, 1.0)
    assert d.shape == (0,) and j.shape == (0,)
    d, j = CE.nearest_numpy(q, np.zeros((0, 3)), 1.0)
    assert (d == 1.0).all() and (j == -1).all()
    d, j = CE.nearest_numpy(q, p[3:], 1.0)  # no valid target
    assert (d == 1.0).all() and (j == -1).all()
    with pytest.raises(ValueError, match=r"\(n,3\)"):
        CE.nearest_numpy(np.zeros((4, 2)), p, 1.0)


def test_scores_by_hand():
    """pred -> gt: 0.1, 0.3, truncated (1);  gt -> pred: 0.1, 0.3, sqrt(0.1^2 + 0.3^2)."""
    gt = np.array([[0, 0, 0], [1, 0, 0], [1.1, 0, 0]], dtype=np.float32)
    pred = np.array([[0, 0, 0.1], [1, 0, 0.3], [5, 0, 0]], dtype=np.float32)
    s = CE.cloud_scores_numpy(pred, gt, (0.2, 0.5), 1.0)
    tol = dict(rtol=1e-6, atol=0)
    np.testing.assert_allclose(s.accuracy, (0.1 + 0.3 + 1.0) / 3, **tol)
    np.testing.assert_allclose(s.completeness, (0.1 + 0.3 + np.sqrt(0.1)) / 3, **tol)
    np.testing.assert_allclose(s.overall, (s.accuracy + s.completeness) / 2, rtol=1e-15)
    np.testing.assert_allclose(s.precision, [1 / 3, 2 / 3], rtol=1e-15)
    np.testing.assert_allclose(s.recall, [1 / 3, 1.0], rtol=1e-15)
    np.testing.assert_allclose(s.fscore, [1 / 3, 0.8], rtol=1e-15)
    assert (s.n_pred, s.n_gt) == (3, 3) and s.dist_pred.dtype == np.float32 and s.dist_pred[2] == 1.0
    # an invalid point is no point: the means and shares are over the valid ones
    s2 = CE.cloud_scores_numpy(np.concatenate([pred, [[np.nan, 0, 0]]]).astype(np.float32), gt, (0.2, 0.5), 1.0)
    assert s2.n_pred == 3 and s2.accuracy == s.accuracy and np.array_equal(s2.precision, s.precision)
    assert s2.completeness == s.completeness and s2.dist_pred[3] == 1.0
    # nothing near anything: precision + recall = 0 gives F = 0, and no point gives NaN
    s3 = CE.cloud_scores_numpy(pred + 50, gt, (0.2,), 1.0)
    assert s3.fscore.tolist() == [0.0] and s3.accuracy == 1.0
    s4 = CE.cloud_scores_numpy(np.zeros((0, 3)), gt, (0.2,), 1.0)
    assert np.isnan(s4.accuracy) and np.isnan(s4.precision[0]) and s4.completeness == 1.0 and s4.n_pred == 0


def test_score_argument_errors():
    with pytest.raises(ValueError, match="above max_dist"):
        CE.PointCloudEvaluation((0.1, 0.5), max_dist=0.4)
    with pytest.raises(ValueError, match="9 thresholds"):
        CE.PointCloudEvaluation(np.linspace(0.1, 0.9, 9))
    with pytest.raises(ValueError, match="thresholds"):
        CE.PointCloudEvaluation(())
    with pytest.raises(ValueError, match="> 0"):
        CE.PointCloudEvaluation((0.0, 0.1))
    with pytest.raises(ValueError, match="voxel"):
        CE.PointCloudEvaluation((0.1,), voxel=-1.0)
    e = CE.PointCloudEvaluation((0.1, 0.25))
    assert e.max_dist == np.float32(1.0) and e.thresholds.dtype == np.float32 and len(CE.PointCloudEvaluation(np.linspace(0.1, 0.8, 8)).thresholds) == 8


def voxel_by_hand(points, voxel, colors=None, origin=None):
    """The definition with a dict and Python loops: nothing shared with voxel_downsample_numpy but the formula of the index."""
    pts = np.asarray(points, dtype=np.float32)
    ok = np.isfinite(pts).all(axis=1)
    o = pts[ok].min(axis=0).astype(np.float64) if origin is None else np.asarray(origin, dtype=np.float64)
    inv = 1.0 / np.float64(np.float32(voxel))
    cells = {}
    for i in np.flatnonzero(ok):
        idx = tuple(int(np.floor((np.float64(pts[i, a]) - o[a]) * inv)) for a in range(3))
        cells.setdefault(idx, []).append(i)
    order = sorted(cells)
    xyz = np.array([[sum(np.float64(pts[i, a]) for i in cells[c]) / len(cells[c]) for a in range(3)] for c in order]).astype(np.float32)
    rgb = None
    if colors is not None:
        rgb = np.array([[sum(np.float64(colors[i, a]) for i in cells[c]) / len(cells[c]) for a in range(3)] for c in order]).astype(np.float32)
    return xyz.reshape(-1, 3), rgb, np.array([len(cells[c]) for c in order], dtype=np.int32), order


@pytest.mark.parametrize("voxel,negative,origin", [(2.0 ** -4, False, (0, 0, 0)), (0.01, False, (0, 0, 0)), (0.01, True, None),
                                                   (2.0 ** -4, True, (-1.5, -1, -2))], ids=["pow2", "0.01", "neg-default", "neg-origin"])
def test_voxel_specification(voxel, negative, origin):
    pts = CC.voxel_faces(voxel, negative=negative).copy()
    pts[7] = [np.nan, 0, 0]
    pts[11] = [0, np.inf, 0]
    col = np.random.default_rng(3).uniform(0, 255, pts.shape).astype(np.float32)
    xyz, rgb, counts = CE.voxel_downsample_numpy(pts, voxel, col, origin)
    wx, wr, wc, order = voxel_by_hand(pts, voxel, col, origin)
    assert np.array_equal(counts, wc) and counts.sum() == len(pts) - 2 and counts.dtype == np.int32
    assert len(order) > 100 and (counts > 1).any() == (voxel > 0.05)
    np.testing.assert_allclose(xyz, wx, rtol=2.0 ** -23, atol=0)
    np.testing.assert_allclose(rgb, wr, rtol=2.0 ** -23, atol=0)
    # a point ON a face belongs to the voxel above it, one float32 step below the face to the voxel below
    on = np.array([[3 * voxel, 0.01, 0.01], [np.nextafter(np.float32(3 * voxel), np.float32(0)), 0.01, 0.01]], dtype=np.float32)
    _, _, c = CE.voxel_downsample_numpy(on, voxel, origin=(0, 0, 0))
    assert c.tolist() == [1, 1]
    assert CE.voxel_downsample_numpy(pts, voxel, None, origin)[1] is None


def test_voxel_argument_errors():
    pts = np.array([[0, 0, 0], [1, 1, 1]], dtype=np.float32)
    with pytest.raises(ValueError, match=r"edge of 1e-07.*\[0, 2097151\)"):
        CE.voxel_downsample_numpy(pts, 1e-7)
    with pytest.raises(ValueError, match="indices -"):
        CE.voxel_downsample_numpy(pts, 0.5, origin=(0.25, 0, 0))  # a point below the origin
    with pytest.raises(ValueError, match="voxel must be"):
        CE.voxel_downsample_numpy(pts, 0.0)
    with pytest.raises(ValueError, match="colors"):
        CE.voxel_downsample_numpy(pts, 0.5, colors=np.zeros((3, 3)))
    xyz, rgb, counts = CE.voxel_downsample_numpy(np.full((3, 3), np.nan, dtype=np.float32), 0.5)
    assert xyz.shape == (0, 3) and counts.shape == (0,)
    xyz, _, counts = CE.voxel_downsample_numpy(pts, 2.0 ** -20)  # index 2^20: fits
    assert counts.tolist() == [1, 1] and np.array_equal(xyz, pts)


def test_mixed_placement_is_refused():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        class OnGpu:  # what _place looks at, without a GPU
            is_cuda, device = True, "cuda:0"
        OnGpu.__module__ = "torch"
        there = OnGpu()
    else:
        there = torch.zeros(4, 3, device="cuda:0")
    with pytest.raises(ValueError, match="different places"):
        CE.PointCloudEvaluation((0.1,))(there, np.zeros((4, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="different places"):
        CE.PointCloudEvaluation((0.1,))(np.zeros((4, 3), dtype=np.float32), there)


def test_read_ply_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    pts = rng.normal(0, 100, (257, 3)).astype(np.float32)
    col = rng.integers(0, 256, (257, 3)).astype(np.float32)
    DF.write_ply(tmp_path / "a.ply", pts, col)
    p, c = CE.read_ply(tmp_path / "a.ply")
    assert p.dtype == np.float32 and np.array_equal(p, pts) and c.dtype == np.float32 and np.array_equal(c, col)
    DF.write_ply(tmp_path / "b.ply", pts)
    p, c = CE.read_ply(tmp_path / "b.ply")
    assert np.array_equal(p, pts) and c is None
    DF.write_ply(tmp_path / "e.ply", np.zeros((0, 3)))
    p, c = CE.read_ply(tmp_path / "e.ply")
    assert p.shape == (0, 3) and c is None
    # ASCII, with a comment, a property to skip, colours, and a face element after the vertices
    (tmp_path / "c.ply").write_text("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 2\nproperty float x\nproperty float y\n"
                                    "property float nx\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                                    "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
                                    "1.5 -2 0.5 3e2 255 0 7\n0 0.25 0.5 -1 1 2 3\n3 0 1 0\n")
    p, c = CE.read_ply(tmp_path / "c.ply")
    assert p.tolist() == [[1.5, -2, 300], [0, 0.25, -1]] and c.tolist() == [[255, 0, 7], [1, 2, 3]]
    # binary with double coordinates, a property between them and z before y
    rec = np.zeros(3, dtype=[("x", "<f8"), ("quality", "<i2"), ("z", "<f8"), ("y", "<f8")])
    rec["x"], rec["y"], rec["z"], rec["quality"] = [1, 2, 3], [0.1, 0.2, 0.3], [-1, -2, -3], [9, 9, 9]
    with open(tmp_path / "d.ply", "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty double x\nproperty short quality\nproperty double z\n"
                b"property double y\nend_header\n" + rec.tobytes())
    p, c = CE.read_ply(tmp_path / "d.ply")
    assert c is None and np.array_equal(p, np.array([[1, 0.1, -1], [2, 0.2, -2], [3, 0.3, -3]], dtype=np.float32))
    (tmp_path / "bad.ply").write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\n"
                                       b"property float z\nend_header\n")
    with pytest.raises(ValueError, match="binary_big_endian"):
        CE.read_ply(tmp_path / "bad.ply")
    (tmp_path / "short.ply").write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\n"
                                         b"property float z\nend_header\n" + bytes(24))
    with pytest.raises(ValueError, match="2 of 5"):
        CE.read_ply(tmp_path / "short.ply")


def test_host_path_of_the_evaluation():
    q, p = CC.scene_s(0.0)
    ev = R.create_evaluation("cloud", thresholds=CC.S_THRESHOLDS, max_dist=CC.S_MAX_DIST)
    assert isinstance(ev, CE.PointCloudEvaluation) and "cloud" in R.list_evaluations() and "mvd" in R.list_evaluations()
    s = ev(q, p)
    fwd, back = CC.reference(("S", 0.0, "qt"), CC.S_MAX_DIST, CC.S_THRESHOLDS), CC.reference(("S", 0.0, "tq"), CC.S_MAX_DIST, CC.S_THRESHOLDS)
    assert np.array_equal(s.dist_pred, fwd["d64"].astype(np.float32)) and np.array_equal(s.dist_gt, back["d64"].astype(np.float32))
    assert s.accuracy == fwd["d64"].sum() / 3000 and s.completeness == back["d64"].sum() / 4000
    for t, tau in enumerate(np.float32(CC.S_THRESHOLDS)):
        assert s.precision[t] == (fwd["d64"] < tau).mean() and s.recall[t] == (back["d64"] < tau).mean()
    assert s.precision[2] == (fwd["i64"] >= 0).mean()  # the last threshold is max_dist: under it = found
    assert (s.n_pred, s.n_gt) == (3000, 4000) and s.pred_points is not None
    # thinning first: the prediction becomes the voxel means (colours with them), the ground truth stays
    col = np.tile(np.arange(3000, dtype=np.float32)[:, None], (1, 3))
    thin = CE.PointCloudEvaluation(CC.S_THRESHOLDS, CC.S_MAX_DIST, voxel=0.05)(q, p, col)
    vx, vc, _ = CE.voxel_downsample_numpy(q, 0.05, col)
    assert thin.n_pred == len(vx) < 3000 and thin.n_gt == 4000
    assert np.array_equal(thin.pred_points, vx) and np.array_equal(thin.pred_colors, vc) and len(thin.dist_pred) == len(vx)
    assert np.array_equal(thin.dist_pred, CE.nearest_numpy(vx, p, CC.S_MAX_DIST)[0].astype(np.float32))


def test_evaluate_scene_on_the_host():
    H, W = FC.SIZES[0]
    sc = FC.scene("B", H, W)
    fusion = DF.DepthFusion()
    want = fusion.reconstruct(FC.StubModel(H, W), sc["images"], sc["Ks"], sc["Ts"])
    assert isinstance(want.points, np.ndarray) and len(want.points) > 500
    # ground truth: the plane itself, sampled more densely than the fused cloud
    g = np.linspace(-2.5, 2.5, 126)
    gx, gy = np.meshgrid(g, g)
    gt = np.stack([gx.ravel(), gy.ravel(), (FC.PLANE_D - FC.PLANE_N[0] * gx.ravel() - FC.PLANE_N[1] * gy.ravel()) / FC.PLANE_N[2]], axis=1)
    model = FC.StubModel(H, W)
    s = CE.evaluate_scene(model, sc["images"], sc["Ks"], sc["Ts"], gt.astype(np.float32), fusion=fusion, thresholds=(0.02, 0.05))
    assert len(model.calls) == 5 and isinstance(s.dist_pred, np.ndarray)
    direct = CE.PointCloudEvaluation((0.02, 0.05))(want.points, gt.astype(np.float32), want.colors)
    assert s.n_pred == len(want.points) and s.accuracy == direct.accuracy and np.array_equal(s.fscore, direct.fscore)
    assert s.precision[1] == 1.0 and s.accuracy < 0.03  # every fused point is on the plane, within the grid's spacing of a sample
    assert 0 < s.recall[1] < 1  # the cameras see a part of the sampled plane
    assert np.array_equal(s.pred_colors, want.colors)
    with pytest.raises(ValueError, match="thresholds"):
        CE.evaluate_scene(model, sc["images"], sc["Ks"], sc["Ts"], gt)
    with pytest.raises(ValueError, match="unexpected"):
        CE.evaluate_scene(model, sc["images"], sc["Ks"], sc["Ts"], gt, evaluation=CE.PointCloudEvaluation((0.1,)), voxel=0.1)
