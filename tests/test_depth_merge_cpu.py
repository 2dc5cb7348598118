"""CPU checks of the merge mode and of the normals of depth fusion: normals_numpy and merge_numpy (the definitions, float64), the host
path of DepthFusion(merge=..., normals=...), and the PLY normal properties.  The check_* functions take the function under test, so
that test_hip_depth_merge.py runs the same edge cases on the device."""
import numpy as np
import pytest

import fusion_cases as FC
import merge_cases as MC
from robustmvd_amd import cloud_eval as CE
from robustmvd_amd import depth_fusion as DF

# plain and merged point counts of scene A from float64 numpy: a property of the definition
SCENE_A_COUNTS = {(37, 53): (6532, 1835), (96, 131): (44561, 12484)}


def check_analytic_normal(normals, size):
    """Scene B is one plane: every view's normal is the plane's, towards the camera, wherever the stencil is inside the image."""
    H, W = size
    sc = FC.scene("B", H, W)
    worst = 0.0
    for i in range(MC.N_VIEWS):
        n = normals(sc["depths"][i], sc["K"], sc["Ts"][i])
        assert n.shape == (3, H, W)
        ok = MC.valid_normal(n)
        inner = np.zeros((H, W), dtype=bool)
        inner[1:-1, 1:-1] = True
        assert np.array_equal(ok, inner)
        assert (np.abs(np.linalg.norm(n[:, ok].astype(np.float64), axis=0) - 1) < 1e-6).all()
        assert (MC.plane_normal() @ n[:, ok] > 0).all()  # towards the camera, not away from it
        worst = max(worst, float(MC.sin_angle(n[:, ok], MC.plane_normal()[:, None]).max()))
    print(f"\n{H}x{W}: largest sin(angle) to the analytic normal {worst:.2e}")
    assert worst <= MC.ANALYTIC_NORMAL_BOUND
    return worst


def check_normal_validity(normals):
    """The border is zero, and a depth that is not finite or <= 0 zeroes exactly the five pixels whose stencil touches it."""
    H, W = FC.SIZES[0]
    sc = FC.scene("B", H, W)
    d = sc["depths"][1].copy()
    holes = {(10, 20): np.nan, (20, 30): 0.0, (5, 5): -1.0, (25, 40): np.inf, (1, 1): -np.inf, (30, 51): np.nan}
    want = np.zeros((H, W), dtype=bool)
    want[1:-1, 1:-1] = True
    for (y, x), value in holes.items():
        d[y, x] = value
        for yy, xx in ((y, x), (y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            want[yy, xx] = False
    n = normals(d, sc["K"], sc["Ts"][1])
    assert np.array_equal(MC.valid_normal(n), want)
    assert np.isfinite(n).all()
    assert MC.sin_angle(n[:, want], MC.plane_normal()[:, None]).max() <= MC.ANALYTIC_NORMAL_BOUND


def check_normal_faces_the_camera(normals):
    """A camera behind the plane, looking back at it, sees the other face: the flipped normal."""
    H, W = FC.SIZES[0]
    K = FC.intrinsics(H, W)
    T = FC.pose(FC.rot_y(np.pi) @ FC.rot_x(0.02), (0.1, -0.05, 8.0))
    d = FC.render(K, T, H, W, patch=False).astype(np.float32)
    assert (d > 0).all()
    n = normals(d, K, T)
    ok = MC.valid_normal(n)
    assert ok[1:-1, 1:-1].all()
    assert (-MC.plane_normal() @ n[:, ok] > 0.999).all()
    assert MC.sin_angle(n[:, ok], -MC.plane_normal()[:, None]).max() <= MC.ANALYTIC_NORMAL_BOUND


@pytest.mark.parametrize("size", FC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_analytic_normal(size):
    check_analytic_normal(DF.normals_numpy, size)


def test_normal_validity():
    check_normal_validity(DF.normals_numpy)
    assert not DF.normals_numpy(np.ones((2, 5)), FC.intrinsics(2, 5), np.eye(4)).any()  # no pixel has a whole stencil


def test_normal_faces_the_camera():
    check_normal_faces_the_camera(DF.normals_numpy)


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("size", FC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_numpy(name, size):
    ref = MC.reference(name, *size)
    sc, m = ref["scene"], ref["f64"]
    plain = [DF.fuse_numpy(*FC.key_and_sources(sc, i)) for i in range(MC.N_VIEWS)]
    for i in range(MC.N_VIEWS):
        for k in ("view_bits", "count", "fused"):
            assert np.array_equal(m[k][i], plain[i][k]), (i, k)
        assert np.array_equal(m["mask"][i], plain[i]["mask"] & (m["claimed_before"][i] == 0))
        assert not (m["mask"][i] & m["claimed_before"][i]).any()  # no emitted pixel was claimed before its view ran
        for k in ("merged_rgb", "merged_normal"):
            assert m[k][i].shape == (3,) + size and not m[k][i][:, m["mask"][i] == 0].any()
    assert np.array_equal(m["mask"][0], plain[0]["mask"]) and not m["claimed_before"][0].any()
    # the claims, replayed from the definition's own bits and (u,v) with a band of zero: every target is certain
    claimed = {j: np.zeros(size, dtype=np.uint8) for j in range(MC.N_VIEWS)}
    for i, src in enumerate(MC.SOURCES):
        assert np.array_equal(claimed[i], m["claimed_before"][i])
        after = {j: c.copy() for j, c in claimed.items()}
        det = ref["views"][i]["f64"]
        for s, mem in enumerate(MC.members(src, m["view_bits"][i], m["mask"][i], det["u"], det["v"], -1.0)):
            assert mem["certain"].all()
            after[src[s]][mem["ty"], mem["tx"]] = 1
        MC.check_claims(src, m["view_bits"][i], m["mask"][i], det["u"], det["v"], -1.0, claimed, after)
        claimed = after
    for j in range(MC.N_VIEWS):
        assert np.array_equal(claimed[j], m["claimed"][j])
    n_plain, n_merged = sum(int(p["mask"].sum()) for p in plain), sum(int(k.sum()) for k in m["mask"])
    print(f"\nscene {name} {size[0]}x{size[1]}: {n_plain} points plain, {n_merged} merged")
    assert 0 < n_merged < n_plain
    if name == "A":
        assert (n_plain, n_merged) == SCENE_A_COUNTS[size]
    else:  # one plane: the merged normal is the plane's
        for i in range(MC.N_VIEWS):
            ok = MC.valid_normal(m["merged_normal"][i])
            assert np.array_equal(ok, m["mask"][i].astype(bool))  # an emitted pixel has three members, not all of them on a border
            assert MC.sin_angle(m["merged_normal"][i][:, ok], MC.plane_normal()[:, None]).max() <= MC.ANALYTIC_NORMAL_BOUND


def test_merged_colour_is_the_mean_over_the_members():
    """The images are (x + 1000 i, y, 7 i) for view i: the mean over a sample pixel's members, by hand."""
    H, W = FC.SIZES[0]
    ref = MC.reference("A", H, W)
    m = ref["f64"]
    for i in (0, 2):
        ys, xs = np.nonzero(m["mask"][i])
        for k in (0, len(ys) // 2, len(ys) - 1):
            y, x = int(ys[k]), int(xs[k])
            total, n = np.array([x + 1000.0 * i, y, 7.0 * i]), 1
            det = ref["views"][i]["f64"]
            for s, j in enumerate(MC.SOURCES[i]):
                if (int(m["view_bits"][i][y, x]) >> s) & 1:
                    tx, ty = round(float(det["u"][s, y, x])), round(float(det["v"][s, y, x]))  # Python's round: half to even
                    total += (tx + 1000.0 * j, ty, 7.0 * j)
                    n += 1
                    assert m["claimed"][j][ty, tx] == 1
            assert n == int(m["count"][i][y, x]) + 1 >= 4
            np.testing.assert_allclose(m["merged_rgb"][i][:, y, x], total / n, rtol=1e-15)


def test_merge_numpy_options():
    H, W = FC.SIZES[0]
    sc = FC.scene("A", H, W)
    with pytest.raises(ValueError, match="among its own sources"):
        DF.merge_numpy(sc["depths"], sc["Ks"], sc["Ts"], sources=[[1, 2], [0, 1], [0], [0], [0]])
    m = DF.merge_numpy(sc["depths"], sc["Ks"], sc["Ts"])
    assert m["merged_rgb"] is None and m["merged_normal"] is None and m["normals"] is None and "claimed_before" not in m
    assert sum(int(k.sum()) for k in m["mask"]) == SCENE_A_COUNTS[(H, W)][1]
    # a view that is nobody's source is never claimed; one source and min_consistent_views=1
    sub = DF.merge_numpy(sc["depths"], sc["Ks"], sc["Ts"], sources=[[1], [0], [0, 1], [0, 1, 2], [3]], min_consistent_views=1, details=True)
    assert not sub["claimed"][4].any() and sub["claimed"][0].any() and sub["claimed"][3].any()
    plain4 = DF.fuse_numpy(*FC.key_and_sources(sc, 4, [3]), min_consistent_views=1)
    assert np.array_equal(sub["mask"][4], plain4["mask"])
    # the uncertainty filters the key pixel before it can claim anything
    unc = [np.full((H, W), 0.25 * i, dtype=np.float32) for i in range(5)]
    m = DF.merge_numpy(sc["depths"], sc["Ks"], sc["Ts"], uncertainties=unc, max_uncertainty=0.3)
    assert m["mask"][0].any() and m["mask"][1].any() and not any(k.any() for k in m["mask"][2:])
    # views 2-4 emit nothing, so they claim nothing: whatever their source lists are, the claimed maps are those of views 0 and 1
    other = DF.merge_numpy(sc["depths"], sc["Ks"], sc["Ts"], sources=[[1, 2, 3, 4], [0, 2, 3, 4], [0], [0], [0]], uncertainties=unc,
                           max_uncertainty=0.3)
    assert m["claimed"][4].any() and all(np.array_equal(a, b) for a, b in zip(other["claimed"], m["claimed"]))


def test_depth_fusion_on_host_arrays_merges():
    H, W = FC.SIZES[0]
    ref = MC.reference("A", H, W)
    sc, m = ref["scene"], ref["f64"]
    out = DF.DepthFusion(merge=True, normals=True)(sc["depths"], sc["Ks"], sc["Ts"], images=sc["images"])
    plain = DF.DepthFusion()(sc["depths"], sc["Ks"], sc["Ts"], images=sc["images"])
    assert plain.normals is None and plain.claimed is None
    assert (len(plain.points), len(out.points)) == SCENE_A_COUNTS[(H, W)]
    assert len(out.colors) == len(out.normals) == len(out.view_index) == len(out.points)
    assert out.points.dtype == out.colors.dtype == out.normals.dtype == np.float32
    for i in range(MC.N_VIEWS):
        assert np.array_equal(out.mask[i], m["mask"][i]) and np.array_equal(out.claimed[i], m["claimed"][i])
        ys, xs = np.nonzero(m["mask"][i])
        sel = out.view_index == i
        assert sel.sum() == len(ys)
        assert np.array_equal(out.colors[sel], m["merged_rgb"][i][:, ys, xs].T.astype(np.float32))
        assert np.array_equal(out.normals[sel], m["merged_normal"][i][:, ys, xs].T.astype(np.float32))
        want, _ = DF.points_numpy(m["mask"][i], out.fused_depth[i], sc["Ks"][i], sc["Ts"][i])
        assert np.array_equal(out.points[sel], want.astype(np.float32))
    # normals without merge: the plain cloud, each point with its key view's own normal
    own = DF.DepthFusion(normals=True)(sc["depths"], sc["Ks"], sc["Ts"], images=sc["images"])
    assert np.array_equal(own.points, plain.points) and np.array_equal(own.colors, plain.colors) and own.claimed is None
    for i in range(MC.N_VIEWS):
        ys, xs = np.nonzero(plain.mask[i])
        assert np.array_equal(own.normals[own.view_index == i], m["normals"][i][:, ys, xs].T.astype(np.float32))
    with pytest.raises(ValueError, match="among its own sources"):
        DF.DepthFusion(merge=True)(sc["depths"], sc["Ks"], sc["Ts"], sources=[[0, 1], [0], [0], [0], [0]])
    DF.DepthFusion()(sc["depths"], sc["Ks"], sc["Ts"], sources=[[0, 1], [0], [0], [0], [0]])  # allowed without merge, as before
    # existing positional construction of the result still works
    r = DF.FusionResult([], [], [], [], None, None, None, [])
    assert r.normals is None and r.claimed is None


def test_ply_round_trips_normals(tmp_path):
    rng = np.random.default_rng(3)
    pts = rng.standard_normal((11, 3)).astype(np.float32)
    cols = rng.integers(0, 256, (11, 3)).astype(np.float32)
    nrm = rng.standard_normal((11, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    path = tmp_path / "cloud.ply"
    DF.write_ply(path, pts, cols, nrm)
    header = path.read_bytes().split(b"end_header\n")[0].decode().split("\n")
    assert [h.split()[-1] for h in header if h.startswith("property")] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    got = CE.read_ply(path, normals=True)
    assert len(got) == 3
    for a, b in zip(got, (pts, cols, nrm)):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    two = CE.read_ply(path)
    assert len(two) == 2 and np.array_equal(two[0], pts) and np.array_equal(two[1], cols)
    DF.write_ply(path, pts, normals=nrm)
    p, c, n = CE.read_ply(path, normals=True)
    assert np.array_equal(p, pts) and c is None and np.array_equal(n, nrm)
    DF.write_ply(path, pts, cols)
    assert CE.read_ply(path, normals=True)[2] is None
    with pytest.raises(ValueError, match="normals for"):
        DF.write_ply(path, pts, normals=nrm[:4])
