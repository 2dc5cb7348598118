"""CPU checks of the depth fusion (robustmvd_amd/depth_fusion.py): fuse_numpy against analytic truth on the scenes of fusion_cases.py,
the edge cases of the definition, DepthFusion on host arrays, reconstruct with a stub model, write_ply and the argument errors.

The edge-case checks take the implementation as an argument (`fuse`: fuse_numpy's positional and keyword arguments -> its dict of
numpy arrays) so that tests/test_hip_depth_fusion.py runs the same assertions on the device."""
import numpy as np
import pytest

import fusion_cases as FC
from robustmvd_amd import depth_fusion as DF

H, W = FC.SIZES[0]


def bit(bits, s):
    return (bits >> np.uint32(s)) & np.uint32(1)


# ---- edge cases shared with the device tests ----------------------------------------------------------------------------------------

def check_identity_source(fuse):
    """A copy of the key with the same pose is consistent wherever the key is valid, column W-1 and row H-1 included."""
    sc = FC.scene("B", H, W)
    d = sc["depths"][0]
    assert (d > 0).all()
    r = fuse(d, sc["K"], sc["Ts"][0], [d.copy()], [sc["K"]], [sc["Ts"][0]])
    assert (r["view_bits"] == 1).all() and (r["count"] == 1).all()
    assert (np.abs(r["fused"].astype(np.float64) - d) <= 1e-6 * d).all()
    return r


def check_invalid_depths(fuse):
    """0, a negative value, NaN and +inf: in the key they clear every bit and give fused = 0; in one tap of a source they clear that
    source's bit for every key pixel whose cell holds the tap and change nothing one pixel further away."""
    sc = FC.scene("B", H, W)
    args = FC.key_and_sources(sc, 0)
    base = DF.fuse_numpy(*args, details=True)
    bad_values = (0.0, -1.5, np.nan, np.inf)
    key = args[0].copy()
    spots = [(3, 5), (H - 1, W - 1), (17, 0), (0, 30)]
    for (y, x), val in zip(spots, bad_values):
        key[y, x] = val
    r = fuse(key, *args[1:])
    other = np.ones((H, W), dtype=bool)
    for y, x in spots:
        assert r["view_bits"][y, x] == 0 and r["count"][y, x] == 0 and r["mask"][y, x] == 0
        assert r["fused"][y, x] == 0
        other[y, x] = False
    assert np.array_equal(r["view_bits"][other], base["view_bits"][other])

    ky, kx, s = 18, 20, 1  # a key pixel in the middle and the source whose tap is spoiled
    assert bit(base["view_bits"], s)[ky, kx] == 1
    ty, tx = int(round(base["v"][s, ky, kx])), int(round(base["u"][s, ky, kx]))
    du, dv = np.abs(base["u"][s] - tx), np.abs(base["v"][s] - ty)
    holds = base["valid"][s] & (du < 1 - 1e-3) & (dv < 1 - 1e-3)   # floor(u) is tx - 1 or tx: the cell holds column tx
    far = (du > 1 + 1e-3) | (dv > 1 + 1e-3)
    assert holds[ky, kx] and holds.sum() >= 2
    for val in bad_values:
        srcs = [a.copy() for a in args[3]]
        srcs[s][ty, tx] = val
        r = fuse(args[0], args[1], args[2], srcs, args[4], args[5])
        assert (bit(r["view_bits"], s)[holds] == 0).all(), val
        assert np.array_equal(bit(r["view_bits"], s)[far], bit(base["view_bits"], s)[far]), val
        for o in (0, 2, 3):
            assert np.array_equal(bit(r["view_bits"], o), bit(base["view_bits"], o)), val


def check_source_facing_away(fuse):
    """A source turned by pi about y sees the key's points behind it (Qz <= 0): its bit is clear everywhere."""
    sc = FC.scene("B", H, W)
    back = np.eye(4)
    back[:3, :3] = FC.rot_y(np.pi)
    r = fuse(sc["depths"][0], sc["K"], sc["Ts"][0], [sc["depths"][1], sc["depths"][0]], [sc["K"]] * 2,
             [sc["Ts"][1], back @ sc["Ts"][0]])
    assert (bit(r["view_bits"], 1) == 0).all()
    assert bit(r["view_bits"], 0).any()
    assert np.array_equal(r["count"], bit(r["view_bits"], 0))


def check_mask_and_uncertainty(fuse):
    """min_consistent_views takes effect at exactly count == min; max_uncertainty is inclusive and a NaN uncertainty fails it."""
    sc = FC.scene("A", H, W)
    args = FC.key_and_sources(sc, 0)
    count = DF.fuse_numpy(*args)["count"]
    assert all((count == c).any() for c in range(5))
    r = fuse(*args)
    assert np.array_equal(r["mask"], count >= 3)  # the default: min(3, V)
    for m in range(6):
        r = fuse(*args, min_consistent_views=m)
        assert np.array_equal(r["count"], count)
        assert np.array_equal(r["mask"], count >= m), m
    unc = (np.arange(H * W, dtype=np.float32).reshape(H, W) % 7) * np.float32(0.125)  # 0 .. 0.75, the threshold 0.5 among them
    unc[4, 4] = unc[20, 33] = np.nan
    unc[5, 5] = np.inf
    r = fuse(*args, uncertainty=unc, min_consistent_views=2, max_uncertainty=0.5)
    with np.errstate(invalid="ignore"):
        want = (count >= 2) & (unc <= np.float32(0.5))
    assert np.array_equal(r["mask"], want)
    assert (unc == 0.5).any() and want[unc == 0.5].any() and not want[4, 4] and not want[5, 5]
    assert np.array_equal(r["count"], count)  # the filter touches the mask only
    r = fuse(*args, uncertainty=unc, min_consistent_views=2)  # no threshold: no filter
    assert np.array_equal(r["mask"], count >= 2)


def test_identity_source():
    r = check_identity_source(DF.fuse_numpy)
    sc = FC.scene("B", H, W)
    d = sc["depths"][0]
    det = DF.fuse_numpy(d, sc["K"], sc["Ts"][0], [d], [sc["K"]], [sc["Ts"][0]], details=True)
    assert det["valid"].all() and det["err"].max() <= 1e-6


def test_invalid_depths():
    check_invalid_depths(DF.fuse_numpy)


def test_source_facing_away():
    check_source_facing_away(DF.fuse_numpy)


def test_mask_and_uncertainty():
    check_mask_and_uncertainty(DF.fuse_numpy)


# ---- analytic truth -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", FC.SIZES)
def test_plane_is_consistent_with_itself(size):
    """Scene B: every valid pair is consistent, count = the number of in-bounds sources and the fused depth is the plane's (bilinear
    interpolation of a plane's depth is off by its curvature, below 1e-4 relative at these sizes)."""
    sc = FC.scene("B", *size)
    for key in range(5):
        args = FC.key_and_sources(sc, key)
        r = DF.fuse_numpy(*args, details=True)
        d = args[0].astype(np.float64)
        inb = (r["u"] >= 0) & (r["u"] <= size[1] - 1) & (r["v"] >= 0) & (r["v"] <= size[0] - 1)
        assert np.array_equal(r["valid"], inb)  # every tap exists: the plane fills every image
        for s in range(4):
            assert np.array_equal(bit(r["view_bits"], s).astype(bool), inb[s])
        assert np.array_equal(r["count"], inb.sum(0))
        assert 0.5 < inb.mean() < 1.0
        assert (np.abs(r["fused"] - d) / d).max() < 1e-4
        assert r["err"][inb].max() < 0.05 and r["rel"][inb].max() < 1e-4


def test_scaled_source_loses_its_bit():
    sc = FC.scene("B", H, W)
    args = FC.key_and_sources(sc, 0)
    base = DF.fuse_numpy(*args)
    srcs = list(args[3])
    srcs[2] = srcs[2] * np.float32(1.05)
    r = DF.fuse_numpy(args[0], args[1], args[2], srcs, args[4], args[5])
    assert (bit(r["view_bits"], 2) == 0).all() and bit(base["view_bits"], 2).any()
    for s in (0, 1, 3):
        assert np.array_equal(bit(r["view_bits"], s), bit(base["view_bits"], s))


def test_float32_chain_agrees_outside_the_bands():
    """The two numpy chains the device test takes its bands from give the same verdict on every pair outside those bands, and the
    excluded share stays below the 0.5 % that the device test allows."""
    for size in FC.SIZES:
        ref = FC.reference("A", *size, 0)
        keep = ~ref["excluded"]
        for s in range(4):
            assert np.array_equal(bit(ref["f64"]["view_bits"], s)[keep[s]], bit(ref["f32"]["view_bits"], s)[keep[s]])
        assert ref["share"] <= 0.005
        consistent = np.mean([bit(ref["f64"]["view_bits"], s).mean() for s in range(4)])
        assert 0.5 < consistent < 0.9 and ref["f64"]["valid"].mean() > consistent  # some pairs fail each test


# ---- DepthFusion --------------------------------------------------------------------------------------------------------------------

def check_fusion_result(out, sc, sources=None, **kwargs):
    """A FusionResult (as numpy) against fuse_numpy and points_numpy per view."""
    N = len(sc["depths"])
    pts, cols, idx = [], [], []
    for i in range(N):
        src = None if sources is None else sources[i]
        r = DF.fuse_numpy(*FC.key_and_sources(sc, i, src), **kwargs)
        assert np.array_equal(out.mask[i], r["mask"]) and np.array_equal(out.view_bits[i], r["view_bits"])
        assert np.array_equal(out.num_consistent[i], r["count"])
        np.testing.assert_allclose(out.fused_depth[i], r["fused"], rtol=1e-6)
        xyz, rgb = DF.points_numpy(r["mask"], r["fused"], sc["Ks"][i], sc["Ts"][i], sc["images"][i])
        pts.append(xyz); cols.append(rgb); idx.append(np.full(len(xyz), i))
    np.testing.assert_allclose(out.points, np.concatenate(pts), rtol=0, atol=4e-6)  # float32 of coordinates below 8
    assert out.points.dtype == np.float32 and out.points.shape == (len(out.view_index), 3)
    assert np.array_equal(out.view_index, np.concatenate(idx))
    if out.colors is not None:
        assert np.array_equal(out.colors, np.concatenate(cols))


def test_depth_fusion_on_host_arrays():
    import torch
    sc = FC.scene("A", H, W)
    out = DF.DepthFusion()(sc["depths"], sc["Ks"], sc["Ts"], images=sc["images"])
    check_fusion_result(out, sc)
    assert len(out.points) == sum(int(m.sum()) for m in out.mask) > 1000
    sources = [[1, 2], [0], [3, 4, 0], [2], [0, 1, 2, 3]]
    out = DF.DepthFusion(min_consistent_views=1, max_reproj_error=0.5)(
        [torch.from_numpy(d)[None] for d in sc["depths"]], [torch.from_numpy(K) for K in sc["Ks"]], np.stack(sc["Ts"]),
        sources=sources)
    assert out.colors is None
    check_fusion_result(out, sc, sources, min_consistent_views=1, max_reproj_error=0.5)


def check_reconstruct(out, model, sc_images, Ks, Ts, as_numpy=np.asarray):
    h, w = model.h, model.w
    pts = as_numpy(out.points)
    assert len(pts) > 0.5 * 5 * h * w
    assert FC.on_plane_residual(pts).max() < 1e-4  # only with the rescaled intrinsics and the right poses
    view_index, colors = as_numpy(out.view_index), as_numpy(out.colors)
    want_idx, want_col = [], []
    for k in range(5):
        mask = as_numpy(out.mask[k])
        assert mask.shape == (h, w)
        ys, xs = np.nonzero(mask)
        want_idx.append(np.full(len(ys), k))
        small = DF._resize_nearest(sc_images[k], h, w)
        want_col.append(small[:, ys, xs].T)
        call = model.calls[k]
        assert call["keyview_idx"] == 0 and len(call["images"]) == 5 and call["images"][0] is sc_images[k]
        np.testing.assert_allclose(call["poses"][0], np.eye(4), atol=1e-6)
        order = [k] + sorted((j for j in range(5) if j != k), key=lambda j: (abs(j - k), j))
        for j, T in zip(order, call["poses"]):
            np.testing.assert_allclose(T, Ts[j] @ np.linalg.inv(Ts[k]), atol=1e-6)
        np.testing.assert_allclose(call["intrinsics"][0], Ks[k], rtol=1e-6)
    assert np.array_equal(view_index, np.concatenate(want_idx))
    assert np.array_equal(colors, np.concatenate(want_col))


def test_reconstruct_with_a_stub_model():
    sc = FC.scene("B", H, W)
    model = FC.StubModel(H, W, with_uncertainty=True)
    out = DF.DepthFusion(max_uncertainty=10.0).reconstruct(model, sc["images"], sc["Ks"], sc["Ts"])
    check_reconstruct(out, model, sc["images"], sc["Ks"], sc["Ts"])
    # the uncertainty of the stub is 0.25 * view: a threshold of 0.6 drops the points of views 3 and 4
    model = FC.StubModel(H, W, with_uncertainty=True)
    cut = DF.DepthFusion(max_uncertainty=0.6).reconstruct(model, sc["images"], sc["Ks"], sc["Ts"])
    assert sorted(set(cut.view_index.tolist())) == [0, 1, 2]
    model = FC.StubModel(H, W, param=__import__("torch").zeros(1))  # parameters on the host: nothing is uploaded
    few = DF.DepthFusion(min_consistent_views=1).reconstruct(model, sc["images"], sc["Ks"], sc["Ts"], num_sources=2)
    assert all(len(c["images"]) == 3 for c in model.calls)
    assert isinstance(few.points, np.ndarray) and FC.on_plane_residual(few.points).max() < 1e-4


def test_write_ply_round_trips(tmp_path):
    rng = np.random.default_rng(3)
    pts = rng.standard_normal((17, 3)).astype(np.float32)
    cols = rng.uniform(0, 255, (17, 3)).astype(np.float32)
    for colors in (None, cols):
        path = tmp_path / "cloud.ply"
        DF.write_ply(path, pts, colors)
        blob = path.read_bytes()
        head, payload = blob.split(b"end_header\n", 1)
        lines = head.decode("ascii").splitlines()
        assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 17"]
        props = lines[3:]
        assert props[:3] == ["property float x", "property float y", "property float z"]
        dtype = [("xyz", "<f4", 3)]
        if colors is not None:
            assert props[3:] == ["property uchar red", "property uchar green", "property uchar blue"]
            dtype.append(("rgb", "u1", 3))
        else:
            assert len(props) == 3
        rec = np.frombuffer(payload, dtype=np.dtype(dtype))
        assert len(rec) == 17 and np.array_equal(rec["xyz"], pts)
        if colors is not None:
            assert np.array_equal(rec["rgb"], np.rint(cols).astype(np.uint8))
    DF.write_ply(tmp_path / "empty.ply", np.zeros((0, 3), np.float32))
    assert (tmp_path / "empty.ply").read_bytes().endswith(b"element vertex 0\nproperty float x\nproperty float y\n"
                                                          b"property float z\nend_header\n")
    with pytest.raises(ValueError):
        DF.write_ply(tmp_path / "bad.ply", pts, cols[:5])


def test_argument_errors():
    import torch
    from robustmvd_amd import ops
    sc = FC.scene("B", H, W)
    args = FC.key_and_sources(sc, 0)
    with pytest.raises(ValueError, match="33 source views"):
        DF.fuse_numpy(args[0], args[1], args[2], [args[3][0]] * 33, [args[4][0]] * 33, [args[5][0]] * 33)
    with pytest.raises(ValueError, match="0 source views"):
        DF.fuse_numpy(args[0], args[1], args[2], [], [], [])
    with pytest.raises(ValueError, match="H, W >= 2"):
        DF.fuse_numpy(args[0][:1], args[1], args[2], [args[3][0][:1]], args[4][:1], args[5][:1])
    with pytest.raises(ValueError, match="expected the key's"):
        DF.fuse_numpy(args[0], args[1], args[2], [args[3][0][:, :-1]], args[4][:1], args[5][:1])
    with pytest.raises(ValueError, match="uncertainty"):
        DF.fuse_numpy(*args, uncertainty=np.zeros((3, 3)), max_uncertainty=1.0)
    fusion = DF.DepthFusion()
    with pytest.raises(ValueError, match="at least 2"):
        fusion(sc["depths"][:1], sc["Ks"][:1], sc["Ts"][:1])
    with pytest.raises(ValueError, match="intrinsics"):
        fusion(sc["depths"], sc["Ks"][:4], sc["Ts"])
    with pytest.raises(ValueError, match="source views"):
        fusion(sc["depths"], sc["Ks"], sc["Ts"], sources=[[1] * 33, [0], [0], [0], [0]])
    with pytest.raises(ValueError, match="out of range"):
        fusion(sc["depths"], sc["Ks"], sc["Ts"], sources=[[5], [0], [0], [0], [0]])
    with pytest.raises(ValueError, match="images"):
        fusion(sc["depths"], sc["Ks"], sc["Ts"], images=sc["images"][:2])
    with pytest.raises(ValueError, match="33 source views"):  # the default sources of 34 views
        fusion([sc["depths"][0]] * 34, [sc["K"]] * 34, [sc["Ts"][0]] * 34)
    # the operator wrappers refuse tensors that are not on a ROCm device before anything is launched
    d = torch.from_numpy(sc["depths"][0])
    with pytest.raises(ValueError, match="cuda"):
        ops.geo_consistency(d, [d], torch.zeros(1, 24))
    with pytest.raises(ValueError, match="cuda"):
        ops.compact_points(torch.zeros(H, W, dtype=torch.uint8), d, torch.zeros(12))
