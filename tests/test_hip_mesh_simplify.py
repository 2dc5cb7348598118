"""GPU checks of the mesh simplification kernels (csrc/mesh_simplify.hip) against the numpy forms of robustmvd_amd/mesh_simplify.py:
every integer equal; the means and the quadrics bit-equal to tests/sum_order.py's model of the device's segment order; the vertices
bit-equal to the numpy solve of the device's own sums, and within one float32 ulp of the plain in-order numpy result (a float64
reordering is ~1e-13 of a cell after the solve's condition of at most (1 + reg) / reg: it can at most move a float32 rounding
boundary); two runs bit-identical."""
import numpy as np
import pytest
import torch

import mesh_cases as MC_
import mesh_simplify_cases as SC
import render_cases as RC
import robustmvd_amd as R
from robustmvd_amd import mesh_simplify as MS
from robustmvd_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SETTINGS = (dict(), dict(placement="mean"), dict(unique=False), dict(remove_unreferenced=False), dict(unique=False, remove_unreferenced=False))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def down(t):
    return t.cpu().numpy()


def bits(a):
    a = down(a) if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def attributes_of(M):
    rng = np.random.default_rng(M + 1)
    return [rng.uniform(0, 255, (M, 3)).astype(np.float32), rng.standard_normal((M, 5)).astype(np.float32) * np.float32(1000.0),
            np.arange(2 * M, dtype=np.float32).reshape(M, 2)]


def device_run(case, rows=(), placement="quadric", unique=True, remove_unreferenced=True):
    return MS._simplify_device(up(case["vertices"]), up(case["triangles"]), float(np.float32(case["cell"])), placement, 1e-3, case["origin"],
                               unique, remove_unreferenced, [up(a) for a in rows])


def within_one_ulp(got, want, what):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    if got.size == 0:
        return 1.0
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / MC_.f32_ulp(want)
    assert (ulps <= 1.0).all(), (what, float(ulps.max()))
    return float((got.view(np.uint32) == want.view(np.uint32)).mean())


@pytest.mark.parametrize("name", SC.NAMES)
def test_kernels_equal_numpy(name):
    ref = SC.reference(name)
    case, cl = ref["case"], ref["clusters"]
    v, t, K = case["vertices"], case["triangles"], cl.num_clusters
    attrs = attributes_of(len(v))
    dv, dt, dattrs, dmap, dkept, dplaced, dcounts, inner = device_run(case, attrs)
    host = SC.result(name)
    g = inner["clusters"]
    # the clusters
    assert g.num_clusters == K
    assert down(g.vertex_cluster).dtype == np.int32 and np.array_equal(down(g.vertex_cluster), cl.vertex_cluster)
    assert down(g.cluster_start).dtype == np.int32 and np.array_equal(down(g.cluster_start), cl.cluster_start)
    assert np.array_equal(down(g.cluster_key), cl.cluster_key)
    assert np.array_equal(down(g.perm)[:len(cl.order)], cl.order)
    # the sums: the device's order, bit for bit
    assert np.array_equal(bits(inner["means"]), bits(ref["device_means"])), name
    assert np.array_equal(bits(inner["quadrics"]), bits(ref["device_quadrics"])), name
    # the triples
    assert np.array_equal(down(inner["triples"]), ref["triples"]) and np.array_equal(down(inner["alive"]) != 0, ref["alive"])
    # the solve: numpy on the device's sums gives the device's vertices
    pos, placed = ops.mesh_cluster_place(up(v), g, inner["means"], inner["quadrics"], 1e-3)
    want_pos, want_placed = MS.place_numpy(v, t, cl, quadrics=down(inner["quadrics"]), means=down(inner["means"]))
    assert np.array_equal(down(placed), want_placed) and np.array_equal(bits(pos), bits(want_pos)), name
    mean_pos, mean_placed = ops.mesh_cluster_place(up(v), g, inner["means"], None)
    want_pos, want_placed = MS.place_numpy(v, t, cl, placement="mean", means=down(inner["means"]))
    assert np.array_equal(down(mean_placed), want_placed) and np.array_equal(bits(mean_pos), bits(want_pos)), name
    # the result against the plain in-order numpy form
    assert np.array_equal(down(dt), host.mesh.triangles) and down(dt).dtype == np.int32
    assert np.array_equal(down(dkept), host.kept_triangles) and np.array_equal(down(dmap), host.vertex_map)
    assert np.array_equal(down(dplaced), host.placed) and np.array_equal(down(dcounts), host.cluster_counts)
    share = within_one_ulp(down(dv), host.mesh.vertices, name)
    print(f"\n{name}: K = {K}, {len(host.mesh.vertices)} vertices, {len(host.mesh.triangles)} triangles, placed "
          f"{np.bincount(host.placed, minlength=3).tolist()}, vertices bit-equal to in-order numpy {100 * share:.2f} %")
    # the attributes: the model of the device's order for every cluster, the in-order means for the short ones
    host_attrs = MS.simplify_numpy(v, t, case["cell"], origin=case["origin"], attributes=attrs).attributes
    keep = host.vertex_map[cl.order[cl.cluster_start[:-1]]] >= 0 if K else np.zeros(0, bool)
    short = (cl.counts <= 64)[keep]
    for a, got, plain in zip(attrs, dattrs, host_attrs):
        with np.errstate(all="ignore"):
            model = (SC.segment_sums(a[cl.order].astype(np.float64), cl.cluster_start) / cl.counts.astype(np.float64)[:, None]).astype(np.float32) \
                if K else np.zeros((0, a.shape[1]), np.float32)
        assert np.array_equal(bits(got), bits(model[keep])), name
        assert np.array_equal(bits(got)[short], bits(plain)[short]), name
        within_one_ulp(down(got), plain, name)
    # two runs: the same bits
    again = device_run(case, attrs)
    assert np.array_equal(bits(again[0]), bits(dv)) and np.array_equal(down(again[1]), down(dt))
    assert np.array_equal(bits(again[7]["quadrics"]), bits(inner["quadrics"])) and np.array_equal(bits(again[7]["means"]), bits(inner["means"]))


@pytest.mark.parametrize("name", SC.NAMES)
def test_settings_equal_numpy(name):
    case = SC.cases()[name]
    for kw in SETTINGS[1:]:
        host = SC.result(name, **kw)
        dv, dt, _, dmap, dkept, dplaced, dcounts, _ = device_run(case, **kw)
        what = f"{name} {kw}"
        assert np.array_equal(down(dt), host.mesh.triangles) and np.array_equal(down(dkept), host.kept_triangles), what
        assert np.array_equal(down(dmap), host.vertex_map) and np.array_equal(down(dplaced), host.placed), what
        assert np.array_equal(down(dcounts), host.cluster_counts), what
        within_one_ulp(down(dv), host.mesh.vertices, what)


def test_mesh_simplify_with_colours_and_normals():
    v, t, colors = SC.sphere()
    host_mesh = R.Mesh(v, t, colors)
    host_mesh.normals = host_mesh.vertex_normals()
    dev_mesh = R.Mesh(up(v), up(t), up(colors), up(host_mesh.normals))
    for cell in SC.SPHERE_CELLS:
        host = host_mesh.simplify(cell, details=True)
        dev = dev_mesh.simplify(cell, details=True)
        m = dev.mesh
        assert m.vertices.is_cuda and m.triangles.is_cuda and m.colors.is_cuda and m.normals.is_cuda and dev.attributes is None
        assert np.array_equal(down(m.triangles), host.mesh.triangles) and np.array_equal(down(dev.vertex_map), host.vertex_map)
        assert np.array_equal(down(dev.kept_triangles), host.kept_triangles) and np.array_equal(down(dev.placed), host.placed)
        assert np.array_equal(down(dev.cluster_counts), host.cluster_counts)
        within_one_ulp(down(m.vertices), host.mesh.vertices, f"cell {cell}")
        within_one_ulp(down(m.colors), host.mesh.colors, f"cell {cell} colours")
        # the normals are those of the device's own vertices
        assert np.array_equal(bits(m.normals), bits(R.vertex_normals(m.vertices, m.triangles)))
        assert tuple(m.normals.shape) == host.mesh.normals.shape
        assert SC.sphere_error(down(m.vertices)) < SC.sphere_error(down(dev_mesh.simplify(cell, placement="mean").vertices))
    plain = R.Mesh(up(v), up(t)).simplify(3.0)
    assert isinstance(plain, R.Mesh) and plain.colors is None and plain.normals is None
    with pytest.raises(ValueError, match="different places"):
        R.simplify_mesh((up(v), t), 3.0)
    with pytest.raises(ValueError, match="different places"):
        R.simplify_mesh((up(v), up(t)), 3.0, attributes=[colors])


def test_extract_mesh_simplify_product_path():
    F, Wt = MC_.blob_volume()
    host_vol = R.TSDFVolume.from_arrays(F, Wt, origin=RC.SPHERE_ORIGIN, voxel=RC.SPHERE_VOXEL)
    dev_vol = R.TSDFVolume.from_arrays(up(F), up(Wt), origin=RC.SPHERE_ORIGIN, voxel=RC.SPHERE_VOXEL)
    raw = dev_vol.extract_mesh()
    plain = dev_vol.extract_mesh(simplify=None)
    assert np.array_equal(bits(plain.vertices), bits(raw.vertices)) and np.array_equal(down(plain.triangles), down(raw.triangles))
    for clean in (None, dict(keep_largest=1)):
        m = dev_vol.extract_mesh(clean=clean, simplify=dict(cell=0.3))
        same = (raw if clean is None else raw.clean(**clean)).simplify(0.3)
        assert m.vertices.is_cuda and np.array_equal(bits(m.vertices), bits(same.vertices)) and np.array_equal(down(m.triangles), down(same.triangles))
        # the host volume's own path runs too; its extraction is only shape-equal to the device's, so nothing finer is compared
        host = host_vol.extract_mesh(clean=clean, simplify=dict(cell=0.3))
        assert 0 < len(host.triangles) < int(raw.triangles.shape[0]) and 0 < int(m.triangles.shape[0]) < int(raw.triangles.shape[0])
        assert int(down(m.triangles).max()) == int(m.vertices.shape[0]) - 1
