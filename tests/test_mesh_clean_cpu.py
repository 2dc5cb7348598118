"""CPU checks of the mesh clean-up definitions (robustmvd_amd/mesh_clean.py: the numpy forms, which are also the host path): the
components against scipy and a plain union-find, the table against bincount and math.fsum, the filter's properties, the vertex
normals on the sphere, the round counts on the long-diameter strips, and the argument errors."""
import numpy as np
import pytest

import mesh_cases as MC_
import render_cases as RC
import tsdf_cases as TC
import robustmvd_amd as R
from robustmvd_amd import mesh_clean as MC

CASES = sorted(MC_.small_cases())


def union_find(triangles, M):
    parent = list(range(M))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(triangles).tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)  # the root is the lowest index
    return np.array([find(x) for x in range(M)], dtype=np.int64)


@pytest.mark.parametrize("name", CASES)
def test_components_equal_union_find_and_scipy(name):
    ref = MC_.reference(name)
    v, t, label, table = ref["vertices"], ref["triangles"], ref["label"], ref["table"]
    M, T = len(v), len(t)
    assert label.dtype == np.int32 and label.shape == (M,)
    assert np.array_equal(label, union_find(t, M))  # the lowest vertex of the component: equal, not only the same partition
    referenced = np.zeros(M, dtype=bool)
    referenced[t.ravel()] = True
    # ids in ascending order of the lowest vertex; -1 exactly on the unreferenced vertices
    roots = np.unique(label[referenced])
    assert table.num_components == len(roots)
    assert np.array_equal(table.vertex_component, np.where(referenced, np.searchsorted(roots, label), -1))
    assert np.array_equal(table.triangle_component, table.vertex_component[t[:, 0]] if T else np.zeros(0, np.int32))
    assert np.array_equal(table.num_triangles, np.bincount(table.triangle_component, minlength=len(roots)))
    assert np.array_equal(table.num_vertices, np.bincount(table.vertex_component[referenced], minlength=len(roots)))
    assert (table.vertex_component[t] == table.triangle_component[:, None]).all()
    assert 1 <= table.rounds <= MC.max_rounds(M)
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]]]).astype(np.int64)
    graph = sparse.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(M, M))
    n, lab = connected_components(graph, directed=False) if M else (0, np.zeros(0, np.int64))
    # the same partition: each scipy component has one label of ours and the counts agree
    assert n == len(np.unique(label))
    assert M == 0 or len(np.unique(lab.astype(np.int64) * (M + 1) + label)) == n


@pytest.mark.parametrize("name", CASES)
def test_areas_against_fsum(name):
    ref = MC_.reference(name)
    exact, bound = MC_.area_bounds(ref["table"], ref["triangle_area"])
    assert ref["table"].area.dtype == np.float64
    assert (np.abs(ref["table"].area - exact) <= bound).all()
    assert np.isfinite(ref["table"].area).all()


def test_known_areas():
    """The area's definition against values that do not come from the code under test."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [2, 2, 5], [2, 6, 2]], dtype=np.float32)
    t = np.array([[0, 1, 2], [3, 4, 5], [5, 4, 3], [0, 0, 1]], dtype=np.int32)
    assert MC.triangle_areas_numpy(v, t).tolist() == [0.5, 6.0, 6.0, 0.0]  # right triangles with legs 1, 1 and 3, 4: exact in float64
    assert np.array_equal(MC.cross_numpy(v, t), [[0, 0, 1], [-12, 0, 0], [12, 0, 0], [0, 0, 0]])
    table = MC.component_table_numpy(v, t)
    assert table.area.tolist() == [0.5, 12.0]
    # the sphere of radius 5.2 voxels: the mesh is inscribed facets of the sphere, a little below 4 pi r^2
    F, Wt = TC.sphere_volume()
    area = R.TSDFVolume.from_arrays(F, Wt).extract_mesh().components().area
    assert area.shape == (1,) and 0.97 * 4 * np.pi * TC.SPHERE[2] ** 2 < area[0] < 4 * np.pi * TC.SPHERE[2] ** 2


def test_known_counts():
    t = MC_.reference("all_separate")["table"]
    assert t.num_components == 1000 and (t.num_triangles == 1) .all() and (t.num_vertices == 3).all() and (t.vertex_component == -1).sum() == 7
    assert t.rounds == 2
    t = MC_.reference("interleaved")["table"]
    assert t.num_components == 2 and t.num_triangles.tolist() == [700, 700]
    t = MC_.reference("degenerate")["table"]
    assert t.num_components == 4 and t.vertex_component[4] == -1 and t.num_triangles.tolist() == [2, 1, 3, 3]
    t = MC_.reference("floaters")["table"]
    assert sorted(t.num_triangles.tolist()) == [4, 4, 4, 3000] and sorted(t.num_vertices.tolist()) == [4, 4, 4, 1502]
    ref = MC_.reference("nonfinite")
    bad = ~np.isfinite(ref["vertices"]).all(axis=1)
    assert bad.sum() == 2 and ref["table"].num_components == 1
    touched = bad[ref["triangles"]].any(axis=1)
    assert touched.any() and (ref["triangle_area"][touched] == 0).all() and (ref["triangle_area"][~touched] > 0).all()
    assert (ref["normals"][bad] == 0).all()


@pytest.mark.parametrize("M", MC_.STRIP_M)
def test_strip_rounds(M):
    """Measured: 8 rounds at M = 1026 and 10 at 16386, the unchanged last one included (14 at 262146): below log2 M + 1."""
    table = MC_.reference(f"strip_M{M}")["table"]
    print(f"\nstrip M = {M}: {table.rounds} rounds, cap {MC.max_rounds(M)}")
    assert table.num_components == 1 and (table.vertex_component == 0).all() and (MC_.reference(f"strip_M{M}")["label"] == 0).all()
    assert table.rounds <= MC.max_rounds(M)
    assert table.rounds <= np.log2(M) + 3  # pointer jumping, not O(diameter) propagation


def test_clean_properties():
    v, t, colors, (sv, st) = MC_.sphere_with_floaters()
    extra = np.arange(len(v) * 2, dtype=np.float32).reshape(-1, 2)
    for kw in (dict(min_triangles=5), dict(keep_largest=1), dict(min_area=10.0), dict(min_triangles=2, keep_largest=2, min_area=3.0)):
        r = R.clean_mesh(R.Mesh(v, t, colors), attributes=[extra], **kw)
        m = r.mesh
        assert m.vertices.dtype == np.float32 and m.triangles.dtype == np.int32 and r.vertex_remap.dtype == np.int32
        TC.check_closed_surface(m.vertices, m.triangles, SPHERE_WORLD_CENTRE)
        assert m.vertices.shape == (1502, 3) and m.triangles.shape == (3000, 3) and len(TC.edge_counts(m.triangles)[0]) == 4500
        assert np.array_equal(m.vertices.view(np.uint32), sv.view(np.uint32)) and np.array_equal(m.triangles, st)
        # order-preserving, attributes follow
        kept_v = np.nonzero(r.vertex_remap >= 0)[0]
        assert np.array_equal(r.vertex_remap[kept_v], np.arange(len(kept_v))) and (np.diff(r.kept_triangles) > 0).all()
        assert np.array_equal(m.colors, colors[kept_v]) and np.array_equal(r.attributes[0], extra[kept_v])
        assert np.array_equal(m.triangles, r.vertex_remap[t[r.kept_triangles]])
        # idempotent
        again = R.clean_mesh(m, details=True, **kw)
        assert np.array_equal(again.mesh.vertices, m.vertices) and np.array_equal(again.mesh.triangles, m.triangles)
        assert np.array_equal(again.vertex_remap, np.arange(1502))
    # keep_largest ties go to the lower id; k = 0 keeps nothing
    r = R.clean_mesh((v, t), keep_largest=2, details=True)
    assert len(r.mesh.triangles) == 3004 and r.kept_triangles[:4].tolist() == [0, 1, 2, 3]
    assert len(R.clean_mesh((v, t), keep_largest=0).triangles) == 0 and len(R.clean_mesh((v, t), keep_largest=0).vertices) == 0
    # no criterion: nothing is removed but, by default, the unreferenced vertices
    dv, dt = MC_.degenerate()
    m = R.clean_mesh((dv, dt))
    assert len(m.triangles) == len(dt) and len(m.vertices) == len(dv) - 1
    m = R.clean_mesh((dv, dt), remove_unreferenced=False, details=True)
    assert np.array_equal(m.mesh.vertices.view(np.uint32), dv.view(np.uint32)) and np.array_equal(m.mesh.triangles, dt)
    d = R.clean_mesh((v, t), keep_largest=1, attributes={"a": extra})
    assert list(d.attributes) == ["a"] and d.attributes["a"].shape == (1502, 2)


SPHERE_WORLD_CENTRE = TC.SPHERE[1]


def test_vertex_normals_of_the_sphere():
    F, Wt = TC.sphere_volume()
    mesh = R.TSDFVolume.from_arrays(F, Wt).extract_mesh()
    n = mesh.vertex_normals()
    assert n.dtype == np.float32 and n.shape == (1502, 3) and mesh.normals is None
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() <= 4 * 2.0 ** -24  # three float32 roundings of a unit vector
    radial = mesh.vertices.astype(np.float64) - np.asarray(TC.SPHERE[1])
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    # the facet angle: no face normal of this mesh is further from the radial direction than the worst one, and a vertex normal
    # is a positive combination of its faces' normals
    face = R.render.normals_of(mesh.vertices, mesh.triangles.astype(np.int64), np.float64)
    centroid = mesh.vertices[mesh.triangles].astype(np.float64).mean(axis=1) - np.asarray(TC.SPHERE[1])
    worst = (face * centroid / np.linalg.norm(centroid, axis=1, keepdims=True)).sum(axis=1).min()
    cos = (n * radial).sum(axis=1)
    print(f"\nsphere: worst face cos {worst:.4f}, worst vertex cos {cos.min():.4f}")
    assert cos.min() >= worst - 0.05 and cos.min() > 0.8
    # a triangle that names a vertex twice counts once per corner; an unreferenced vertex gets zeros
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], dtype=np.float32)
    assert np.array_equal(R.vertex_normals(v, np.array([[0, 1, 2], [0, 0, 1]], dtype=np.int32)),
                          np.array([[0, 0, 1]] * 3 + [[0, 0, 0]], dtype=np.float32))


def test_mesh_methods_and_extract_clean():
    F, Wt = MC_.blob_volume()
    vol = R.TSDFVolume.from_arrays(F, Wt)
    raw = vol.extract_mesh()
    comps = raw.components()
    assert comps.num_components == 3 and comps.num_triangles.max() == 3000
    for kw in (dict(min_triangles=100), dict(keep_largest=1)):
        m = vol.extract_mesh(clean=kw)
        TC.check_closed_surface(m.vertices, m.triangles, TC.SPHERE[1])
        assert m.vertices.shape == (1502, 3) and m.triangles.shape == (3000, 3)
        same = raw.clean(**kw)
        assert np.array_equal(m.vertices, same.vertices) and np.array_equal(m.triangles, same.triangles)
    plain = vol.extract_mesh(clean=None)
    assert np.array_equal(plain.vertices, raw.vertices) and np.array_equal(plain.triangles, raw.triangles) and plain.normals is None


def test_render_vertex_normals_host():
    v, t, c = RC.mesh("sphere")
    Ks, Ts = RC.cameras(37, 53)
    flat = R.render_mesh((v, t), Ks, Ts, (37, 53), normals=True)
    smooth = R.render_mesh((v, t), Ks, Ts, (37, 53), normals="vertex", colors=c)
    plain = R.render_mesh((v, t), Ks, Ts, (37, 53), colors=c)
    for k in range(len(Ks)):
        assert np.array_equal(smooth.depth[k], flat.depth[k]) and np.array_equal(smooth.colors[k], plain.colors[k])
        n, mask = smooth.normals[k], flat.mask[k]
        assert n.dtype == np.float32 and (n[:, ~mask] == 0).all()
        assert np.abs(np.linalg.norm(n[:, mask].astype(np.float64), axis=0) - 1).max() <= 4 * 2.0 ** -24
        assert (n[:, mask] * flat.normals[k][:, mask]).sum(axis=0).min() > 0.8  # close to the face normal, not equal to it
        assert not np.array_equal(n, flat.normals[k])
    only = R.render_mesh(R.Mesh(v, t, normals=R.vertex_normals(v, t)), Ks, Ts, (37, 53), normals="vertex")
    assert only.colors is None and all(np.array_equal(a, b) for a, b in zip(only.normals, smooth.normals))
    with pytest.raises(ValueError, match="vertex"):
        R.render_mesh((v, t), Ks, Ts, (37, 53), normals="face")


def test_argument_errors():
    v, t = MC_.degenerate()
    with pytest.raises(ValueError, match="dtype"):
        R.mesh_components(v.astype(np.float64), t)
    with pytest.raises(ValueError, match="dtype"):
        R.mesh_components(v, t.astype(np.float32))
    with pytest.raises(ValueError, match="vertex indices"):
        R.mesh_components(v[:13], t)
    with pytest.raises(ValueError, match="vertex indices"):
        R.vertex_normals(v, t - 1)
    with pytest.raises(ValueError, match=r"\(T,3\)"):
        R.components_numpy(t.reshape(-1), len(v))
    with pytest.raises(ValueError, match=r"\(M,3\)"):
        R.clean_mesh((v[:, :2], t))
    with pytest.raises(ValueError, match="attributes"):
        R.clean_mesh((v, t), attributes=[np.zeros((3, 2), np.float32)])
    with pytest.raises(ValueError, match="min_triangles"):
        R.clean_mesh((v, t), min_triangles=-1)
    with pytest.raises(ValueError, match="keep_largest"):
        R.clean_mesh((v, t), keep_largest=1.5)
    with pytest.raises(ValueError, match="min_area"):
        R.clean_mesh((v, t), min_area=float("nan"))
    with pytest.raises(ValueError, match="own triangles"):
        R.mesh_components(R.Mesh(v, t), t)
    with pytest.raises(ValueError, match="extract_mesh: clean takes"):
        R.TSDFVolume.from_arrays(*TC.sphere_volume()).extract_mesh(clean=dict(keep_largest=1, details=True))
    # the operators take GPU tensors only (a mesh with arrays in different places needs a GPU: tests/test_hip_mesh_clean.py)
    import torch
    from robustmvd_amd import ops
    with pytest.raises(ValueError, match="cuda"):
        ops.mesh_hook_round(torch.zeros((1, 3), dtype=torch.int32), 3, torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.uint8),
                            torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="cuda"):
        ops.mesh_filter(torch.zeros((1, 3), dtype=torch.int32), 3)


def test_entry_points_validate_without_a_gpu():
    """The C entries refuse bad arguments before anything is launched."""
    import ctypes
    from robustmvd_amd import _lib
    lib = _lib.load()
    word = (ctypes.c_int * 4)()
    p = ctypes.cast(word, ctypes.c_void_p)
    assert lib.mvd_mesh_hook_round(None, -1, 3, 1, p, p, p, None) != 0 and b"triangles" in lib.mvd_last_error()
    assert lib.mvd_mesh_hook_round(None, 0, 3, 1, None, None, p, None) != 0
    assert lib.mvd_mesh_component_rank(p, p, 3, p, None, None, 0, None) != 0
    assert lib.mvd_mesh_component_table(p, p, 1, 3, 4, p, p, None) != 0 and b"components" in lib.mvd_last_error()
    assert lib.mvd_mesh_component_sums_f64(p, 3, p, 1, p, p, 2, p, p, None, 0, None) != 0
    assert lib.mvd_mesh_filter(p, 1, 3, None, None, 0, 1, 0, None, None, None, 0, None, None, 0, None) != 0
    assert lib.mvd_mesh_gather_rows_f32(p, p, 3, 0, 3, p, None) != 0 and b"columns" in lib.mvd_last_error()
    assert lib.mvd_mesh_gather_rows_f32(p, p, 2 ** 20, 4096, 3, p, None) != 0 and b"M k" in lib.mvd_last_error()
    assert lib.mvd_mesh_vertex_normals_f32(p, 3, p, 2 ** 30, p, p, p, None) != 0 and b"3 T" in lib.mvd_last_error()
    assert lib.mvd_mesh_component_rank_workspace_bytes(0) == 0 and lib.mvd_mesh_component_rank_workspace_bytes(1000) >= 4000
    assert lib.mvd_mesh_filter_workspace_bytes(1000, 2000) >= 1000
    assert lib.mvd_mesh_component_sums_workspace_bytes(5000, 3) >= 5000 * 8
