"""CPU checks of the mesh simplification's numpy forms (robustmvd_amd/mesh_simplify.py): the invariants of the result, the distance
bound, a slow per-cluster restatement, the placement flags, the quadric's gain on the sphere, the argument errors, the public entry
points on host arrays, and the margins test_hip_mesh_simplify.py relies on."""
import numpy as np
import pytest

import mesh_cases as MC_
import mesh_simplify_cases as SC
import render_cases as RC
import robustmvd_amd as R
from robustmvd_amd import mesh_simplify as MS

SETTINGS = (dict(), dict(placement="mean"), dict(unique=False), dict(remove_unreferenced=False), dict(unique=False, remove_unreferenced=False))
MARGIN = 1e6  # a threshold is "far" from a value when it is this many sum-order effects away


def rotated(t):
    first = np.argmin(t, axis=1)
    return np.take_along_axis(t, (first[:, None] + np.arange(3)) % 3, axis=1)


@pytest.mark.parametrize("name", SC.NAMES)
def test_invariants(name):
    case = SC.cases()[name]
    M, T = len(case["vertices"]), len(case["triangles"])
    for kw in SETTINGS:
        r = SC.result(name, **kw)
        v, t = r.mesh.vertices, r.mesh.triangles
        assert v.dtype == np.float32 and t.dtype == np.int32 and r.vertex_map.dtype == np.int32 and r.kept_triangles.dtype == np.int32
        assert r.placed.dtype == np.uint8 and r.placed.shape == (len(v),) and r.cluster_counts.shape == (len(v),)
        assert len(t) <= T and len(r.kept_triangles) == len(t) and r.vertex_map.shape == (M,)
        assert (np.diff(r.kept_triangles) > 0).all()
        if len(t):
            assert t.min() >= 0 and t.max() < len(v)
            assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 0] != t[:, 2]).all()
            if kw.get("unique", True):
                assert len(np.unique(rotated(t), axis=0)) == len(t)
        if kw.get("remove_unreferenced", True):
            assert np.array_equal(np.unique(t), np.arange(len(v)))
        assert r.vertex_map.max(initial=-1) < len(v)
        if kw.get("placement") == "mean":
            assert np.isin(r.placed, (0, 2)).all()
        assert (r.placed[r.cluster_counts == 1] == 2).all() and (r.placed[r.cluster_counts > 1] != 2).all()
        # the kept triangles are the input's, through the map
        assert np.array_equal(rotated(r.vertex_map[case["triangles"][r.kept_triangles].astype(np.int64)].reshape(-1, 3)), rotated(t).reshape(-1, 3))


@pytest.mark.parametrize("name", SC.NAMES)
def test_every_vertex_stays_within_its_cell(name):
    case, ref = SC.cases()[name], SC.reference(name)
    c = float(np.float32(case["cell"]))
    for placement in MS.PLACEMENTS:
        r = SC.result(name, placement=placement, remove_unreferenced=False)
        vc = ref["clusters"].vertex_cluster
        assert np.array_equal(r.vertex_map, vc)
        ok = vc >= 0
        d = np.linalg.norm(case["vertices"][ok].astype(np.float64) - r.mesh.vertices[vc[ok]].astype(np.float64), axis=1)
        assert (d <= np.sqrt(3.0) * c * (1 + 2.0 ** -20)).all(), (name, placement, float(d.max()), c)


def slow_simplify(v, t, cell, origin, placement="quadric", reg=1e-3, unique=True, remove_unreferenced=True):
    """The definition once more, cluster by cluster and corner by corner in Python loops over float64 scalars."""
    f = np.float64
    c = f(np.float32(cell))
    finite = np.isfinite(v).all(axis=1)
    o = v[finite].min(axis=0).astype(f) if origin is None else np.asarray(origin, dtype=f)
    inv = f(1.0) / c
    cells = {}
    for i in range(len(v)):
        if finite[i]:
            idx = tuple(int(np.floor((f(v[i, a]) - o[a]) * inv)) for a in range(3))
            cells.setdefault(idx, []).append(i)
    order = sorted(cells)  # ascending (x, y, z) = ascending key
    cluster = {i: k for k, idx in enumerate(order) for i in cells[idx]}
    K = len(order)
    ctr = [[(f(idx[a]) + f(0.5)) * c + o[a] for a in range(3)] for idx in order]
    mean = []
    for idx in order:
        s = [f(0.0)] * 3
        for i in cells[idx]:
            s = [s[a] + f(v[i, a]) for a in range(3)]
        mean.append([s[a] / f(len(cells[idx])) for a in range(3)])
    Q = [[f(0.0)] * 10 for _ in range(K)]
    for tri in t:
        if not all(int(i) in cluster for i in tri):
            continue
        p = [[f(v[int(i), a]) for a in range(3)] for i in tri]
        e1, e2 = [p[1][a] - p[0][a] for a in range(3)], [p[2][a] - p[0][a] for a in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        for i in tri:
            k = cluster[int(i)]
            q = [p[0][a] - ctr[k][a] for a in range(3)]
            d = -((n[0] * q[0] + n[1] * q[1]) + n[2] * q[2])
            terms = [n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2], n[0] * d, n[1] * d, n[2] * d, d * d]
            Q[k] = [Q[k][j] + terms[j] for j in range(10)]
    pos, placed = np.zeros((K, 3), np.float32), np.zeros(K, np.uint8)
    for k, idx in enumerate(order):
        pos[k] = [np.float32(m) for m in mean[k]]
        if len(cells[idx]) == 1:
            pos[k], placed[k] = v[cells[idx][0]], 2
            continue
        if placement != "quadric":
            continue
        a00, a01, a02, a11, a12, a22, b0, b1, b2, _ = Q[k]
        lam = f(reg) * ((a00 + a11) + a22)
        d00, d11, d22 = a00 + lam, a11 + lam, a22 + lam
        r = [-b + lam * (mean[k][a] - ctr[k][a]) for a, b in enumerate((b0, b1, b2))]
        C00, C01, C02 = d11 * d22 - a12 * a12, a02 * a12 - a01 * d22, a01 * a12 - a02 * d11
        C11, C12, C22 = d00 * d22 - a02 * a02, a01 * a02 - d00 * a12, d00 * d11 - a01 * a01
        det = (d00 * C00 + a01 * C01) + a02 * C02
        with np.errstate(all="ignore"):
            x = [((C00 * r[0] + C01 * r[1]) + C02 * r[2]) / det, ((C01 * r[0] + C11 * r[1]) + C12 * r[2]) / det,
                 ((C02 * r[0] + C12 * r[1]) + C22 * r[2]) / det]
        if lam > 0 and np.isfinite(det) and det > 0 and all(np.isfinite(xi) and abs(xi) <= f(0.5) * c for xi in x):
            pos[k], placed[k] = [np.float32(ctr[k][a] + x[a]) for a in range(3)], 1
    seen, kept, triples = set(), [], []
    for ti, tri in enumerate(t):
        if not all(int(i) in cluster for i in tri):
            continue
        cl = [cluster[int(i)] for i in tri]
        if len(set(cl)) < 3:
            continue
        s = cl.index(min(cl))
        rot = tuple(cl[s:] + cl[:s])
        if unique and rot in seen:
            continue
        seen.add(rot)
        kept.append(ti)
        triples.append(rot)
    used = sorted({k for tr in triples for k in tr}) if remove_unreferenced else list(range(K))
    new = {k: i for i, k in enumerate(used)}
    out_t = np.array([[new[k] for k in tr] for tr in triples], dtype=np.int32).reshape(-1, 3)
    vmap = np.array([new.get(cluster[i], -1) if i in cluster else -1 for i in range(len(v))], dtype=np.int32)
    counts = np.array([len(cells[order[k]]) for k in used], dtype=np.int32)
    return pos[used].reshape(-1, 3), out_t, vmap, np.array(kept, dtype=np.int32), placed[used], counts


@pytest.mark.parametrize("name", SC.NAMES)
def test_equals_the_slow_restatement(name):
    case = SC.cases()[name]
    for kw in (dict(), dict(placement="mean", unique=False), dict(remove_unreferenced=False)):
        r = SC.result(name, **kw)
        sv, st, smap, skept, splaced, scounts = slow_simplify(case["vertices"], case["triangles"], case["cell"], case["origin"],
                                                              kw.get("placement", "quadric"), 1e-3, kw.get("unique", True),
                                                              kw.get("remove_unreferenced", True))
        assert np.array_equal(r.mesh.triangles, st) and np.array_equal(r.kept_triangles, skept) and np.array_equal(r.vertex_map, smap), name
        assert np.array_equal(r.placed, splaced) and np.array_equal(r.cluster_counts, scounts), name
        assert np.array_equal(r.mesh.vertices.view(np.uint32), sv.view(np.uint32)), name


def test_case_properties():
    """What each case is there for."""
    counts = np.concatenate([SC.reference(f"sphere_c{c:g}")["corner_counts"] for c in SC.SPHERE_CELLS])
    assert (counts <= 64).any() and (counts > 64).any() and (counts > 256).any()
    for c in SC.SPHERE_CELLS:
        vc = SC.reference(f"sphere_c{c:g}")["clusters"].counts
        print(f"\nsphere cell {c:g}: K = {len(vc)}, vertices per cluster up to {vc.max()}, corners up to {SC.reference(f'sphere_c{c:g}')['corner_counts'].max()}")
    assert max(SC.reference(f"sphere_c{c:g}")["clusters"].counts.max() for c in SC.SPHERE_CELLS) > 64  # the means' wave path
    for K in MC_.CHUNK_SWEEP:
        assert SC.reference(f"sheet_K{K}")["clusters"].num_clusters == K
        assert len(SC.result(f"sheet_K{K}").mesh.triangles) > 0
    # identity: every vertex its own cluster, kept bit for bit, in key order
    case, ref, r = SC.cases()["identity"], SC.reference("identity"), SC.result("identity", remove_unreferenced=False)
    assert ref["clusters"].num_clusters == len(case["vertices"]) and (r.placed == 2).all() and len(r.mesh.triangles) == len(case["triangles"])
    assert np.array_equal(r.mesh.vertices.view(np.uint32), case["vertices"][ref["clusters"].order].view(np.uint32))
    assert np.array_equal(r.mesh.triangles, rotated(r.vertex_map[case["triangles"].astype(np.int64)]))
    # one cell
    r = SC.result("one_cell")
    assert SC.reference("one_cell")["clusters"].num_clusters == 1 and r.mesh.triangles.shape == (0, 3) and r.mesh.vertices.shape == (0, 3)
    assert (r.vertex_map == -1).all()
    assert SC.result("one_cell", remove_unreferenced=False).mesh.vertices.shape == (1, 3)
    # double sided: the repeated sheet's triangles go, the flipped one's stay
    case = SC.cases()["double_sided"]
    T = len(case["triangles"]) // 3
    r, every = SC.result("double_sided"), SC.result("double_sided", unique=False)
    first, second, third = (int(((k >= a * T) & (k < (a + 1) * T)).sum()) for k in (r.kept_triangles,) for a in range(3))
    e1, e2, e3 = (int(((k >= a * T) & (k < (a + 1) * T)).sum()) for k in (every.kept_triangles,) for a in range(3))
    assert first == e1 > 0 and second < e2 and third > 0 and len(every.kept_triangles) > len(r.kept_triangles)
    flipped = {tuple(x) for x in rotated(r.mesh.triangles[:, ::-1]).tolist()}
    assert flipped & {tuple(x) for x in r.mesh.triangles.tolist()}  # both orientations of a triple are there
    # nonfinite: the invalid vertices have no cluster, their triangles are gone
    case, r = SC.cases()["nonfinite"], SC.result("nonfinite")
    bad = ~np.isfinite(case["vertices"]).all(axis=1)
    assert bad.sum() == 2 and (r.vertex_map[bad] == -1).all() and np.isfinite(r.mesh.vertices).all()
    assert not np.isin(case["triangles"][r.kept_triangles], np.flatnonzero(bad)).any()
    # unreferenced: the far vertex's cluster goes with remove_unreferenced, and stays without
    case, r = SC.cases()["unreferenced"], SC.result("unreferenced")
    assert r.vertex_map[len(case["vertices"]) - 2] == -1 and r.vertex_map[len(case["vertices"]) - 1] >= 0
    keep = SC.result("unreferenced", remove_unreferenced=False)
    assert keep.vertex_map[len(case["vertices"]) - 2] >= 0 and keep.placed[keep.vertex_map[len(case["vertices"]) - 2]] == 2


def test_planar_patch_is_placed_by_the_regularisation():
    case, ref = SC.cases()["planar"], SC.reference("planar")
    r = SC.result("planar", remove_unreferenced=False)
    Q, cl = ref["quadrics"], ref["clusters"]
    assert (Q[:, [0, 1, 2, 3, 4]] == 0).all() and (Q[:, 5] > 0).all()  # n = (0, 0, nz): rank 1
    assert (r.placed == 1).all()
    assert np.array_equal(r.mesh.vertices[:, 2], np.full(len(r.mesh.vertices), np.float32(0.375)))  # on the plane
    # in the plane nothing but the regularisation acts: the mean's coordinates
    assert np.abs(r.mesh.vertices[:, :2].astype(np.float64) - ref["means"][:, :2]).max() <= 2.0 ** -22 * 16
    assert cl.num_clusters == 20


def test_quadric_beats_the_mean_on_the_sphere():
    for c in SC.SPHERE_CELLS:
        q, m = SC.result(f"sphere_c{c:g}"), SC.result(f"sphere_c{c:g}", placement="mean")
        eq, em = SC.sphere_error(q.mesh.vertices), SC.sphere_error(m.mesh.vertices)
        print(f"\nsphere cell {c:g}: {len(q.mesh.vertices)} vertices, {len(q.mesh.triangles)} triangles, placed {np.bincount(q.placed, minlength=3).tolist()}, "
              f"mean | |v - centre| - r |: quadric {eq:.5f}, mean {em:.5f} voxels")
        assert np.array_equal(q.mesh.triangles, m.mesh.triangles)
        assert eq < em


def test_argument_errors():
    v, t = MC_.degenerate()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell"):
            R.simplify_mesh((v, t), bad)
        with pytest.raises(ValueError, match="regularisation"):
            R.simplify_mesh((v, t), 0.5, regularisation=bad)
    with pytest.raises(ValueError, match="placement"):
        R.simplify_mesh((v, t), 0.5, placement="median")
    with pytest.raises(ValueError, match="float32"):
        R.simplify_mesh((v.astype(np.float64), t), 0.5)
    with pytest.raises(ValueError, match="vertex indices"):
        R.simplify_mesh((v, t + 5), 0.5)
    with pytest.raises(ValueError, match="attributes"):
        R.simplify_mesh((v, t), 0.5, attributes=[np.zeros((len(v) + 1, 2), np.float32)])
    with pytest.raises(ValueError, match=r"must be in \[0"):
        R.simplify_mesh((v, t), 1e-9)
    with pytest.raises(ValueError, match=r"must be in \[0"):
        R.simplify_mesh((v, t), 0.5, origin=(5.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="origin"):
        R.simplify_mesh((v, t), 0.5, origin=(0.0, float("nan"), 0.0))
    with pytest.raises(ValueError):
        R.simplify_mesh(v, 0.5)


def test_public_entry_points_on_host_arrays():
    for name in ("simplify_mesh", "simplify_numpy", "cluster_numpy", "cluster_quadrics_numpy", "place_numpy", "SimplifyResult", "mesh_simplify"):
        assert hasattr(R, name)
    v, t, colors = SC.sphere()
    mesh = R.Mesh(v, t, colors)
    mesh.normals = mesh.vertex_normals()
    ref = SC.result("sphere_c3")
    out = mesh.simplify(3.0)
    assert isinstance(out, R.Mesh) and np.array_equal(out.triangles, ref.mesh.triangles)
    assert np.array_equal(out.vertices.view(np.uint32), ref.mesh.vertices.view(np.uint32))
    assert out.colors.dtype == np.float32 and out.colors.shape == out.vertices.shape and out.colors.min() >= 0 and out.colors.max() <= 255
    assert np.array_equal(out.normals, R.vertex_normals(out.vertices, out.triangles))
    assert np.abs(np.linalg.norm(out.normals, axis=1) - 1).max() < 1e-6
    plain = R.Mesh(v, t).simplify(3.0)
    assert plain.colors is None and plain.normals is None
    full = mesh.simplify(3.0, attributes={"id": np.arange(len(v), dtype=np.float32)[:, None]}, details=True)
    assert isinstance(full, R.SimplifyResult) and set(full.attributes) == {"id"} and np.array_equal(full.vertex_map, ref.vertex_map)
    # an attribute's mean: of the vertex indices, through the map
    want = np.array([np.flatnonzero(full.vertex_map == k).astype(np.float64).mean() for k in range(len(full.mesh.vertices))])
    assert np.abs(full.attributes["id"][:, 0] - want).max() <= 1502 * 2.0 ** -23
    assert np.array_equal(full.cluster_counts, np.bincount(full.vertex_map[full.vertex_map >= 0], minlength=len(full.mesh.vertices)))
    as_list = R.simplify_mesh((v, t), 3.0, attributes=[colors])
    assert np.array_equal(as_list.attributes[0], out.colors) and as_list.mesh.colors is None
    # the volume's path: simplify after clean, and the default None changes nothing
    F, Wt = MC_.blob_volume()
    vol = R.TSDFVolume.from_arrays(F, Wt, origin=RC.SPHERE_ORIGIN, voxel=RC.SPHERE_VOXEL)
    raw = vol.extract_mesh()
    same = vol.extract_mesh(simplify=None)
    assert np.array_equal(raw.vertices, same.vertices) and np.array_equal(raw.triangles, same.triangles)
    m = vol.extract_mesh(clean=dict(keep_largest=1), simplify=dict(cell=0.3))
    two = vol.extract_mesh(clean=dict(keep_largest=1)).simplify(0.3)
    assert np.array_equal(m.vertices, two.vertices) and np.array_equal(m.triangles, two.triangles) and 0 < len(m.triangles) < 3000
    assert np.array_equal(np.unique(m.triangles), np.arange(len(m.vertices)))  # no manifold promise: only that nothing dangles
    with pytest.raises(ValueError, match="simplify takes"):
        vol.extract_mesh(simplify=dict(cell=0.3, details=True))
    with pytest.raises(ValueError, match="simplify takes"):
        vol.extract_mesh(simplify=dict(placement="mean"))


def reversed_sums(ref):
    """The quadrics and the means with every segment added in the opposite order."""
    case, cl = ref["case"], ref["clusters"]
    K = cl.num_clusters
    key, terms = MS.corner_terms_numpy(case["vertices"], case["triangles"], cl)
    ok = key < K
    k, w = key[ok][::-1], terms[ok][::-1]
    Q = np.stack([np.bincount(k, weights=w[:, j], minlength=K) for j in range(10)], axis=1) if K else np.zeros((0, 10))
    lab, rows = cl.vertex_cluster[cl.order][::-1], case["vertices"][cl.order].astype(np.float64)[::-1]
    mean = np.stack([np.bincount(lab, weights=rows[:, j], minlength=K) for j in range(3)], axis=1) / cl.counts[:, None] if K else np.zeros((0, 3))
    return Q, mean


@pytest.mark.parametrize("name", SC.NAMES)
def test_margins_the_gpu_test_relies_on(name):
    """test_hip_mesh_simplify.py asserts that the device's `placed` equals numpy's although the device adds long segments in another
    order.  That holds when every decision of step 5 is far from its threshold: here, MARGIN times the effect of adding every segment
    in the opposite order, which is at least as large a reordering as the device's."""
    ref = SC.reference(name)
    case, cl = ref["case"], ref["clusters"]
    if cl.num_clusters == 0:
        return
    Qr, mr = reversed_sums(ref)
    _, pf, f = MS.place_numpy(case["vertices"], case["triangles"], cl, quadrics=ref["quadrics"], means=ref["means"], details=True)
    _, pr, r = MS.place_numpy(case["vertices"], case["triangles"], cl, quadrics=Qr, means=mr, details=True)
    _, pd, d = MS.place_numpy(case["vertices"], case["triangles"], cl, quadrics=ref["device_quadrics"], means=ref["device_means"], details=True)
    assert np.array_equal(pf, pr) and np.array_equal(pf, pd)
    many = cl.counts > 1
    assert np.array_equal(f["lam"] > 0, r["lam"] > 0) and ((f["lam"] > 0) | (f["lam"] == 0)).all()
    live = many & (f["lam"] > 0)
    if not live.any():
        return
    half = 0.5 * cl.c
    det_effect = np.abs(f["det"] - r["det"])[live]
    x_effect = np.abs(f["x"] - r["x"])[live]
    det_margin = np.abs(f["det"])[live]
    x_margin = np.abs(np.abs(f["x"]) - half)[live]
    with np.errstate(all="ignore"):
        print(f"\n{name}: {int(live.sum())} solved clusters, placed {np.bincount(pf, minlength=3).tolist()}, smallest det margin / effect "
              f"{float((det_margin / np.maximum(det_effect, 1e-300)).min()):.3g}, smallest | |x| - c/2 | margin / effect "
              f"{float((x_margin / np.maximum(x_effect, 1e-300)).min()):.3g}, largest x effect {float(x_effect.max() / cl.c):.3g} cells")
    assert np.isfinite(f["det"][live]).all() and (f["det"][live] > 0).all()
    assert (det_margin >= MARGIN * det_effect).all()
    assert (x_margin >= MARGIN * x_effect).all()
