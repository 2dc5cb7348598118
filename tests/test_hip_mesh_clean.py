"""GPU checks of the mesh clean-up kernels (csrc/mesh_clean.hip) against the numpy forms of robustmvd_amd/mesh_clean.py: integers equal,
kept vertices and attributes bit for bit, areas within the fsum bound, two runs bit-identical.  The vertex normals' float64 chain (no
contraction, correctly rounded square root and division) turned out bit-equal to numpy on the device on every case, so the test asserts
equal bits instead of the one-ulp band the last rounding would allow."""
import numpy as np
import pytest
import torch

import mesh_cases as MC_
import render_cases as RC
import tsdf_cases as TC
import robustmvd_amd as R
from robustmvd_amd import mesh_clean as MC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = sorted(MC_.small_cases())


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def down(t):
    return t.cpu().numpy()


def bits(t):
    a = down(t)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def check_table(ref, got, what):
    table = ref["table"]
    for name in ("vertex_component", "triangle_component", "num_triangles", "num_vertices"):
        g = down(getattr(got, name))
        assert g.dtype == np.int32 and np.array_equal(g, getattr(table, name)), f"{what}: {name}"
    exact, bound = MC_.area_bounds(table, ref["triangle_area"])
    area = down(got.area)
    assert area.dtype == np.float64 and area.shape == exact.shape
    if len(area):
        print(f"\n{what}: C = {len(area)}, rounds {got.rounds} (numpy {table.rounds}), area |device - fsum| / bound "
              f"{float((np.abs(area - exact) / np.maximum(bound, 1e-300)).max()):.3f}, bit-equal to numpy {np.array_equal(area, table.area)}")
    assert (np.abs(area - exact) <= bound).all(), what
    assert 1 <= got.rounds <= MC.max_rounds(len(ref["vertices"]))


def check_normals(ref, got, what):
    want = ref["normals"].astype(np.float32)
    g = down(got)
    assert g.dtype == np.float32 and g.shape == want.shape
    zero = (ref["normals"] == 0).all(axis=1)
    assert (g[zero] == 0).all(), what
    if len(g):
        ulps = np.abs(g.astype(np.float64) - want.astype(np.float64)) / MC_.f32_ulp(want)
        print(f"\n{what}: normals max {float(ulps.max()):.2f} ulp, bit-equal {np.array_equal(g.view(np.uint32), want.view(np.uint32))}")
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), what


@pytest.mark.parametrize("name", CASES)
def test_components_table_and_normals(name):
    ref = MC_.reference(name)
    v, t = up(ref["vertices"]), up(ref["triangles"])
    got = R.mesh_components(v, t)
    check_table(ref, got, name)
    normals = R.vertex_normals(v, t)
    check_normals(ref, normals, name)
    # labels: the lowest vertex of the component
    from robustmvd_amd.mesh_clean import _labels_device
    label, referenced, _ = _labels_device(t, len(ref["vertices"]))
    assert np.array_equal(down(label), ref["label"])
    assert np.array_equal(down(referenced) != 0, ref["table"].vertex_component >= 0)
    # two runs: the same bits, areas and normals included
    again = R.mesh_components(v, t)
    assert np.array_equal(bits(again.area), bits(got.area)) and np.array_equal(down(again.vertex_component), down(got.vertex_component))
    assert np.array_equal(bits(R.vertex_normals(v, t)), bits(normals))


@pytest.mark.parametrize("M", MC_.STRIP_M + (MC_.STRIP_M_GPU,))
def test_strip_rounds(M):
    """The long-diameter case.  Measured rounds, the unchanged last one included, numpy form / device: M = 1026: 8 / 7, 16386: 10 / 8,
    262146: 14 / 10 (caps 26, 34, 42).  The device needs fewer: a hook that lands early in a launch is seen by the later ones."""
    ref = MC_.reference(f"strip_M{M}")
    got = R.mesh_components(up(ref["vertices"]), up(ref["triangles"]))
    print(f"\nstrip M = {M}: device {got.rounds} rounds, numpy {ref['table'].rounds}, cap {MC.max_rounds(M)}")
    assert (down(got.vertex_component) == 0).all() and got.num_components == 1
    assert got.rounds <= MC.max_rounds(M)
    assert got.rounds <= 2 * ref["table"].rounds + 2
    if M == MC_.STRIP_M_GPU:
        check_table(ref, got, f"strip_M{M}")  # one segment of 262144 triangles: whole blocks, a head and a tail
        check_normals(ref, R.vertex_normals(up(ref["vertices"]), up(ref["triangles"])), f"strip_M{M}")


def clean_both(v, t, attrs, **kw):
    host = R.clean_mesh((v, t), attributes=attrs, **kw)
    dev = R.clean_mesh((up(v), up(t)), attributes=[up(a) for a in attrs], **kw)
    return host, dev


def assert_clean_equal(host, dev, what):
    assert np.array_equal(down(dev.mesh.triangles), host.mesh.triangles), what
    assert down(dev.mesh.triangles).dtype == np.int32
    assert np.array_equal(down(dev.kept_triangles), host.kept_triangles) and np.array_equal(down(dev.vertex_remap), host.vertex_remap), what
    assert np.array_equal(bits(dev.mesh.vertices), host.mesh.vertices.view(np.uint32)), what
    for a, b in zip(dev.attributes, host.attributes):
        assert np.array_equal(bits(a), b.view(np.uint32)), what


@pytest.mark.parametrize("name", CASES)
def test_clean_equals_numpy(name):
    ref = MC_.reference(name)
    v, t, table = ref["vertices"], ref["triangles"], ref["table"]
    attrs = [np.random.default_rng(1).standard_normal((len(v), 3)).astype(np.float32), np.arange(len(v) * 5, dtype=np.float32).reshape(-1, 5)]
    attrs[0][::7] = np.nan  # bit for bit
    settings = [dict(), dict(remove_unreferenced=False), dict(keep_largest=1), dict(keep_largest=2, remove_unreferenced=False),
                dict(min_triangles=3), dict(min_triangles=4, keep_largest=3)]
    # thresholds no component's numpy area lies within 1e-9 relative of: asserted here for the numpy values alone
    clear = lambda thr: bool((np.abs(table.area - thr) > 1e-9 * np.maximum(np.abs(table.area), thr)).all())
    if table.num_components:
        areas = np.sort(np.unique(table.area))
        picks = [0.5 * (areas[len(areas) // 2] + areas[min(len(areas) // 2 + 1, len(areas) - 1)]), 0.75 * areas[-1], 0.0]
        settings += [dict(min_area=float(thr)) for thr in picks if clear(thr)]
        assert len(settings) >= 8 or table.num_components <= 2
    else:
        settings.append(dict(min_area=1.0))  # no component at all: nothing to be near; the filter's C == 0 path with a criterion
    for kw in settings:
        assert "min_area" not in kw or clear(kw["min_area"])  # the numpy areas alone: then device and numpy keep the same components
        host, dev = clean_both(v, t, attrs, **kw)
        assert_clean_equal(host, dev, f"{name} {kw}")
    host, dev = clean_both(v, t, attrs, keep_largest=1)
    again = R.clean_mesh((up(v), up(t)), keep_largest=1, details=True)
    assert np.array_equal(down(again.mesh.triangles), down(dev.mesh.triangles)) and np.array_equal(bits(again.mesh.vertices), bits(dev.mesh.vertices))


def test_arrays_in_different_places():
    v, t = MC_.degenerate()
    with pytest.raises(ValueError, match="different places"):
        R.mesh_components(v, up(t))
    with pytest.raises(ValueError, match="different places"):
        R.clean_mesh((up(v), up(t)), attributes=[np.zeros((len(v), 2), np.float32)])
    with pytest.raises(ValueError, match="different places"):
        R.vertex_normals(up(v), t)
    with pytest.raises(ValueError, match="different places"):
        R.clean_mesh(R.Mesh(up(v), up(t), np.zeros((len(v), 3), np.float32)), keep_largest=1)


def test_floaters_leave_the_sphere():
    v, t, colors, (sv, st) = MC_.sphere_with_floaters()
    mesh = R.Mesh(up(v), up(t), up(colors))
    for kw in (dict(min_triangles=5), dict(keep_largest=1)):
        m = mesh.clean(**kw)
        assert m.vertices.is_cuda and m.triangles.is_cuda and m.colors.is_cuda
        TC.check_closed_surface(down(m.vertices), down(m.triangles), TC.SPHERE[1])
        assert tuple(m.vertices.shape) == (1502, 3) and tuple(m.triangles.shape) == (3000, 3) and len(TC.edge_counts(down(m.triangles))[0]) == 4500
        assert np.array_equal(bits(m.vertices), sv.view(np.uint32)) and np.array_equal(down(m.triangles), st)
        assert np.array_equal(bits(m.colors), colors[4:1506].view(np.uint32))
    comps = mesh.components()
    assert sorted(down(comps.num_triangles).tolist()) == [4, 4, 4, 3000]


def test_extract_mesh_clean_product_path():
    F, Wt = MC_.blob_volume()
    host_vol = R.TSDFVolume.from_arrays(F, Wt, origin=RC.SPHERE_ORIGIN, voxel=RC.SPHERE_VOXEL)
    dev_vol = R.TSDFVolume.from_arrays(up(F), up(Wt), origin=RC.SPHERE_ORIGIN, voxel=RC.SPHERE_VOXEL)
    raw = dev_vol.extract_mesh()
    assert raw.normals is None and tuple(raw.triangles.shape)[0] > 3000
    for kw in (dict(min_triangles=100), dict(keep_largest=1), dict(min_triangles=1, remove_unreferenced=False)):
        m = dev_vol.extract_mesh(clean=kw)
        same = R.clean_mesh(raw, **kw)
        assert np.array_equal(bits(m.vertices), bits(same.vertices)) and np.array_equal(down(m.triangles), down(same.triangles))
        host = host_vol.extract_mesh(clean=kw)
        assert tuple(m.vertices.shape) == host.vertices.shape and np.array_equal(down(m.triangles), host.triangles)
    m = dev_vol.extract_mesh(clean=dict(keep_largest=1))
    TC.check_closed_surface(down(m.vertices), down(m.triangles), RC.SPHERE_CENTRE)
    assert tuple(m.vertices.shape) == (1502, 3) and tuple(m.triangles.shape) == (3000, 3)
    # the default is exactly today's extraction
    plain = dev_vol.extract_mesh(clean=None)
    assert np.array_equal(bits(plain.vertices), bits(raw.vertices)) and np.array_equal(down(plain.triangles), down(raw.triangles))


def test_render_vertex_normals():
    """render_mesh(normals="vertex") on the device against the host path on the three 96 x 131 views of render_cases: the band is the
    one render_cases derives for an interpolated per-vertex attribute (here the vertex normals), the excluded pixels and their cap
    are that file's."""
    H, W = 96, 131
    v, t, c = RC.mesh("sphere")
    Ks, Ts = RC.cameras(H, W)
    vn = MC.vertex_normals_numpy(v, t).astype(np.float32)
    ref = RC.reference_of(v, t, vn, Ks, Ts, (H, W))
    host = R.render_mesh((v, t), Ks, Ts, (H, W), normals="vertex")
    dv, dt, dc = up(v), up(t), up(c)
    dev = R.render_mesh((dv, dt), Ks, Ts, (H, W), normals="vertex", colors=dc)
    assert ref["share"] <= RC.MAX_EXCLUDED_SHARE
    gap = 0.0
    for k in range(len(Ks)):
        keep = ~ref["excluded"][k]
        n, mask = down(dev.normals[k]), ref["r64"].mask[k]
        assert n.dtype == np.float32 and np.array_equal(down(dev.triangle[k])[keep], ref["r64"].triangle[k][keep])
        assert (n[:, keep & ~mask] == 0).all()
        gap = max(gap, float(np.abs(n.astype(np.float64) - host.normals[k])[:, keep].max()) / ref["span"])
        assert np.abs(np.linalg.norm(n[:, keep & mask].astype(np.float64), axis=0) - 1).max() <= 4 * 2.0 ** -24
    print(f"\nsmooth normals: excluded {100 * ref['share']:.3f} %, device - host {gap:.2e} of the span (band {ref['band']['colors']:.2e})")
    assert gap <= ref["band"]["colors"]
    # the colours of the same call, the face normals and the maps of a plain call: today's bits
    plain = R.render_mesh((dv, dt), Ks, Ts, (H, W), colors=dc, normals=True)
    from robustmvd_amd import ops, render
    table = up(np.stack([render.compose_projection(K, T) for K, T in zip(Ks, Ts)]).astype(np.float32))
    raw = ops.mesh_render(dv, dt, table, (H, W), dc, True)
    for k in range(len(Ks)):
        assert np.array_equal(bits(dev.colors[k]), bits(plain.colors[k])) and np.array_equal(bits(dev.depth[k]), bits(plain.depth[k]))
        assert np.array_equal(bits(plain.normals[k]), bits(raw["normals"][k])) and np.array_equal(bits(plain.colors[k]), bits(raw["colors"][k]))
        assert np.array_equal(bits(plain.depth[k]), bits(raw["depth"][k])) and np.array_equal(down(plain.triangle[k]), down(raw["triangle"][k]))
