"""Cases for the mesh clean-up tests (test_mesh_clean_cpu.py, test_hip_mesh_clean.py): the smallest meshes at which the kernels of
csrc/mesh_clean.hip can go wrong, and the bounds both suites share.  Everything is built once (treat the arrays as read-only).

A case is (vertices (M,3) float32, triangles (T,3) int32).  Strips are quad strips (two rows of vertices, two triangles per quad)
with the vertex numbering and the triangle order shuffled: one component whose diameter is M / 2, the worst case for a labelling
that spreads one edge per round.
"""
import functools
import math

import numpy as np

import tsdf_cases as TC
from robustmvd_amd import mesh_clean as MC
from robustmvd_amd import tsdf as TS

CHUNK_SWEEP = (63, 64, 65, 255, 256, 257, 1025)  # compact.h's 64 / 256 chunk edges and its 1024-chunk block, in triangles
STRIP_M = (1026, 16386)  # both suites
STRIP_M_GPU = 262146  # the GPU suite only
F32_EPS = 2.0 ** -23


def _f(a):
    return np.asarray(a, dtype=np.float32).reshape(-1, 3)


def _i(a):
    return np.asarray(a, dtype=np.int32).reshape(-1, 3)


def strip_arrays(num_triangles, seed, shuffle=True):
    """The first num_triangles triangles of a quad strip -> (vertices, triangles).  Vertex (i, r) of the unshuffled strip is 2 i + r."""
    q = (num_triangles + 1) // 2
    M = 2 * (q + 1)
    rng = np.random.default_rng(seed)
    i = np.arange(M) // 2
    v = np.stack([i * 0.5 + rng.uniform(-0.1, 0.1, M), (np.arange(M) % 2) + rng.uniform(-0.1, 0.1, M), rng.uniform(-0.2, 0.2, M)], axis=1)
    a = 2 * np.arange(q)
    t = np.stack([np.stack([a, a + 2, a + 1], axis=1), np.stack([a + 1, a + 2, a + 3], axis=1)], axis=1).reshape(-1, 3)[:num_triangles]
    if shuffle:
        number = rng.permutation(M)  # old vertex -> new index
        pos = np.empty_like(v)
        pos[number] = v
        v, t = pos, number[t][rng.permutation(len(t))]
    return _f(v), _i(t)


@functools.lru_cache(maxsize=None)
def strip(M):
    """A shuffled quad strip of M vertices (M even): M - 2 triangles, one component."""
    v, t = strip_arrays(M - 2, seed=M)
    assert len(v) == M
    return v, t


@functools.lru_cache(maxsize=None)
def all_separate():
    """1000 triangles on 3000 distinct shuffled vertices and 7 unreferenced ones: C = T."""
    rng = np.random.default_rng(5)
    M = 3007
    t = rng.permutation(M)[:3000].reshape(1000, 3)
    return _f(rng.uniform(-1, 1, (M, 3))), _i(t)


@functools.lru_cache(maxsize=None)
def interleaved():
    """Two strips of 700 triangles whose triangles alternate in the list: both components straddle every workgroup."""
    va, ta = strip_arrays(700, seed=11)
    vb, tb = strip_arrays(700, seed=12)
    t = np.stack([ta, tb + len(va)], axis=1).reshape(-1, 3)
    return _f(np.concatenate([va, vb + np.float32(3.0)])), _i(t)


@functools.lru_cache(maxsize=None)
def degenerate():
    """(i,i,j), (i,i,i), a triangle listed twice, a non-manifold edge (5,6) shared by three triangles, an unreferenced vertex 4."""
    rng = np.random.default_rng(7)
    t = [[0, 0, 1], [2, 2, 2], [1, 3, 1], [5, 6, 7], [5, 6, 8], [6, 5, 9], [10, 11, 12], [10, 11, 12], [12, 13, 10]]
    return _f(rng.uniform(-1, 1, (14, 3))), _i(t)


@functools.lru_cache(maxsize=None)
def nonfinite():
    """A strip of 40 triangles with a NaN and an inf vertex: connectivity ignores them, their triangles' areas are 0."""
    v, t = strip_arrays(40, seed=3)
    v = v.copy()
    v[int(t[5, 0])] = np.nan
    v[int(t[30, 1]), 1] = np.inf
    return v, t


def _tetrahedron(centre, r):
    c = np.asarray(centre, dtype=np.float64)
    v = c + r * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64)
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])  # closed, outward


SPHERE_CENTRE = TC.SPHERE[1]
NUM_FLOATERS = 3


@functools.lru_cache(maxsize=None)
def sphere_with_floaters():
    """tsdf_cases.sphere_volume()'s mesh (1502 vertices, 3000 triangles) with three tetrahedra: one's vertices in front of the
    sphere's in the vertex list (so that every kept index moves), two behind; their triangles at the start, in the middle and at
    the end of the triangle list.  -> (vertices, triangles, colors, the sphere's own (vertices, triangles))."""
    F, Wt = TC.sphere_volume()
    sv, _, st = TS.extract_numpy(F, Wt)
    sv, st = sv.astype(np.float32), st.astype(np.int64)
    assert sv.shape == (1502, 3) and st.shape == (3000, 3)
    tets = [_tetrahedron((1.0, 1.0, 1.0), 0.4), _tetrahedron((16.0, 2.0, 3.0), 0.3), _tetrahedron((2.0, 16.0, 15.0), 0.2)]
    v = np.concatenate([tets[0][0], sv, tets[1][0], tets[2][0]])
    t = np.concatenate([tets[0][1], st[:1500] + 4, tets[1][1] + 4 + 1502, st[1500:] + 4, tets[2][1] + 4 + 1502 + 4])
    v = _f(v)
    colors = _f(np.random.default_rng(9).uniform(0, 255, v.shape))
    return v, _i(t), colors, (sv, _i(st))


@functools.lru_cache(maxsize=None)
def blob_volume():
    """sphere_volume() with two small closed blobs written into the same volume before extraction -> (tsdf, weight)."""
    F, Wt = TC.sphere_volume()
    F = F.copy()
    for (i, j, k) in ((1, 1, 1), (16, 15, 2)):
        F[k, j, i] = -0.5  # one inside voxel far from the sphere: an octahedron-like blob around it
    return F, Wt


def small_cases():
    """name -> (vertices, triangles)"""
    cases = {
        "empty_M0": (_f([]), _i([])),
        "empty_M5": (_f(np.arange(15)), _i([])),
        "one": (_f([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), _i([[0, 1, 2]])),
        "no_triangle_names_most": (_f(np.arange(30) % 7), _i([[8, 2, 5]])),
        "all_separate": all_separate(),
        "interleaved": interleaved(),
        "degenerate": degenerate(),
        "nonfinite": nonfinite(),
        "floaters": sphere_with_floaters()[:2],
    }
    for T in CHUNK_SWEEP:
        cases[f"strip_T{T}"] = strip_arrays(T, seed=T)
    for M in STRIP_M:
        cases[f"strip_M{M}"] = strip(M)
    return cases


@functools.lru_cache(maxsize=None)
def reference(name):
    """The numpy forms on a case, computed once -> dict"""
    v, t = strip(STRIP_M_GPU) if name == f"strip_M{STRIP_M_GPU}" else small_cases()[name]
    table = MC.component_table_numpy(v, t)
    return {"vertices": v, "triangles": t, "label": MC.components_numpy(t, len(v)), "table": table,
            "normals": MC.vertex_normals_numpy(v, t), "triangle_area": MC.triangle_areas_numpy(v, t)}


def area_bounds(table, triangle_area):
    """Per component: (math.fsum of its triangles' areas, the bound (n + 16) 2^-52 sum: n additions and a generous 16 roundings for
    the cross product, the square root and the halving of each term)."""
    tc = np.asarray(table.triangle_component)
    exact, bound = [], []
    for c in range(table.num_components):
        a = triangle_area[tc == c]
        s = math.fsum(a.tolist())
        exact.append(s)
        bound.append((len(a) + 16) * 2.0 ** -52 * s)
    return np.asarray(exact), np.asarray(bound)


def f32_ulp(x):
    """The spacing of float32 at |x| (x float32), at least the smallest normal's."""
    x = np.abs(np.asarray(x, dtype=np.float32))
    return np.maximum(np.spacing(x), np.float32(2.0 ** -149)).astype(np.float64)
