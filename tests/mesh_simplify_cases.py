"""Cases for the mesh simplification tests (test_mesh_simplify_cpu.py, test_hip_mesh_simplify.py): the smallest meshes at which the
kernels of csrc/mesh_simplify.hip can go wrong, and the numpy reference both suites share.  Everything is built once (treat the arrays
as read-only).

A case is a dict: vertices (M,3) float32, triangles (T,3) int32, cell, origin (None: the default).  Sheets are height fields over
two rows of unit cells, four jittered vertices per cell, with the vertex numbering and the triangle order shuffled; the triangles
that survive are the ones around the points where four cells meet.
"""
import functools

import numpy as np

import mesh_cases as MC_
import sum_order as SO
import tsdf_cases as TC
from robustmvd_amd import mesh_simplify as MS
from robustmvd_amd import tsdf as TS

# In voxels: clusters of a few corners, of about 64, and of several hundred.  The sphere's radius is 5.2: up to an edge of 5 the quadric's
# vertices lie nearer the sphere than the means (test_mesh_simplify_cpu.py), at 6 (8 vertices for the whole sphere) they no longer do.
SPHERE_CELLS = (1.5, 3.0, 4.5)
SPHERE_CENTRE, SPHERE_RADIUS = np.asarray(TC.SPHERE[1], dtype=np.float64), float(TC.SPHERE[2])


def _f(a):
    return np.asarray(a, dtype=np.float32).reshape(-1, 3)


def _i(a):
    return np.asarray(a, dtype=np.int32).reshape(-1, 3)


def sheet_arrays(num_cells, seed, flat=None, shuffle=True):
    """A sheet over num_cells unit cells, ceil(n / 2) in the row y in [0,1) and floor(n / 2) in the row y in [1,2) -> (vertices,
    triangles).  Vertex (i, j) sits at (0.5 i + 0.25, 0.5 j + 0.25) with a jitter of 0.1, so that every cell holds four vertices;
    z is a smooth height with noise, or the constant `flat`."""
    rng = np.random.default_rng(seed)
    n0, n1 = (num_cells + 1) // 2, num_cells // 2
    index, pos = {}, []
    for j in range(4):
        for i in range(2 * (n0 if j < 2 else n1)):
            index[(i, j)] = len(pos)
            x, y = 0.5 * i + 0.25 + rng.uniform(-0.1, 0.1), 0.5 * j + 0.25 + rng.uniform(-0.1, 0.1)
            z = flat if flat is not None else 0.5 + 0.2 * np.sin(0.9 * x) * np.cos(1.3 * y) + rng.uniform(-0.03, 0.03)
            pos.append((x, y, z))
    tri = []
    for (i, j), a in index.items():
        if (i + 1, j) in index and (i, j + 1) in index and (i + 1, j + 1) in index:
            b, c, d = index[(i + 1, j)], index[(i, j + 1)], index[(i + 1, j + 1)]
            tri += [(a, b, c), (b, d, c)]
    v, t = np.asarray(pos), np.asarray(tri).reshape(-1, 3)
    if shuffle:
        number = rng.permutation(len(v))  # old vertex -> new index
        moved = np.empty_like(v)
        moved[number] = v
        v, t = moved, number[t][rng.permutation(len(t))]
    return _f(v), _i(t)


@functools.lru_cache(maxsize=None)
def sphere():
    """tsdf_cases.sphere_volume()'s mesh, in voxels: 1502 vertices, 3000 triangles -> (vertices, triangles, colors)."""
    F, Wt = TC.sphere_volume()
    v, _, t = TS.extract_numpy(F, Wt)
    v, t = _f(v), _i(t)
    assert v.shape == (1502, 3) and t.shape == (3000, 3)
    return v, t, _f(np.random.default_rng(21).uniform(0, 255, v.shape))


def _case(v, t, cell, origin=None):
    return {"vertices": v, "triangles": t, "cell": cell, "origin": origin}


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case"""
    out = {}
    sv, st, _ = sphere()
    for cell in SPHERE_CELLS:
        out[f"sphere_c{cell:g}"] = _case(sv, st, cell)
    for K in MC_.CHUNK_SWEEP:
        out[f"sheet_K{K}"] = _case(*sheet_arrays(K, seed=K), 1.0, (0.0, 0.0, 0.0))
    # nothing at all, and vertices without a triangle: every quadric is zero, every cluster of more than one vertex its mean
    out["empty"] = _case(_f([]), _i([]), 1.0, (0.0, 0.0, 0.0))
    out["no_triangles"] = _case(_f(np.random.default_rng(4).uniform(0, 3, (40, 3))), _i([]), 1.0)
    # a cell smaller than every vertex separation: every vertex its own cluster
    av, at = MC_.all_separate()
    out["identity"] = _case(av, at, 1e-3)
    # every vertex in one cell
    out["one_cell"] = _case(*MC_.strip_arrays(40, seed=3), 100.0)
    # three coincident sheets (their vertices a hair apart): the second repeats the first's orientation, the third is flipped
    dv, dt = sheet_arrays(16, seed=101)
    M = len(dv)
    out["double_sided"] = _case(_f(np.concatenate([dv, dv + np.float32(1e-3), dv - np.float32(1e-3)])),
                                _i(np.concatenate([dt, dt + M, (dt + 2 * M)[:, ::-1]])), 1.0, (-0.5, -0.5, -1.0))
    out["degenerate"] = _case(*MC_.degenerate(), 0.5)
    out["nonfinite"] = _case(*MC_.nonfinite(), 0.7)
    # vertices that no triangle names: one far away in a cell of its own, one inside an occupied cell (it moves that cell's mean)
    uv, ut = sheet_arrays(12, seed=102)
    out["unreferenced"] = _case(_f(np.concatenate([uv, [[40.5, 0.5, 0.5], [1.5, 0.5, 0.9]]])), ut, 1.0, (0.0, 0.0, 0.0))
    # a planar patch: every quadric has rank 1, the regularisation decides the two in-plane coordinates
    out["planar"] = _case(*sheet_arrays(20, seed=103, flat=0.375), 1.0, (0.0, 0.0, 0.0))
    return out


NAMES = tuple(sorted(cases()))


def segment_sums(terms, start):
    """sum_order.segment_sum over every segment of a table -> (K, ...)"""
    return np.stack([SO.segment_sum(terms, int(start[k]), int(start[k + 1])) for k in range(len(start) - 1)]) if len(start) > 1 \
        else np.zeros((0,) + terms.shape[1:])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The numpy forms on a case, computed once -> dict.  means / quadrics: the plain in-order sums; device_means /
    device_quadrics: the same terms in the device's segment order (tests/sum_order.py)."""
    case = cases()[name]
    v, t, cell, origin = case["vertices"], case["triangles"], case["cell"], case["origin"]
    cl = MS.cluster_numpy(v, cell, origin)
    K = cl.num_clusters
    key, terms = MS.corner_terms_numpy(v, t, cl)
    order = np.argsort(key, kind="stable")
    corner_start = np.searchsorted(key[order], np.arange(K + 1)).astype(np.int64)
    vterms = v[cl.order].astype(np.float64)
    with np.errstate(all="ignore"):
        dmeans = segment_sums(vterms, cl.cluster_start) / cl.counts.astype(np.float64)[:, None] if K else np.zeros((0, 3))
    triples, alive = MS.triples_numpy(t, cl.vertex_cluster)
    return {"case": case, "clusters": cl, "means": MS.cluster_means_numpy(v, cl), "quadrics": MS.cluster_quadrics_numpy(v, t, cl),
            "device_means": dmeans, "device_quadrics": segment_sums(terms[order], corner_start),
            "corner_counts": np.diff(corner_start), "triples": triples, "alive": alive,
            "results": {}}


def result(name, **kw):
    """simplify_numpy on a case with the given settings, computed once per setting"""
    ref = reference(name)
    k = tuple(sorted(kw.items()))
    if k not in ref["results"]:
        case = ref["case"]
        ref["results"][k] = MS.simplify_numpy(case["vertices"], case["triangles"], case["cell"], origin=case["origin"], **kw)
    return ref["results"][k]


def sphere_error(vertices):
    """The mean of | |v - centre| - r | over the vertices"""
    return float(np.abs(np.linalg.norm(np.asarray(vertices, dtype=np.float64) - SPHERE_CENTRE, axis=1) - SPHERE_RADIUS).mean())
