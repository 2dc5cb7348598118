"""Mesh simplification: vertex clustering on a uniform grid with quadric-error placement (Lindstrom 2000).  It is the "make this
mesh smaller" step of the reconstruction chain (depth maps -> DepthFusion -> TSDFVolume -> Mesh -> clean-up -> simplify): marching
tetrahedra leaves several almost coplanar triangles per occupied voxel, and every consumer (mesh_nearest, mesh_render, write_ply)
pays for them.  The reference has no such component; the definition is this docstring, the *_numpy functions (the readable
specification and the CPU path) and include/mvd.h.  No step uses an atomic: two runs give the same bits.

Inputs.  vertices (M,3) float32, triangles (T,3) integers in 0 .. M-1 (int32 on a GPU).  cell is taken as float32 and
c = float64(float32(cell)).  Every float64 step below is one IEEE operation per written operation, in the written association, with
no contraction.

  1. Keys.  A vertex's key is cloud_eval.voxel_keys_numpy(vertices, cell, origin)'s: per axis idx = floor((float64(x) - origin) *
     (1 / c)), key = idx_x << 42 | idx_y << 21 | idx_z (csrc/cloud_grid.h: cell_index, cell_key).  origin defaults to the per-axis
     minimum over the finite vertices; ValueError when an index leaves [0, 2^21 - 1).  A vertex with a non-finite coordinate is
     INVALID: key INT64_MAX, no cluster; every triangle that names it is dropped and contributes nothing.
  2. Clusters.  The occupied cells in ascending key order are the clusters 0 .. K-1.  vertex_cluster (M) int32, -1 for an invalid
     vertex.  A cluster's vertices are taken in ascending vertex index (the order of a stable sort of the keys).  The centre of
     cluster k, per axis: ctr = (idx + 0.5) * c + origin.
  3. Means.  Per cluster the float64 sum of its vertices' coordinates in that order, divided by their number: mean (K,3) float64.
     Every per-vertex attribute (mesh.colors, attributes=) likewise, then rounded to float32.
  4. Quadrics.  Corner (t, j) of a triangle with three valid vertices belongs to the cluster of triangles[t][j].  p0, p1, p2 are
     float64 from float32; e1 = p1 - p0, e2 = p2 - p0; n = mesh_clean.cross_numpy's (e1y e2z - e1z e2y, e1z e2x - e1x e2z,
     e1x e2y - e1y e2x); q = p0 - ctr(cluster); d = -((nx qx + ny qy) + nz qz).  The corner's ten terms, in this order:
         nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, nx d, ny d, nz d, d d
     = (a00, a01, a02, a11, a12, a22, b0, b1, b2, cc): the squared distance to the triangle's plane, weighted by its squared area
     (Lindstrom's weighting: no square root is taken), as x^T A x + 2 b.x + cc in coordinates relative to the cell centre.  A
     triangle with two corners in one cluster contributes once per corner.  quadric[k] (K,10) float64 is the sum of the cluster's
     corners in ascending (t, j) order.  (The device adds a segment of more than 64 items, vertices in step 3 or corners here, as
     csrc/fixed_sums.h's segment walk does: lane l the items l, l + 64, ... in order, then the xor tree over the 64 lanes;
     tests/sum_order.segment_sum is that order in numpy.  The same value within the rounding of n float64 additions, the same
     bits in every run.)
  5. Placement.  placement="quadric" (the default): lam = regularisation * ((a00 + a11) + a22), regularisation float64 (default
     1e-3); A' = A + lam I, that is a00' = a00 + lam, a11' = a11 + lam, a22' = a22 + lam; r_i = -b_i + lam * (mean_i - ctr_i);
     x = adj(A') r / det(A') with the six cofactors of the symmetric matrix
         C00 = a11' a22' - a12 a12      C01 = a02 a12 - a01 a22'      C02 = a01 a12 - a02 a11'
         C11 = a00' a22' - a02 a02      C12 = a01 a02 - a00' a12      C22 = a00' a11' - a01 a01
     (each a difference of two products), det = (a00' C00 + a01 C01) + a02 C02 and
         x0 = ((C00 r0 + C01 r1) + C02 r2) / det,  x1 = ((C01 r0 + C11 r1) + C12 r2) / det,  x2 = ((C02 r0 + C12 r1) + C22 r2) / det.
     The vertex is float32(ctr + x) with placed = 1 when lam > 0, det is finite and > 0, every x_i is finite and |x_i| <= 0.5 * c for
     every i (the point stays in its own cell); otherwise it is float32(mean) with placed = 0.  A cluster of exactly one vertex
     keeps that vertex bit for bit (placed = 2).  placement="mean" gives every cluster placed = 0, or 2 for a single-vertex cluster:
     plain vertex clustering, as Open3D's Average.
  6. Triangles.  A triangle survives when its three vertices are valid and its three clusters are pairwise different.  It becomes
     its cluster triple, rotated so that the smallest index comes first (a rotation keeps the orientation); a triangle that does
     not survive has the triple (-1,-1,-1).  With unique=True (the default) survivors whose rotated triples are equal are
     duplicates: the one with the lowest original index stays.  The opposite orientation is another triple and stays.  Kept
     triangles keep their original order; kept_triangles holds their old indices.
  7. Unreferenced clusters.  With remove_unreferenced=True (the default) clusters that no kept triangle names are dropped and the
     triangles are re-indexed: mesh_clean's filter with no component verdict.  vertex_map (M) int32 is the final index of each input
     vertex's cluster, or -1.
  8. mesh.colors follow as means (step 3).  mesh.normals, if the input had them, are recomputed with mesh_clean.vertex_normals on
     the result: a mean of normals is not a normal.

Two implementations: the numpy forms on the host and the HIP kernels of csrc/mesh_simplify.hip (ops.mesh_cluster_*) for a mesh on a
GPU, with the stable sorts (vertices by key, corners by cluster, the triples for the duplicates) through torch.  The public
functions pick by where the arrays live.

Not here: edge-collapse decimation, a target triangle count, manifold guarantees (vertex clustering gives none: a thin
wall inside one cell collapses), and a fused quadric + placement kernel.
"""
from dataclasses import dataclass

import numpy as np

from .cloud_eval import voxel_keys_numpy
from .mesh import Mesh, check_mesh, int32_triangles, is_mesh, one_place, split_mesh, to_numpy
from .mesh_clean import clean_numpy, cross_numpy, vertex_normals

INVALID_KEY = np.iinfo(np.int64).max
_MASK = (1 << 21) - 1
PLACEMENTS = ("quadric", "mean")


@dataclass
class Clusters:
    """cluster_numpy's result.  vertex_cluster (M) int32; cluster_start (K+1) int32 into order; cluster_key (K) int64; order: the
    valid vertices sorted stably by key (int64); origin (3) float64; c: float64(float32(cell))."""
    vertex_cluster: object
    cluster_start: object
    cluster_key: object
    order: object
    origin: object
    c: float

    @property
    def num_clusters(self):
        return int(self.cluster_key.shape[0])

    @property
    def counts(self):
        return np.diff(self.cluster_start).astype(np.int32)

    @property
    def centres(self):
        return centres_numpy(self.cluster_key, self.origin, self.c)


@dataclass
class SimplifyResult:
    """simplify_mesh's full result: the new mesh, the per-vertex attributes' means (same container as handed in), vertex_map (M)
    int32 (the new index of each input vertex's cluster, or -1), kept_triangles (T') int32 (old indices), placed (M') uint8 (0: the
    mean, 1: the quadric's minimum, 2: a single vertex kept as it is) and cluster_counts (M') int32 (the input vertices behind each
    output vertex)."""
    mesh: object
    attributes: object
    vertex_map: object
    kept_triangles: object
    placed: object
    cluster_counts: object


# ---- argument checks -----------------------------------------------------------------------------------------------------------------
def _check_cell(cell):
    c = np.float32(cell)
    if not (np.isfinite(c) and c > 0):
        raise ValueError(f"cell must be finite and > 0, got {cell}")
    return c


def _check_settings(placement, regularisation):
    if placement not in PLACEMENTS:
        raise ValueError(f"placement must be one of {PLACEMENTS}, got {placement!r}")
    reg = float(regularisation)
    if not (np.isfinite(reg) and reg > 0):
        raise ValueError(f"regularisation must be finite and > 0, got {regularisation}")
    return reg


# ---- the numpy forms ------------------------------------------------------------------------------------------------------------------
def centres_numpy(cluster_key, origin, c):
    """Step 2's cell centres (K,3) float64 from the keys."""
    k = np.asarray(cluster_key, dtype=np.int64)
    idx = np.stack([k >> 42, (k >> 21) & _MASK, k & _MASK], axis=1).astype(np.float64)
    return (idx + 0.5) * np.float64(c) + np.asarray(origin, dtype=np.float64)


def cluster_numpy(vertices, cell, origin=None):
    """Steps 1 and 2 -> Clusters."""
    c32 = _check_cell(cell)
    keys, origin = voxel_keys_numpy(vertices, c32, origin)
    M = len(keys)
    order = np.argsort(keys, kind="stable")[:int((keys != INVALID_KEY).sum())]
    sk = keys[order]
    heads = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]])) if len(sk) else np.zeros(0, dtype=np.int64)
    start = np.concatenate([heads, [len(sk)]]).astype(np.int32)
    vc = np.full(M, -1, dtype=np.int32)
    vc[order] = np.repeat(np.arange(len(heads), dtype=np.int32), np.diff(start))
    return Clusters(vc, start, sk[heads], order.astype(np.int64), origin, float(np.float64(c32)))


def cluster_means_numpy(rows, clusters):
    """Step 3 -> (K,k) float64: the means of a per-vertex (M,k) float32 array, every sum in ascending vertex index."""
    r = np.asarray(to_numpy(rows), dtype=np.float32)[clusters.order].astype(np.float64)
    lab, K = clusters.vertex_cluster[clusters.order], clusters.num_clusters
    if K == 0:
        return np.zeros((0, r.shape[1]))
    # bincount adds its weights one after the other in the order of the list
    sums = np.stack([np.bincount(lab, weights=r[:, j], minlength=K) for j in range(r.shape[1])], axis=1)
    with np.errstate(all="ignore"):
        return sums / clusters.counts.astype(np.float64)[:, None]


def corner_terms_numpy(vertices, triangles, clusters):
    """Step 4's terms -> (corner_cluster (3T) int32, terms (3T,10) float64) in (t, j) order; a corner of a dropped triangle has the
    cluster K (the sentinel the device sorts last) and its terms are not to be read."""
    v = np.asarray(to_numpy(vertices), dtype=np.float32)
    tri = np.asarray(to_numpy(triangles)).astype(np.int64).reshape(-1, 3)
    K = clusters.num_clusters
    tc = clusters.vertex_cluster[tri]
    valid = (tc >= 0).all(axis=1)
    key = np.where(valid[:, None], tc, K).astype(np.int32)
    n = cross_numpy(v, tri)
    p0 = v.astype(np.float64)[tri[:, 0]]
    ctr = np.concatenate([clusters.centres, np.zeros((1, 3))])
    terms = np.zeros((len(tri), 3, 10))
    with np.errstate(all="ignore"):
        for j in range(3):
            q = p0 - ctr[key[:, j]]
            d = -((n[:, 0] * q[:, 0] + n[:, 1] * q[:, 1]) + n[:, 2] * q[:, 2])
            terms[:, j] = np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2],
                                    n[:, 2] * n[:, 2], n[:, 0] * d, n[:, 1] * d, n[:, 2] * d, d * d], axis=1)
    return key.reshape(-1), terms.reshape(-1, 10)


def cluster_quadrics_numpy(vertices, triangles, clusters):
    """Step 4 -> (K,10) float64, every sum in ascending (t, j)."""
    key, terms = corner_terms_numpy(vertices, triangles, clusters)
    K = clusters.num_clusters
    ok = key < K
    if K == 0:
        return np.zeros((0, 10))
    return np.stack([np.bincount(key[ok], weights=terms[ok, j], minlength=K) for j in range(10)], axis=1)


def place_numpy(vertices, triangles, clusters, placement="quadric", regularisation=1e-3, quadrics=None, means=None, details=False):
    """Step 5 -> (vertices (K,3) float32, placed (K) uint8).  quadrics (K,10) and means (K,3) float64 replace the ones formed here
    (the tests hand in the device's).  details=True -> also a dict of lam, det (K) and x (K,3) float64 as the quadric branch formed
    them (placement="mean": None)."""
    reg = _check_settings(placement, regularisation)
    v = np.asarray(to_numpy(vertices), dtype=np.float32)
    K, c = clusters.num_clusters, np.float64(clusters.c)
    mean = cluster_means_numpy(v, clusters) if means is None else np.asarray(means, dtype=np.float64).reshape(K, 3)
    out = mean.astype(np.float32)
    placed = np.zeros(K, dtype=np.uint8)
    extra = None
    if placement == "quadric" and K:
        Q = cluster_quadrics_numpy(v, triangles, clusters) if quadrics is None else np.asarray(quadrics, dtype=np.float64).reshape(K, 10)
        a00, a01, a02, a11, a12, a22 = (Q[:, j] for j in range(6))
        ctr = clusters.centres
        with np.errstate(all="ignore"):
            lam = np.float64(reg) * ((a00 + a11) + a22)
            d00, d11, d22 = a00 + lam, a11 + lam, a22 + lam
            r = -Q[:, 6:9] + lam[:, None] * (mean - ctr)
            C00, C01, C02 = d11 * d22 - a12 * a12, a02 * a12 - a01 * d22, a01 * a12 - a02 * d11
            C11, C12, C22 = d00 * d22 - a02 * a02, a01 * a02 - d00 * a12, d00 * d11 - a01 * a01
            det = (d00 * C00 + a01 * C01) + a02 * C02
            x = np.stack([((C00 * r[:, 0] + C01 * r[:, 1]) + C02 * r[:, 2]) / det, ((C01 * r[:, 0] + C11 * r[:, 1]) + C12 * r[:, 2]) / det,
                          ((C02 * r[:, 0] + C12 * r[:, 1]) + C22 * r[:, 2]) / det], axis=1)
            good = (lam > 0) & np.isfinite(det) & (det > 0) & np.isfinite(x).all(axis=1) & (np.abs(x) <= 0.5 * c).all(axis=1)
            out = np.where(good[:, None], (ctr + x).astype(np.float32), out)
        placed[good] = 1
        extra = {"lam": lam, "det": det, "x": x}
    single = clusters.counts == 1
    out[single] = v[clusters.order[clusters.cluster_start[:-1][single]]]
    placed[single] = 2
    return (out, placed, extra) if details else (out, placed)


def triples_numpy(triangles, vertex_cluster):
    """Step 6's first half -> (triples (T,3) int32, alive (T) bool)."""
    tri = np.asarray(to_numpy(triangles)).astype(np.int64).reshape(-1, 3)
    tc = np.asarray(vertex_cluster)[tri]
    alive = (tc >= 0).all(axis=1) & (tc[:, 0] != tc[:, 1]) & (tc[:, 1] != tc[:, 2]) & (tc[:, 0] != tc[:, 2])
    first = np.argmin(tc, axis=1) if len(tc) else np.zeros(0, dtype=np.int64)
    rot = np.take_along_axis(tc, (first[:, None] + np.arange(3)) % 3, axis=1)
    return np.where(alive[:, None], rot, -1).astype(np.int32), alive


def kept_numpy(triples, alive, unique=True):
    """Step 6's second half -> kept_triangles (T') int32 ascending."""
    idx = np.flatnonzero(alive)
    if unique and len(idx):
        _, first = np.unique(triples[idx], axis=0, return_index=True)  # the first occurrence of every distinct triple
        idx = idx[np.sort(first)]
    return idx.astype(np.int32)


def simplify_numpy(vertices, triangles, cell, placement="quadric", regularisation=1e-3, origin=None, unique=True,
                   remove_unreferenced=True, attributes=(), quadrics=None, means=None):
    """Steps 1 to 7 -> SimplifyResult of numpy arrays (mesh: a Mesh without colours or normals; attributes: the list of the
    attributes' means (M',k) float32).  quadrics / means: place_numpy's overrides."""
    vertices, tri = np.asarray(to_numpy(vertices)), np.asarray(to_numpy(triangles))
    attributes = [np.asarray(to_numpy(a)) for a in attributes]
    check_mesh(vertices, tri, tuple((f"attributes[{i}]", a) for i, a in enumerate(attributes)))
    _check_settings(placement, regularisation)
    clusters = cluster_numpy(vertices, cell, origin)
    pos, placed = place_numpy(vertices, tri, clusters, placement, regularisation, quadrics, means)
    with np.errstate(all="ignore"):
        attrs = [cluster_means_numpy(a, clusters).astype(np.float32) for a in attributes]
    triples, alive = triples_numpy(tri, clusters.vertex_cluster)
    kept = kept_numpy(triples, alive, unique)
    v, t, attrs, remap, _ = clean_numpy(pos, triples[kept].reshape(-1, 3), remove_unreferenced=remove_unreferenced, attributes=attrs)
    vc = clusters.vertex_cluster
    vertex_map = np.where(vc >= 0, remap[np.maximum(vc, 0)] if len(remap) else -1, -1).astype(np.int32)
    keep_v = remap >= 0
    return SimplifyResult(Mesh(v, t.astype(np.int32)), attrs, vertex_map, kept, placed[keep_v], clusters.counts[keep_v])


# ---- the device path ---------------------------------------------------------------------------------------------------------------------
def _simplify_device(vertices, tri, cell, placement, reg, origin, unique, remove_unreferenced, rows):
    """The kernels of csrc/mesh_simplify.hip between torch's stable sorts.  Host reads: the extent (the default origin and the index
    check, 6 floats), K, and the filter's two counts."""
    import torch
    from . import ops
    cl = ops.mesh_cluster_ids(vertices, cell, origin)
    K = cl.num_clusters
    means = ops.mesh_cluster_means(vertices, cl)
    triples, alive, corner_key = ops.mesh_cluster_triples(tri, cl)
    quadrics = None
    if placement == "quadric":
        key, perm = torch.sort(corner_key.reshape(-1), stable=True)
        quadrics = ops.mesh_cluster_quadrics(vertices, tri, key, perm, cl)
    pos, placed = ops.mesh_cluster_place(vertices, cl, means, quadrics, reg)
    attrs = [ops.mesh_cluster_means(a, cl).to(torch.float32) for a in rows]
    keep = alive
    if unique and tri.shape[0]:
        # lexicographic by two stable sorts: the third index first, then the 64-bit pair of the first two (dead triples last)
        p1 = torch.sort(triples[:, 2], stable=True)[1]
        pair = (triples[:, 0].to(torch.int64) << 32) | triples[:, 1].to(torch.int64)
        pair = torch.where(alive.bool(), pair, torch.full_like(pair, INVALID_KEY))
        p2 = torch.sort(pair[p1], stable=True)[1]
        keep = ops.mesh_cluster_mark_first(triples, alive, p1[p2])
    T, dev = int(tri.shape[0]), tri.device
    if K:
        # mesh_clean's filter: every triangle its own "component", the verdicts are the keep bytes
        own = torch.arange(T, dtype=torch.int32, device=dev)
        t, kept, remap, Mk = ops.mesh_filter(triples, K, own, keep, remove_unreferenced)
    else:  # no valid vertex: nothing to filter
        t, kept, Mk = torch.empty((0, 3), dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev), 0
        remap = torch.empty(0, dtype=torch.int32, device=dev)
    v = ops.mesh_gather_rows(pos, remap, Mk)
    attrs = [ops.mesh_gather_rows(a.contiguous(), remap, Mk) for a in attrs]
    vc = cl.vertex_cluster
    vertex_map = torch.where(vc >= 0, remap[vc.clamp(min=0).long()], torch.full_like(vc, -1)) if K else torch.full_like(vc, -1)
    keep_v = remap >= 0
    return v, t, attrs, vertex_map, kept, placed[keep_v], cl.counts[keep_v], {"clusters": cl, "means": means, "quadrics": quadrics,
                                                                                "triples": triples, "alive": alive}


# ---- public --------------------------------------------------------------------------------------------------------------------------
def simplify_mesh(mesh, cell, placement="quadric", regularisation=1e-3, origin=None, unique=True, remove_unreferenced=True,
                  attributes=None, details=False):
    """-> a new Mesh with one vertex per occupied cell of edge `cell` (module docstring); its colors are the clusters' means, its
    normals (if the input had them) are recomputed.  mesh: a Mesh or a pair (vertices, triangles).  attributes: per-vertex (M,k)
    float32 arrays, a list or a dict of them.  With attributes or details=True the result is a SimplifyResult.  Arrays on the host
    run simplify_numpy; GPU tensors run the kernels and give GPU tensors."""
    if not is_mesh(mesh):
        mesh = Mesh(*split_mesh(mesh)[:2])
    cell = float(_check_cell(cell))
    reg = _check_settings(placement, regularisation)
    names = list(attributes) if isinstance(attributes, dict) else None
    given = [] if attributes is None else list(attributes.values() if names is not None else attributes)
    colors, had_normals = getattr(mesh, "colors", None), getattr(mesh, "normals", None) is not None
    rows = ([colors] if colors is not None else []) + given
    labels = (["mesh.colors"] if colors is not None else []) + [f"attributes[{i if names is None else repr(names[i])}]" for i in range(len(given))]
    extra = tuple(zip(labels, rows)) + ((("mesh.normals", mesh.normals),) if had_normals else ())
    place = one_place(mesh.vertices, mesh.triangles, *(a for _, a in extra), what="mesh arrays")
    check_mesh(mesh.vertices, mesh.triangles, extra)
    if place == "host":
        r = simplify_numpy(mesh.vertices, mesh.triangles, cell, placement, reg, origin, unique, remove_unreferenced, rows)
        new, out, vertex_map, kept, placed, counts = r.mesh, list(r.attributes), r.vertex_map, r.kept_triangles, r.placed, r.cluster_counts
    else:
        v, t, out, vertex_map, kept, placed, counts, _ = _simplify_device(mesh.vertices.contiguous(), int32_triangles(mesh.triangles), cell,
                                                                           placement, reg, origin, unique, remove_unreferenced,
                                                                           [a.contiguous() for a in rows])
        new = Mesh(v, t)
    if colors is not None:
        new.colors = out.pop(0)
    if had_normals:
        new.normals = vertex_normals(new)
    if attributes is None and not details:
        return new
    attrs = None if attributes is None else (dict(zip(names, out)) if names is not None else out)
    return SimplifyResult(new, attrs, vertex_map, kept, placed, counts)
