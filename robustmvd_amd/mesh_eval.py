"""Mesh evaluation: score a reconstructed triangle mesh (TSDFVolume.extract_mesh, Mesh.clean) against a ground-truth scan, a scan
against a mesh, or two meshes: DTU's accuracy / completeness and Tanks and Temples' precision / recall / F-score for a SURFACE.  The
reference has no such component (it stops at the per-view depth map); the definition is this docstring, the numpy functions below
(the readable specification and the CPU path) and include/mvd.h.

Vertices (M,3) are float32, triangles (T,3) int32; max_dist and spacing are taken as float32, the grid's cell as the double it is
given as (cloud_grid's convention).  A triangle is INVALID if an index is outside [0, M) or a vertex has a non-finite coordinate: it
matches no query and gets no sample.  A degenerate but finite triangle (zero area) is valid and acts as its segment or point.

1. Point-to-triangle distance.  For a query q and a triangle A, B, C everything is taken relative to the query first (as
   cloud_eval.nearest_numpy uses coordinate differences: the values must survive coordinates of 10^3); the edges come from the
   vertices, so they do not depend on the query:
       a = A - q, b = B - q, c = C - q;   E0 = B - A, E1 = C - B, E2 = A - C;   dot(u,v) = (u.x v.x + u.y v.y) + u.z v.z
       seg(p, E): ee = dot(E,E); t = clamp(-dot(p,E) / ee, 0, 1), t = 0 when ee == 0; r = p + t E; the result is dot(r,r)
       d2 = min(seg(a,E0), seg(b,E1), seg(c,E2));   n = E0 x E1, nn = dot(n,n)
       inside iff nn > 0 and dot(n, a x E0) >= 0 and dot(n, b x E1) >= 0 and dot(n, c x E2) >= 0
       inside: d2 = min(d2, dot(n,a)^2 / nn);   dist(q, triangle) = sqrt(d2)
   No region case analysis, and no division that a degenerate triangle can poison.
   Truncated nearest triangle (mesh_distance_numpy), as cloud_eval's definition 1:
       dist[i]  = min(max_dist, min over valid triangles)    (max_dist for an invalid query, T = 0 or no valid triangle)
       index[i] = the triangle of that minimum when it is < max_dist (strict), else -1
   Among triangles with an equal d2, as the device computed it, the smallest triangle index wins.  No atomic decides a value: two
   calls give the same bits.

2. The triangle grid.  Cells, keys and inv are the cloud grid's (cloud_eval.py, definition 3): i_a = floor((float64(x_a) - o_a) * inv),
   21 bits per axis, inv = 1.0 / cell formed on the host as a double.  A valid triangle is entered into every cell of its axis-aligned
   box, per axis floor((float64(min_a) - o_a) * inv) .. floor((float64(max_a) - o_a) * inv), no dilation.  The pair list (key,
   triangle) is emitted in triangle order, inside a triangle x-major, then y, then z, and then sorted STABLY by key: a pure function
   of the inputs (mesh_grid_pairs_numpy).  With cell >= max_dist (1 + 2^-10) the 27 cells around a query's hold every triangle
   within max_dist: the triangle's point nearest to the query lies in a cell of the triangle's box, and that cell is within one of
   the query's on every axis (csrc/mesh_eval.hip has the argument).  A triangle in several scanned cells is seen several times, which
   is harmless under min.  More than max_pairs pairs raise ValueError; the remedy is a larger cell.

3. Surface sampling (sample_mesh_numpy).  For a spacing s > 0 a triangle with longest squared edge L2 (float64 differences of the
   float32 coordinates, (dx^2 + dy^2) + dz^2) gets k = max(1, ceil(sqrt(L2) / s)), formed independently of how sqrt rounds:
   r = L2 * inv_s2 with inv_s2 = 1.0 / (float64(s) * float64(s)), and k is the smallest integer >= 1 with k k >= r (capped at 2^26).
   The samples are the centroids of the k^2 congruent sub-triangles.  Rows i = 0 .. k-1; row i holds 2 (k - i) - 1 samples; position
   t in the row gives j = t >> 1 and down = t & 1, and the weights
       on B (3 i + 1 + down) / (3 k),   on C (3 j + 1 + down) / (3 k),   on A (3 (k - i - j) - 2 - 2 down) / (3 k),
   each one double division of two exactly representable integers; the point is (wA A + wB B) + wC C in double, rounded once to
   float32, and per-vertex attributes (M,c) go through the same expression: numpy and the device produce the same bits.  Output, in
   triangle order then sample order: points (S,3), triangle (S) int32, attributes; S = sum of k^2 exactly.  Every surface point lies
   within 2 s / 3 of a sample (a sub-triangle's longest edge is <= s).  This is a COVERING sampler, not an area-uniform one: a mesh
   of triangles below the spacing gets one sample per triangle.  Density is equalised afterwards by cloud_eval's voxel
   down-sampling (MeshEvaluation(voxel=...)), as PointCloudEvaluation does for predictions.

4. Scores (MeshEvaluation).  Each side is a cloud (n,3), a Mesh or (vertices, triangles); at least one side is a mesh.  A mesh side
   ANSWERS queries through definition 1 and ASKS them through its samples at `spacing` (default: the smallest threshold), thinned by
   `voxel` when given; a cloud side answers through cloud_eval's nearest neighbour and asks with its points.  The sums and their
   combination are cloud_eval's definition 2, and the result is its CloudScore.
"""
import numpy as np

from .cloud_eval import (INDEX_LIMIT, CloudScore, check_thresholds, combine_scores, host_points, nearest_numpy,  # noqa: F401
                         voxel_downsample_numpy)
from .mesh import check_mesh, one_place, place, split_mesh, to_numpy

MAX_PAIRS = 1 << 28
MAX_SAMPLES = 1 << 28
HARD_LIMIT = 2 ** 31 - 1
K_CAP = 1 << 26


def _mesh_numpy(vertices, triangles):
    """The numpy forms' mesh: vertices converted to float32, an empty triangle array of any shape taken as (0,3), and no index
    range: a triangle with an index outside 0 .. M-1 is invalid (valid_triangles_numpy), not an error."""
    v = np.asarray(to_numpy(vertices), dtype=np.float32)
    t = np.asarray(to_numpy(triangles))
    if t.size == 0:
        t = t.reshape(-1, 3)
    check_mesh(v, t, index_range=False)
    return v, t.astype(np.int64)


def valid_triangles_numpy(vertices, triangles):
    """-> (T,) bool: every index in [0, M) and every coordinate of the three vertices finite."""
    v, t = _mesh_numpy(vertices, triangles)
    ok = ((t >= 0) & (t < len(v))).all(axis=1)
    finite = np.isfinite(v).all(axis=1)
    ok[ok] = finite[t[ok]].all(axis=1)
    return ok


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _seg(p, E):
    ft = p.dtype.type
    ee = _dot(E, E)
    zero = ee == 0
    t = np.where(zero, ft(0), np.clip(-_dot(p, E) / np.where(zero, ft(1), ee), ft(0), ft(1)))
    r = p + t[..., None] * E
    return _dot(r, r)


def triangle_d2_numpy(q, A, B, C):
    """Definition 1's d2 for arrays that broadcast against each other (..., 3), all of one float dtype: the chain runs in that dtype."""
    a, b, c = A - q, B - q, C - q
    E0, E1, E2 = B - A, C - B, A - C
    d2 = np.minimum(_seg(a, E0), np.minimum(_seg(b, E1), _seg(c, E2)))
    n = _cross(E0, E1)
    nn = _dot(n, n)
    ft = d2.dtype.type
    inside = (nn > 0) & (_dot(n, _cross(a, E0)) >= 0) & (_dot(n, _cross(b, E1)) >= 0) & (_dot(n, _cross(c, E2)) >= 0)
    na = _dot(n, a)
    plane = na * na / np.where(nn > 0, nn, ft(1))
    return np.where(inside, np.minimum(d2, plane), d2)


def triangle_distance_numpy(query, vertices, triangles, index, dtype=np.float64):
    """dist(query[i], triangle index[i]) per query -> (n,) of dtype: what a returned index is worth."""
    ft = np.dtype(dtype).type
    v, t = _mesh_numpy(vertices, triangles)
    q = host_points(query, "query").astype(ft)
    tri = t[np.asarray(index, dtype=np.int64)]
    with np.errstate(all="ignore"):
        return np.sqrt(triangle_d2_numpy(q, v[tri[:, 0]].astype(ft), v[tri[:, 1]].astype(ft), v[tri[:, 2]].astype(ft)))


def mesh_distance_numpy(query, vertices, triangles, max_dist, dtype=np.float64):
    """Definition 1 as chunked brute force -> (dist (n,) of dtype, index (n,) int32).  dtype=np.float32 evaluates the same chain in
    float32: the gap between the two is what tests/mesh_eval_cases.py derives its band from.  max_dist=np.inf gives the untruncated
    distance (inf without a valid triangle)."""
    ft = np.dtype(dtype).type
    v, t = _mesh_numpy(vertices, triangles)
    q = host_points(query, "query").astype(ft)
    md = ft(np.float32(max_dist))
    if not md > 0:
        raise ValueError(f"max_dist must be > 0, got {max_dist}")
    n = len(q)
    dist, index = np.full(n, md, dtype=ft), np.full(n, -1, dtype=np.int32)
    ok = valid_triangles_numpy(v, t)
    which = np.flatnonzero(ok)  # ascending: the first minimum is the smallest triangle index
    if n == 0 or len(which) == 0:
        return dist, index
    A, B, C = (v[t[which, k]].astype(ft)[None] for k in range(3))
    q_ok = np.isfinite(q).all(axis=1)
    step = max(1, (1 << 19) // len(which))
    with np.errstate(all="ignore"):
        for b in range(0, n, step):
            d2 = triangle_d2_numpy(np.where(q_ok[b:b + step, None], q[b:b + step], ft(0))[:, None, :], A, B, C)
            j = np.argmin(d2, axis=1)
            dm = np.sqrt(d2[np.arange(len(j)), j])
            found = (dm < md) & q_ok[b:b + step]
            dist[b:b + step] = np.where(found, dm, md)
            index[b:b + step] = np.where(found, which[j], -1)
    return dist, index


def mesh_grid_pairs_numpy(vertices, triangles, origin, cell):
    """Definition 2's pair list -> (keys (P,) int64 ascending, triangle (P,) int32): the (cell, triangle) pairs in the order a stable
    sort by key leaves them.  ValueError when a cell index of a valid triangle leaves [0, 2^21 - 1)."""
    v, t = _mesh_numpy(vertices, triangles)
    origin = np.asarray(origin, dtype=np.float64).reshape(-1)
    cell = float(cell)
    if origin.shape != (3,) or not np.isfinite(origin).all() or not 0 < cell < np.inf:
        raise ValueError(f"origin must be 3 finite numbers and cell finite and > 0, got {origin.tolist()} and {cell}")
    inv = 1.0 / np.float64(cell)
    which = np.flatnonzero(valid_triangles_numpy(v, t))
    if len(which) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int32)
    corners = v[t[which]]  # (T',3 vertices,3 axes) float32
    lo = np.floor((corners.min(axis=1).astype(np.float64) - origin) * inv)
    hi = np.floor((corners.max(axis=1).astype(np.float64) - origin) * inv)
    if lo.min() < 0 or hi.max() >= INDEX_LIMIT:
        raise ValueError(f"mesh_grid: at an edge of {cell:g} from origin {origin.tolist()} the triangles' cell indices span "
                         f"{lo.min():.0f} .. {hi.max():.0f}; each must be in [0, {INDEX_LIMIT})")
    lo, size = lo.astype(np.int64), (hi - lo).astype(np.int64) + 1
    counts = size.prod(axis=1)
    if counts.astype(np.float64).sum() > HARD_LIMIT:
        raise ValueError(f"mesh_grid: about {counts.astype(np.float64).sum():.3g} pairs, above 2^31 - 1; use a larger cell")
    owner = np.repeat(np.arange(len(which)), counts)
    rank = np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts)
    ny, nz = size[owner, 1], size[owner, 2]
    ix, iy, iz = lo[owner, 0] + rank // (nz * ny), lo[owner, 1] + (rank // nz) % ny, lo[owner, 2] + rank % nz
    keys = (ix << 42) | (iy << 21) | iz
    order = np.argsort(keys, kind="stable")
    return keys[order], which[owner[order]].astype(np.int32)


def _ceil_sqrt(r):
    """The smallest integer k >= 1 with k k >= r, per element of the float64 array r, capped at 2^26: integer correction steps
    around sqrt, so that the result does not depend on how sqrt rounds (k k is an exact double below the cap)."""
    r = np.asarray(r, dtype=np.float64)
    big = ~(r < float(K_CAP) ** 2)
    with np.errstate(all="ignore"):
        k = np.maximum(np.sqrt(np.where(big, 1.0, r)).astype(np.int64), 1)
    for _ in range(4):
        k = k + (k.astype(np.float64) ** 2 < r)
    for _ in range(4):
        k = k - ((k > 1) & ((k - 1).astype(np.float64) ** 2 >= r))
    return np.where(big, K_CAP, k)


def sample_counts_numpy(vertices, triangles, spacing):
    """-> (k (T,) int64: definition 3's k per triangle, 0 for an invalid one; inv_s2)"""
    v, t = _mesh_numpy(vertices, triangles)
    s = np.float32(spacing)
    if not (s > 0 and np.isfinite(s)):
        raise ValueError(f"spacing must be finite and > 0, got {spacing}")
    inv_s2 = 1.0 / (np.float64(s) * np.float64(s))
    ok = valid_triangles_numpy(v, t)
    k = np.zeros(len(t), np.int64)
    if ok.any():
        P = v[t[ok]].astype(np.float64)
        e2 = lambda d: (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        L2 = np.maximum(e2(P[:, 1] - P[:, 0]), np.maximum(e2(P[:, 2] - P[:, 1]), e2(P[:, 0] - P[:, 2])))
        k[ok] = _ceil_sqrt(L2 * inv_s2)
    return k, inv_s2


def sample_mesh_numpy(vertices, triangles, spacing, attributes=None, max_samples=MAX_SAMPLES):
    """Definition 3 -> (points (S,3) float32, triangle (S,) int32, attributes (S,c) float32 or None)."""
    v, t = _mesh_numpy(vertices, triangles)
    attr = None
    if attributes is not None:
        attr = np.asarray(to_numpy(attributes), dtype=np.float32)
        if attr.ndim != 2 or attr.shape[0] != len(v) or attr.shape[1] < 1:
            raise ValueError(f"attributes must be ({len(v)},c), got {attr.shape}")
    max_samples = int(max_samples)
    if not 1 <= max_samples <= HARD_LIMIT:
        raise ValueError(f"max_samples must be in 1 .. 2^31 - 1, got {max_samples}")
    k, _ = sample_counts_numpy(v, t, spacing)
    total = sum(int(c) * int(c) for c in k[k > 1]) + int((k == 1).sum())  # Python integers: exact
    if total > max_samples:
        raise ValueError(f"mesh_sample: {total} samples at a spacing of {float(np.float32(spacing)):g}, above max_samples = {max_samples}; "
                         f"the largest triangle alone gets {int(k.max()) ** 2}.  Pass a larger spacing or raise max_samples")
    counts = k * k
    owner = np.repeat(np.arange(len(t)), counts)
    rank = np.arange(total) - np.repeat(np.cumsum(counts) - counts, counts)
    kk = k[owner]
    left = kk * kk - rank
    w = _ceil_sqrt(left)
    i, pos = kk - w, w * w - left
    j, down = pos >> 1, pos & 1
    k3 = (3 * kk).astype(np.float64)
    wb = (3 * i + 1 + down).astype(np.float64) / k3
    wc = (3 * j + 1 + down).astype(np.float64) / k3
    wa = (3 * (kk - i - j) - 2 - 2 * down).astype(np.float64) / k3
    tri = t[owner]
    mix = lambda x: ((wa[:, None] * x[tri[:, 0]].astype(np.float64) + wb[:, None] * x[tri[:, 1]].astype(np.float64))
                     + wc[:, None] * x[tri[:, 2]].astype(np.float64)).astype(np.float32)
    if total == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32), None if attr is None else np.zeros((0, attr.shape[1]), np.float32)
    return mix(v), owner.astype(np.int32), None if attr is None else mix(attr)


# ---- front ends: the host or the device, by where the inputs are -------------------------------------------------------------------

def _device_origin(ops, clouds):
    extents = [e for e in (ops.cloud_extent(c) for c in clouds) if e is not None]
    return np.min([e[0] for e in extents], axis=0).tolist() if extents else [0.0, 0.0, 0.0]


def mesh_distance(points, mesh, max_dist, max_pairs=MAX_PAIRS):
    """The truncated distance of every point to the mesh's surface (definition 1) -> (dist (n) float32, index (n) int32: the nearest
    triangle, or -1 where nothing is nearer than max_dist).  mesh: a Mesh or (vertices, triangles).  GPU tensors run the HIP
    kernels (ops.mesh_grid at a cell of max_dist (1 + 2^-10), ops.mesh_nearest), numpy arrays the numpy specification."""
    vertices, triangles, _ = split_mesh(mesh)
    if one_place(points, vertices, triangles) == "host":
        d, i = mesh_distance_numpy(points, vertices, triangles, max_dist)
        return d.astype(np.float32), i
    from . import ops
    md = float(np.float32(max_dist))
    v = ops.cloud_points(vertices, "vertices")
    grid = ops.mesh_grid(v, triangles, _device_origin(ops, [v]), md * ops.CLOUD_CELL_MARGIN, max_pairs=max_pairs)
    return ops.mesh_nearest(points, grid, md)


def sample_mesh(mesh, spacing, attributes=None, max_samples=MAX_SAMPLES):
    """Deterministic covering samples of the mesh's surface (definition 3) -> (points (S,3) float32, triangle (S) int32, attributes
    (S,c) or None); GPU tensors run the HIP kernels (ops.mesh_sample), numpy arrays the numpy specification: the same bits."""
    vertices, triangles, _ = split_mesh(mesh)
    if one_place(vertices, triangles, *([] if attributes is None else [attributes])) == "host":
        return sample_mesh_numpy(vertices, triangles, spacing, attributes, max_samples)
    from . import ops
    return ops.mesh_sample(vertices, triangles, spacing, attributes, max_samples=max_samples)


class MeshEvaluation:
    """Scores a surface against a scan, a scan against a surface, or two surfaces (module docstring, definition 4).

        evaluation = MeshEvaluation(thresholds=(0.005, 0.01))                       # or create_evaluation("mesh", ...)
        score = evaluation(volume.extract_mesh(), gt_points)                        # -> cloud_eval.CloudScore
        score.fscore, score.accuracy, score.completeness, score.dist_gt

    pred and gt are each a cloud (n,3), a Mesh or (vertices, triangles); at least one must be a mesh (two clouds:
    PointCloudEvaluation).  max_dist defaults to 4 x the largest threshold, spacing (of a mesh side's samples) to the smallest
    threshold.  The sampler COVERS the surface (every surface point within 2 spacing / 3 of a sample) but is not area-uniform: a
    region of triangles below the spacing gets one sample per triangle; voxel= thins the samples (and a predicted cloud) to one
    per voxel, as PointCloudEvaluation(voxel=) does.  Registration is out of scope here: align first with
    cloud_register.register_clouds on Mesh.sample(...) and apply the result to the vertices.
    The result's dist_pred / dist_gt belong to the asked points of each side; pred_points are those of the prediction (a mesh's
    samples).  Inputs on the GPU run the HIP kernels, inputs on the host the numpy specification; a mixed pair raises."""

    def __init__(self, thresholds, max_dist=None, spacing=None, voxel=None, max_pairs=MAX_PAIRS, max_samples=MAX_SAMPLES):
        self.thresholds, self.max_dist = check_thresholds(thresholds, max_dist)
        spacing = self.thresholds.min() if spacing is None else np.float32(spacing)
        for name, value in (("spacing", spacing), ("voxel", voxel)):
            if value is not None and not (np.float32(value) > 0 and np.isfinite(np.float32(value))):
                raise ValueError(f"{name} must be finite and > 0, got {value}")
        self.spacing = float(spacing)
        self.voxel = None if voxel is None else float(np.float32(voxel))
        self.max_pairs, self.max_samples = max_pairs, max_samples

    def __call__(self, pred, gt):
        sides = [split_mesh(pred, required=False), split_mesh(gt, required=False)]
        if sides[0] is None and sides[1] is None:
            raise ValueError("MeshEvaluation needs a mesh on at least one side; two clouds are PointCloudEvaluation's")
        arrays = [a for side, raw in zip(sides, (pred, gt)) for a in (side[:2] if side is not None else (raw,))]
        run = self._run_host if one_place(*arrays) == "host" else self._run_device
        return run(sides, pred, gt)

    def _run_host(self, sides, pred, gt):
        th, md = self.thresholds, self.max_dist
        asks, answers = [], []
        for k, (side, raw) in enumerate(zip(sides, (pred, gt))):
            if side is None:
                p = host_points(raw, ("pred", "gt")[k])
                if self.voxel is not None and k == 0:
                    p = voxel_downsample_numpy(p, self.voxel)[0]
                asks.append(p)
                answers.append(lambda q, p=p: nearest_numpy(q, p, md)[0])
            else:
                v, t = _mesh_numpy(side[0], side[1])
                p = sample_mesh_numpy(v, t, self.spacing, max_samples=self.max_samples)[0]
                if self.voxel is not None:
                    p = voxel_downsample_numpy(p, self.voxel)[0]
                asks.append(p)
                answers.append(lambda q, v=v, t=t: mesh_distance_numpy(q, v, t, md)[0])

        def direction(q, answer):
            d = answer(q)
            dv = d[np.isfinite(q).all(axis=1)]
            return d.astype(np.float32), float(np.sum(dv)), len(dv), np.array([(dv < np.float64(t)).sum() for t in th], dtype=np.int64)

        dp, sp, np_, cp = direction(asks[0], answers[1])
        dg, sg, ng, cg = direction(asks[1], answers[0])
        return combine_scores(sp, np_, cp, sg, ng, cg, dist_pred=dp, dist_gt=dg, thresholds=th, max_dist=float(md), pred_points=asks[0])

    def _run_device(self, sides, pred, gt):
        import torch
        from . import ops
        md, T = float(self.max_dist), len(self.thresholds)
        cell = md * ops.CLOUD_CELL_MARGIN
        asks, meshes = [], []
        for k, (side, raw) in enumerate(zip(sides, (pred, gt))):
            if side is None:
                p = ops.cloud_points(raw, ("pred", "gt")[k])
                if self.voxel is not None and k == 0:
                    p = ops.voxel_downsample(p, self.voxel)[0]
                meshes.append(None)
            else:
                v = ops.cloud_points(side[0], "vertices")
                p = ops.mesh_sample(v, side[1], self.spacing, max_samples=self.max_samples)[0]
                if self.voxel is not None:
                    p = ops.voxel_downsample(p, self.voxel)[0]
                meshes.append((v, side[1]))
            asks.append(p)
        dev = asks[0].device
        # one grid for everything: each side's asked points are sorted once, as queries and (a cloud's) as targets
        origin = _device_origin(ops, asks + [m[0] for m in meshes if m is not None])
        grids = [ops.cloud_grid(p, origin, cell, check=m is None) for p, m in zip(asks, meshes)]
        answers = [g if m is None else ops.mesh_grid(m[0], m[1], origin, cell, max_pairs=self.max_pairs) for g, m in zip(grids, meshes)]

        def nearest(query, answer):
            return (ops.mesh_nearest if isinstance(answer, ops.MeshGrid) else ops.cloud_nearest)(query, answer, md)

        th = torch.from_numpy(self.thresholds).to(dev)
        dp, ip = nearest(grids[0], answers[1])
        dg, ig = nearest(grids[1], answers[0])
        blocks = torch.empty((2, 10), dtype=torch.int64, device=dev)
        ops.cloud_scores(dp, ip, th, asks[0], result=blocks[0])
        ops.cloud_scores(dg, ig, th, asks[1], result=blocks[1])
        blocks = blocks.cpu()  # the one read of the scores
        sp, np_, cp = ops.cloud_scores_read(blocks[0], T)
        sg, ng, cg = ops.cloud_scores_read(blocks[1], T)
        return combine_scores(sp, np_, cp, sg, ng, cg, dist_pred=dp, dist_gt=dg, thresholds=self.thresholds, max_dist=md, pred_points=asks[0])


def evaluate_mesh(mesh, gt, thresholds, **evaluation_args):
    """MeshEvaluation(thresholds, **evaluation_args)(mesh, gt) -> CloudScore: a reconstructed mesh against a ground-truth cloud or mesh.
    A ground truth on the host follows a mesh on the GPU (and the other way round)."""
    vertices, triangles, _ = split_mesh(mesh)
    other = split_mesh(gt, required=False)
    where = place(vertices)
    if place(gt if other is None else other[0]) != where:
        def move(a):
            if where == "host":
                return to_numpy(a)
            import torch
            return torch.as_tensor(to_numpy(a)).to(vertices.device)
        gt = move(gt) if other is None else (move(other[0]), move(other[1]))
    return MeshEvaluation(thresholds, **evaluation_args)(mesh, gt)
