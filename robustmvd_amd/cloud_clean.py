"""Point-cloud clean-up: the neighbours within a radius, the k nearest, PCA normals and outlier removal, for the clouds DepthFusion
makes and the ground-truth scans PointCloudEvaluation reads.  The reference has no such component (it stops at the per-view depth
map); the definition is this docstring, the numpy functions below (the readable specification and the CPU path) and include/mvd.h.

A point with a non-finite coordinate is INVALID.  Coordinates and radii are taken as float32.

Pair distance of a query q and a target p, in float32 and in exactly this order, with no FMA:
       dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z,  d2 = (dx*dx + dy*dy) + dz*dz
   The library is built without contraction, so the device forms float32 numpy's bits: membership and k-NN order are exact integers,
   not verdicts inside bands.  (cloud_eval's nearest kernel contracts to FMAs; its d2 is another number.)
Self exclusion.  When the query cloud IS the target cloud (target=None) a point is never its own neighbour, by index; duplicates of
   a point are its neighbours at distance 0.

(a) Radius neighbourhood.  p_j is a neighbour of q_i iff both are valid and d2 < r2 (strict), r2 = float32(r) * float32(r) in float32.
    Per query: count (int32); sum_dist, the float64 sum of double(sqrtf(d2)); nine float64 moments of
    v = (double(p.x) - double(q.x), double(p.y) - double(q.y), double(p.z) - double(q.z)), taken relative to the QUERY so that
    coordinates of 10^3 cost no digits: sum v (3) and sum v_a v_b for a <= b (6, row-major).
    ORDER: every sum starts from +0.0 and adds the neighbours one after the other in ascending position of the target grid's sorted
    order, that is by (cell key, original index), the cells being those of cloud_eval's definition 3 with edge `cell` from `origin`.
    An invalid query or one without neighbours gives count 0 and zeros.
(b) k nearest within a radius, 1 <= k <= 16.  Per query the up-to-k valid targets with d2 < r2 that are smallest in (bits of d2,
    original index): index (n,k) int32 ascending in that order and -1 past the found ones, dist (n,k) float32 = sqrtf(d2) and max_dist
    past them, count (n) int32.
(c) Moments over a list: (a)'s count, sum of distances (from double(dist)) and moments over each query's list of (b), in list order.
(d) Normals from moments.  The PCA is over the neighbours AND the point itself, which adds zeros: N = count + 1, in float64
    m = sum v / N and C = sum v v^T / N - m m^T.  l0 <= l1 <= l2 are C's eigenvalues and the normal is the unit eigenvector of l0, as
    float32; curvature = float32(l0 / ((l0 + l1) + l2)), the surface variation, 0 when the sum is 0.  The normal is (0,0,0) and the
    curvature NaN where count < min_neighbours (default 5, at least 2), where l1 <= 1e-9 l2 (collinear or coincident neighbours:
    cloud_register.EIGEN_CUT) or where the point is invalid.
    Orientation, in float64 on the unit vector u before it is rounded: with a viewpoint w (one (3,) for the cloud or (n,3) per
    point) dot = (u.x (w.x - q.x) + u.y (w.y - q.y)) + u.z (w.z - q.z); with reference normals r, dot = (u.x r.x + u.y r.y) + u.z r.z;
    u is flipped when dot < 0.  With neither, or where the dot is 0 or not a number (an invalid reference), u is flipped when its
    component of largest magnitude is negative; among equal magnitudes the first one decides.
(e) Outlier removal.  Density: keep iff count >= min_neighbours within radius.  Statistical (PCL's / Open3D's rule):
    mean_i = (sum over the list of double(dist), in list order) / k for a FULL list of k neighbours within max_dist; a point without
    a full list is an outlier.  Over the N points with full lists S1 = sum mean and S2 = sum mean^2 are float64 sums in the two-level
    order of csrc/fixed_sums.h (fixed_sum_numpy); mu = S1 / N, sigma = sqrt(max(S2 - S1 mu, 0) / (N - 1)) (0 for N < 2) and
    threshold = mu + std_ratio sigma (-inf for N = 0); keep iff mean_i <= threshold.  Invalid points are always dropped.  The kept rows
    (points, colours, normals) follow in ascending original index, with `kept`, their indices.

On the device (csrc/cloud_clean.hip) the two queries run on the sorted grid of ops.cloud_grid with cell = radius * (1 + 2^-10) from
the per-axis minimum of the valid targets; no kernel uses an atomic, and two calls give the same bits.  Every function picks the
host or the device by where its inputs are.
"""
from dataclasses import dataclass

import numpy as np

from .cloud_eval import INDEX_LIMIT, host_points
from .cloud_register import EIGEN_CUT
from .mesh import one_place, place, to_numpy

KNN_MAX = 16
CELL_MARGIN = 1.0 + 2.0 ** -10  # ops.CLOUD_CELL_MARGIN, which the host path does not import torch for


@dataclass
class KNN:
    """index (n,k) int32, dist (n,k) float32, count (n) int32 (definition b)"""
    index: object
    dist: object
    count: object


@dataclass
class Neighbourhood:
    """count (n) int32, sum_dist (n) float64, moments (n,9) float64 (definition a)"""
    count: object
    sum_dist: object
    moments: object


@dataclass
class CleanResult:
    """points (K,3), colors and normals (K,3) or None: the kept rows; keep (n) bool; kept (K) int32: the kept points' indices;
    threshold: the statistical rule's float, None for the density rule"""
    points: object
    colors: object
    normals: object
    keep: object
    kept: object
    threshold: object


def _f32(value, name):
    v = np.float32(value)
    if not (v > 0 and np.isfinite(v)):
        raise ValueError(f"{name} must be finite and > 0, got {value}")
    return v


def _check_k(k):
    if int(k) != k or not 1 <= int(k) <= KNN_MAX:
        raise ValueError(f"k = {k}, supported 1..{KNN_MAX}")
    return int(k)


def _pair_d2(q, p):
    """(a,3) x (b,3) float32 -> (a,b) float32: the pair distance's chain"""
    with np.errstate(all="ignore"):
        d = q[:, None, :] - p[None, :, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _chunks(n, m):
    step = max(1, (1 << 22) // max(m, 1))
    return [(b, min(b + step, n)) for b in range(0, n, step)]


def knn_numpy(points, k, max_dist, target=None):
    """Definition (b) as chunked brute force -> KNN."""
    q, k, md = host_points(points, "points"), _check_k(k), _f32(max_dist, "max_dist")
    p = q if target is None else host_points(target, "target")
    n, m, r2 = len(q), len(p), md * md
    index, dist, count = np.full((n, k), -1, np.int32), np.full((n, k), md, np.float32), np.zeros(n, np.int32)
    q_ok, p_ok = np.isfinite(q).all(axis=1), np.isfinite(p).all(axis=1)
    none = np.uint64(0xffffffffffffffff)
    for b, e in _chunks(n, m):
        if m == 0:
            break
        d2 = _pair_d2(q[b:e], p)
        with np.errstate(invalid="ignore"):
            ok = (d2 < r2) & p_ok[None, :] & q_ok[b:e, None]
        if target is None:
            ok[np.arange(e - b), np.arange(b, e)] = False
        key = (np.where(ok, d2, np.float32(0)).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(m, dtype=np.uint64)[None, :]
        key = np.where(ok, key, none)
        kk = min(k, m)
        best = np.sort(np.partition(key, kk - 1, axis=1)[:, :kk], axis=1)
        found = best != none
        index[b:e, :kk] = np.where(found, (best & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32)
        d = np.sqrt((best >> np.uint64(32)).astype(np.uint32).view(np.float32))
        dist[b:e, :kk] = np.where(found, d, md)
        count[b:e] = found.sum(axis=1)
    return KNN(index, dist, count)


def grid_order_numpy(target, cell, origin=None):
    """The target grid's sorted order -> (order (m) int64: the stable sort of the cell keys, invalid points last; origin (3,) float64).
    The keys are cloud_eval's definition 3 with the edge `cell` as a float64 (voxel_keys_numpy takes its edge as float32, which
    radius * (1 + 2^-10) is not); ValueError when an index leaves [0, 2^21 - 1)."""
    p = host_points(target, "target")
    cell = float(cell)
    if not 0.0 < cell < float("inf"):
        raise ValueError(f"cell must be finite and > 0, got {cell}")
    ok = np.isfinite(p).all(axis=1)
    if origin is None:
        origin = p[ok].min(axis=0).astype(np.float64) if ok.any() else np.zeros(3)
    origin = np.asarray(origin, dtype=np.float64).reshape(-1)
    if origin.shape != (3,) or not np.isfinite(origin).all():
        raise ValueError(f"origin must be 3 finite numbers, got {origin.tolist()}")
    inv = 1.0 / cell
    keys = np.full(len(p), np.iinfo(np.int64).max, dtype=np.int64)
    if ok.any():
        idx = np.floor((p[ok].astype(np.float64) - origin) * inv)
        if idx.min() < 0 or idx.max() >= INDEX_LIMIT:
            raise ValueError(f"cloud_grid: the points span {p[ok].min(axis=0).tolist()} .. {p[ok].max(axis=0).tolist()} from origin "
                             f"{origin.tolist()}, which at an edge of {cell:g} gives indices {idx.min():.0f} .. {idx.max():.0f}; each "
                             f"must be in [0, {INDEX_LIMIT})")
        idx = idx.astype(np.int64)
        keys[ok] = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    return np.argsort(keys, kind="stable"), origin


def _moment_terms(q, p, dist):
    """rows of (double(dist), v (3), v_a v_b for a <= b (6)) for the pairs (q[i], p[i]) -> (pairs,10) float64"""
    v = p.astype(np.float64) - q.astype(np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([dist.astype(np.float64), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], axis=1)


def neighbourhood_numpy(points, radius, target=None, origin=None, cell=None):
    """Definition (a) as chunked brute force -> Neighbourhood.  origin, cell: the target grid's, which fix the order of the sums;
    by default the per-axis minimum over the valid targets and radius * (1 + 2^-10), the device path's.  ValueError as ops.cloud_grid
    when the targets do not fit the grid's keys, or when cell is below radius * (1 + 2^-10)."""
    q, r = host_points(points, "points"), _f32(radius, "radius")
    p = q if target is None else host_points(target, "target")
    cell = float(r) * CELL_MARGIN if cell is None else float(cell)
    if cell < float(r) * CELL_MARGIN * (1 - 1e-12):
        raise ValueError(f"the grid's cell {cell:g} is below radius * (1 + 2^-10) = {float(r) * CELL_MARGIN:g}")
    order, _ = grid_order_numpy(p, cell, origin)
    n, m, r2 = len(q), len(p), r * r
    ps = p[order]
    q_ok, p_ok = np.isfinite(q).all(axis=1), np.isfinite(ps).all(axis=1)
    count, sums = np.zeros(n, np.int32), np.zeros((n, 10))
    for b, e in _chunks(n, m):
        if m == 0:
            break
        d2 = _pair_d2(q[b:e], ps)
        with np.errstate(invalid="ignore"):
            ok = (d2 < r2) & p_ok[None, :] & q_ok[b:e, None]
        if target is None:
            ok &= order[None, :] != np.arange(b, e)[:, None]
        qi, pj = np.nonzero(ok)  # row-major: per query in ascending sorted position
        count[b:e] = ok.sum(axis=1)
        np.add.at(sums, qi + b, _moment_terms(q[qi + b], ps[pj], np.sqrt(d2[qi, pj])))  # unbuffered: one pair after the other
    return Neighbourhood(count, sums[:, 0].copy(), sums[:, 1:].copy())


def list_moments_numpy(points, target, index, dist):
    """Definition (c) -> Neighbourhood; target None: the points themselves."""
    q = host_points(points, "points")
    p = q if target is None else host_points(target, "target")
    index, dist = np.asarray(to_numpy(index), dtype=np.int32), np.asarray(to_numpy(dist), dtype=np.float32)
    if index.ndim != 2 or index.shape[0] != len(q) or dist.shape != index.shape:
        raise ValueError(f"index and dist must be ({len(q)},k), got {index.shape} and {dist.shape}")
    count, sums = np.zeros(len(q), np.int32), np.zeros((len(q), 10))
    live = np.ones(len(q), dtype=bool)
    for s in range(index.shape[1]):
        live &= (index[:, s] >= 0) & (index[:, s] < len(p))  # the first index outside the targets ends a list
        rows = np.flatnonzero(live)
        sums[rows] += _moment_terms(q[rows], p[index[rows, s]], dist[rows, s])
        count[rows] += 1
    return Neighbourhood(count, sums[:, 0].copy(), sums[:, 1:].copy())


def _orientation(toward, like, n):
    """-> (mode 0..3, array): no orientation, one viewpoint (3,) float64, per-point viewpoints (n,3) float32, reference normals"""
    if toward is not None and like is not None:
        raise ValueError("toward and like: at most one of them")
    if like is not None:
        ref = np.asarray(to_numpy(like), dtype=np.float32)
        if ref.shape != (n, 3):
            raise ValueError(f"like: shape {ref.shape}, expected {(n, 3)}")
        return 3, ref
    if toward is None:
        return 0, None
    w = np.asarray(to_numpy(toward))
    if w.shape == (3,):
        w = w.astype(np.float64)
        if not np.isfinite(w).all():
            raise ValueError(f"toward must be finite, got {w.tolist()}")
        return 1, w
    if w.shape != (n, 3):
        raise ValueError(f"toward: shape {w.shape}, expected (3,) or {(n, 3)}")
    return 2, w.astype(np.float32)


def normals_from_moments_numpy(points, count, moments, min_neighbours=5, toward=None, like=None):
    """Definition (d) -> (normals (n,3) float32, curvature (n) float32), the eigenvectors from numpy.linalg.eigh."""
    q = host_points(points, "points")
    n = len(q)
    count, M = np.asarray(to_numpy(count)), np.asarray(to_numpy(moments), dtype=np.float64)
    if count.shape != (n,) or M.shape != (n, 9):
        raise ValueError(f"count and moments must be ({n},) and ({n},9), got {count.shape} and {M.shape}")
    if int(min_neighbours) < 2:
        raise ValueError(f"min_neighbours = {min_neighbours}, at least 2")
    mode, w = _orientation(toward, like, n)
    normals, curvature = np.zeros((n, 3), np.float32), np.full(n, np.nan, np.float32)
    rows = np.flatnonzero(np.isfinite(q).all(axis=1) & (count >= int(min_neighbours)))
    if len(rows) == 0:
        return normals, curvature
    N = count[rows].astype(np.float64) + 1.0
    mean = M[rows, :3] / N[:, None]
    C = np.empty((len(rows), 3, 3))
    for t, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[:, a, b] = C[:, b, a] = M[rows, 3 + t] / N - mean[:, a] * mean[:, b]
    lam, vec = np.linalg.eigh(C)
    good = lam[:, 1] > EIGEN_CUT * lam[:, 2]
    rows, lam, u = rows[good], lam[good], vec[good][:, :, 0]
    u = u / np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])[:, None]
    dot = np.zeros(len(rows))
    if mode in (1, 2):
        d = (w[None, :] if mode == 1 else w[rows].astype(np.float64)) - q[rows].astype(np.float64)
        dot = (u[:, 0] * d[:, 0] + u[:, 1] * d[:, 1]) + u[:, 2] * d[:, 2]
    elif mode == 3:
        d = w[rows].astype(np.float64)
        with np.errstate(invalid="ignore"):
            dot = (u[:, 0] * d[:, 0] + u[:, 1] * d[:, 1]) + u[:, 2] * d[:, 2]
    au = np.abs(u)
    first = np.where((au[:, 0] >= au[:, 1]) & (au[:, 0] >= au[:, 2]), 0, np.where(au[:, 1] >= au[:, 2], 1, 2))
    with np.errstate(invalid="ignore"):
        tie = ~(dot < 0) & ~(dot > 0)
        flip = np.where(tie, u[np.arange(len(rows)), first] < 0, dot < 0)
    u = np.where(flip[:, None], -u, u)
    normals[rows] = u.astype(np.float32)
    total = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
    with np.errstate(all="ignore"):
        curvature[rows] = np.where(total == 0, 0.0, lam[:, 0] / total).astype(np.float32)
    return normals, curvature


def _normal_arguments(radius, k, max_dist):
    if (radius is None) == (k is None):
        raise ValueError("estimate_normals: exactly one of radius and k is given")
    if k is not None and max_dist is None:
        raise ValueError("estimate_normals: k needs max_dist")
    if radius is not None and max_dist is not None:
        raise ValueError("estimate_normals: max_dist belongs to k")


def estimate_normals_numpy(points, radius=None, k=None, max_dist=None, toward=None, like=None, min_neighbours=5):
    """estimate_normals on the host: (a), or (b) followed by (c), then (d)."""
    _normal_arguments(radius, k, max_dist)
    if radius is not None:
        nb = neighbourhood_numpy(points, radius)
    else:
        lists = knn_numpy(points, k, max_dist)
        nb = list_moments_numpy(points, None, lists.index, lists.dist)
    return normals_from_moments_numpy(points, nb.count, nb.moments, min_neighbours, toward, like)


def _wave_tree(v):
    """(..., 64) -> (...): v += shuffle_xor(v, s) for s = 32 .. 1, as lane 0 sees it"""
    for s in (32, 16, 8, 4, 2, 1):
        v = v[..., :s] + v[..., s:2 * s]
    return v[..., 0]


def _workgroup_sum(acc):
    """(B,256) per-thread values -> (B,): the tree inside each wave, then the waves in wave order"""
    w = _wave_tree(acc.reshape(len(acc), 4, 64))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def fixed_sum_numpy(terms):
    """The float64 sum of terms (n,) in the two-level order of csrc/fixed_sums.h with 2048 items per workgroup, as
    mvd_cloud_knn_mean_sums_f32 forms it: thread t of workgroup g adds the items 2048 g + t + 256 j for j = 0..7 from +0.0; the
    workgroup's sum is the xor tree inside each wave, then the four waves in order; one workgroup adds the workgroups' sums, thread t
    the sums t, t + 256, ... from +0.0, and joins them the same way.  A skipped item is a +0.0, which leaves the bits alone."""
    a = np.asarray(terms, dtype=np.float64).reshape(-1)
    groups = -(-len(a) // 2048)
    pad = np.zeros(groups * 2048)
    pad[:len(a)] = a
    acc = np.zeros((groups, 256))
    for j in range(8):
        acc = acc + pad.reshape(groups, 8, 256)[:, j]
    partial = _workgroup_sum(acc) if groups else np.zeros(0)
    steps = -(-groups // 256)
    pad = np.zeros(steps * 256)
    pad[:groups] = partial
    acc = np.zeros(256)
    for row in pad.reshape(steps, 256):
        acc = acc + row
    return float(_workgroup_sum(acc[None])[0])


def statistical_threshold(sum_mean, sum_square, N, std_ratio):
    """Definition (e)'s threshold from the two float64 sums over the N full lists."""
    if N == 0:
        return float("-inf")
    mu = np.float64(sum_mean) / np.float64(N)
    sigma = np.sqrt(max(np.float64(sum_square) - np.float64(sum_mean) * mu, 0.0) / np.float64(N - 1)) if N >= 2 else np.float64(0.0)
    return float(mu + np.float64(std_ratio) * sigma)


def knn_means_numpy(dist, count):
    """dist (n,k), count (n) of (b) -> mean (n) float64: the sum of double(dist) in list order over k, NaN without a full list"""
    dist, count = np.asarray(dist, dtype=np.float32), np.asarray(count)
    k = dist.shape[1]
    s = np.zeros(len(dist))
    for j in range(k):
        s = s + dist[:, j].astype(np.float64)
    return np.where(count == k, s / np.float64(k), np.nan)


def _outlier_rule(radius, min_neighbours, k, std_ratio, max_dist):
    """-> "density" or "statistical"; ValueError names the arguments that do not go together"""
    given = {name for name, v in (("radius", radius), ("min_neighbours", min_neighbours), ("k", k), ("std_ratio", std_ratio),
                                  ("max_dist", max_dist)) if v is not None}
    if given == {"radius", "min_neighbours"}:
        if int(min_neighbours) != min_neighbours or int(min_neighbours) < 0:
            raise ValueError(f"min_neighbours = {min_neighbours}, an integer >= 0")
        return "density"
    if given == {"k", "std_ratio", "max_dist"}:
        if not np.isfinite(np.float64(std_ratio)):
            raise ValueError(f"std_ratio must be finite, got {std_ratio}")
        return "statistical"
    raise ValueError(f"remove_outliers takes radius with min_neighbours (the density rule) or k with std_ratio and max_dist (the "
                     f"statistical rule), got {sorted(given)}")


def _host_rows(a, name, n):
    if a is None:
        return None
    a = np.asarray(to_numpy(a), dtype=np.float32)
    if a.shape != (n, 3):
        raise ValueError(f"{name}: shape {a.shape}, expected {(n, 3)}")
    return a


def remove_outliers_numpy(points, colors=None, normals=None, *, radius=None, min_neighbours=None, k=None, std_ratio=None, max_dist=None):
    """Definition (e) on the host -> CleanResult."""
    rule = _outlier_rule(radius, min_neighbours, k, std_ratio, max_dist)
    p = host_points(points, "points")
    colors, normals = _host_rows(colors, "colors", len(p)), _host_rows(normals, "normals", len(p))
    if rule == "density":
        keep = np.isfinite(p).all(axis=1) & (neighbourhood_numpy(p, radius).count >= int(min_neighbours))
        threshold = None
    else:
        lists = knn_numpy(p, k, max_dist)
        mean = knn_means_numpy(lists.dist, lists.count)
        full = ~np.isnan(mean)
        mu = np.where(full, mean, 0.0)
        threshold = statistical_threshold(fixed_sum_numpy(mu), fixed_sum_numpy(mu * mu), int(full.sum()), std_ratio)
        with np.errstate(invalid="ignore"):
            keep = mean <= threshold
    kept = np.flatnonzero(keep).astype(np.int32)
    take = lambda a: None if a is None else a[kept]
    return CleanResult(p[kept], take(colors), take(normals), keep, kept, threshold)


# ---- the device path and the front ends ------------------------------------------------------------------------------------------------

def _on_host(points, *others):
    return one_place(points, *[o for o in others if o is not None], what="clouds and their attributes") == "host"


def _device_grid(target, radius, name="target"):
    """The target grid of a query at `radius`: cell = float32(radius) * (1 + 2^-10) from the per-axis minimum of the valid targets."""
    from . import ops
    p = ops.cloud_points(target, name)
    extent = ops.cloud_extent(p)
    origin = [0.0, 0.0, 0.0] if extent is None else extent[0].tolist()
    return ops.cloud_grid(p, origin, float(_f32(radius, "radius")) * ops.CLOUD_CELL_MARGIN)


def cloud_knn(points, k, max_dist, target=None):
    """The k nearest targets of every point within max_dist (definition b) -> KNN.  target None: the cloud against itself."""
    if _on_host(points, target):
        return knn_numpy(points, k, max_dist, target)
    from . import ops
    k, md = _check_k(k), _f32(max_dist, "max_dist")
    grid = _device_grid(points if target is None else target, md, "points" if target is None else "target")
    return KNN(*ops.cloud_knn(None if target is None else points, grid, k, float(md)))


def cloud_neighbourhood(points, radius, target=None):
    """The neighbours of every point within radius (definition a) -> Neighbourhood.  target None: the cloud against itself."""
    if _on_host(points, target):
        return neighbourhood_numpy(points, radius, target)
    from . import ops
    r = _f32(radius, "radius")
    grid = _device_grid(points if target is None else target, r, "points" if target is None else "target")
    return Neighbourhood(*ops.cloud_radius_moments(None if target is None else points, grid, float(r)))


def estimate_normals(points, radius=None, k=None, max_dist=None, toward=None, like=None, min_neighbours=5):
    """PCA normals of a cloud (definition d) -> (normals (n,3) float32, curvature (n) float32).  Exactly one of radius (the
    neighbours within it) and k (the k nearest within max_dist) is given.  toward: a viewpoint (3,) or per-point viewpoints (n,3) the
    normals look at; like: reference normals (n,3) they agree with; neither: the largest component is positive.  Where there are fewer
    than min_neighbours neighbours, or they are collinear, the normal is (0,0,0) and the curvature NaN."""
    _normal_arguments(radius, k, max_dist)
    if place(points) == "host":
        return estimate_normals_numpy(points, radius, k, max_dist, toward, like, min_neighbours)
    import torch
    from . import ops
    p = ops.cloud_points(points, "points")
    if radius is not None:
        count, _, moments = ops.cloud_radius_moments(None, _device_grid(p, radius, "points"), float(_f32(radius, "radius")))
    else:
        k, md = _check_k(k), _f32(max_dist, "max_dist")
        index, dist, _ = ops.cloud_knn(None, _device_grid(p, md, "points"), k, float(md))
        count, _, moments = ops.cloud_list_moments(p, p, index, dist)
    mode, w = _orientation(toward, like, p.shape[0])  # the same checks as the host's; the arrays go back to the device
    if mode >= 2:
        w = torch.from_numpy(w).to(p.device)
    return ops.cloud_normals(p, count, moments, min_neighbours, toward=w if mode in (1, 2) else None, like=w if mode == 3 else None)


def remove_outliers(points, colors=None, normals=None, *, radius=None, min_neighbours=None, k=None, std_ratio=None, max_dist=None):
    """Outlier removal (definition e) -> CleanResult.  radius with min_neighbours: keep the points with at least that many neighbours
    within radius.  k with std_ratio and max_dist: keep the points whose mean distance to their k nearest neighbours (within max_dist)
    is at most the cloud's mean + std_ratio standard deviations.  colors, normals (n,3): rows that follow the points."""
    rule = _outlier_rule(radius, min_neighbours, k, std_ratio, max_dist)
    if _on_host(points, colors, normals):
        return remove_outliers_numpy(points, colors, normals, radius=radius, min_neighbours=min_neighbours, k=k, std_ratio=std_ratio,
                                     max_dist=max_dist)
    import torch
    from . import _lib as L
    from . import ops
    p = ops.cloud_points(points, "points")
    n, dev = p.shape[0], p.device
    rows = [p] + [None if a is None else L.as_f32(a, name, (n, 3), dev) for a, name in ((colors, "colors"), (normals, "normals"))]
    if rule == "density":
        count, _, _ = ops.cloud_radius_moments(None, _device_grid(p, radius, "points"), float(_f32(radius, "radius")))
        keep, threshold = ops.cloud_keep_density(p, count, min_neighbours), None
    else:
        k, md = _check_k(k), _f32(max_dist, "max_dist")
        _, dist, count = ops.cloud_knn(None, _device_grid(p, md, "points"), k, float(md))
        mean, block = ops.cloud_knn_mean_sums(dist, count)
        threshold = statistical_threshold(*ops.cloud_knn_mean_sums_read(block), std_ratio)  # the one read of the rule
        keep = ops.cloud_keep_threshold(mean, threshold)
    kept, remap, K = ops.cloud_select(keep)
    out = [None if a is None else ops.mesh_gather_rows(a, remap, K) for a in rows]
    return CleanResult(out[0], out[1], out[2], keep.view(torch.bool), kept, threshold)


def cloud_spacing(points, max_dist):
    """The mean distance of a point to its nearest neighbour within max_dist, over the points that have one (NaN when none has):
    a scale for choosing `radius` and the evaluation's `voxel`.  k = 1 of definition (b); a float64 sum of the float32 distances."""
    md = _f32(max_dist, "max_dist")
    if place(points) == "host":
        lists = knn_numpy(points, 1, md)
        found = lists.count == 1
        return float(np.sum(lists.dist[found, 0].astype(np.float64)) / found.sum()) if found.any() else float("nan")
    import torch
    from . import ops
    p = ops.cloud_points(points, "points")
    n = p.shape[0]
    index, dist, _ = ops.cloud_knn(None, _device_grid(p, md, "points"), 1, float(md))
    # mvd_cloud_scores_f32 looks at `points` only where index < 0, and leaves an invalid one out: with every point invalid it
    # sums and counts exactly the queries that found a neighbour
    nobody = torch.full((n, 3), float("nan"), dtype=torch.float32, device=p.device)
    total, found, _ = ops.cloud_scores_read(ops.cloud_scores(dist.reshape(n), index.reshape(n), (float(md),), nobody), 1)
    return total / found if found else float("nan")
