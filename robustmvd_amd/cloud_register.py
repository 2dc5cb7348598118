"""Point-cloud registration (ICP): a source cloud S (n,3) float32 is moved onto a fixed target cloud P (m,3) float32 by a rigid map, a
similarity or a point-to-plane fit, on the truncated nearest neighbour of cloud_eval.py.  DTU and Tanks and Temples register the
reconstruction to the ground truth before they take distances; PointCloudEvaluation(align=...) does it with this module.  The
reference has no such component: the definition is this docstring, the float64 numpy functions below (the readable specification
and the CPU path) and include/mvd.h.

A registration is T: x -> M x + t with M = s R (3,3) float64 and t float64, kept as a (4,4) matrix [[M, t], [0, 1]].  A point with
a non-finite coordinate is INVALID and never pairs.  One iteration k, from T_k and a radius rho:

1. Move (transform_numpy).  q_i,a = float32(((M[a,0] x + M[a,1] y) + M[a,2] z) + t[a]) per axis a, in float64 in exactly this order,
   rounded once.  A row with a non-finite coordinate before or after the move is (NaN, NaN, NaN) with the bits 0x7fc00000.  numpy and
   the device agree bit for bit.  A normal goes through M alone, in the same order, and is divided by its float64 length
   sqrt((w_x w_x + w_y w_y) + w_z w_z); an invalid or vanishing normal becomes (0, 0, 0).

2. Pair.  (d_i, j_i) = the truncated nearest neighbour of q_i in P with max_dist = rho (cloud_eval.py, definition 1).  Pair i exists
   iff j_i >= 0; in plane mode also only if the target normal at j_i is finite and not (0, 0, 0).

3. Sum (pair_sums_numpy).  With one pivot c (3 float64 from the host: the centre of the valid targets' bounding box),
   a = float64(q_i) - c, b = float64(P_j) - c, d = a - b, every operation in float64 and per pair in this order:
     point mode (N and 18 sums):  a_x, a_y, a_z;  b_x, b_y, b_z;  a_r * b_c for r, c in x, y, z (row-major);
                                  (a_x a_x + a_y a_y) + a_z a_z;  the same of b;  the same of d
     plane mode (N and 28 sums):  u = float64(normal_j),  r = (d_x u_x + d_y u_y) + d_z u_z,
                                  J = (a_y u_z - a_z u_y,  a_z u_x - a_x u_z,  a_x u_y - a_y u_x,  u_x, u_y, u_z);
                                  J_i * J_k for i <= k (21, row-major);  J_k * r (6);  r * r
   Per pair the device and numpy form the same bits; only the order in which the pairs are added differs (numpy: pairwise, in the
   source's order; the device: csrc/cloud_register.hip).

4. Solve (host, float64 numpy, shared by both paths).
     rigid / similarity (solve_point): Umeyama.  mu_a = sum a / N, mu_b = sum b / N, C = sum b a^T / N - mu_b mu_a^T = U D V^T (SVD),
       S = diag(1, 1, sign(det U det V)) (the reflection fix), R = U S V^T, s = 1 (rigid) or tr(D S) / var_a with
       var_a = sum |a|^2 / N - |mu_a|^2 (similarity; 1 when var_a is 0).  Delta: x -> c + mu_b + s R (x - c - mu_a).
     plane (solve_plane): the minimum-norm solution of (sum J J^T) x = - sum J r through the eigen-decomposition, leaving out the
       eigen-directions whose eigenvalue is below 1e-9 x the largest: a direction in which the target can slide gets a zero update.
       omega = x[:3] is a rotation vector (Rodrigues) about the pivot, v = x[3:]: Delta: x -> c + Rod(omega) (x - c) + v.
   N >= 3 pairs are needed (N >= 6 in plane mode): otherwise the registration stops with converged=False, reason="too few pairs".

5. Step and stop.  T_{k+1} = Delta_k o T_k.  step_k = the largest displacement Delta_k gives to the 8 corners of the valid source's
   bounding box as T_k moves them.  The displacement of an affine map is convex, and the moved box holds every moved source point, so
   step_k bounds the displacement of every point; the box comes from one read before the first iteration, which keeps an iteration
   on the device at one 256-byte read.  A stage has converged when step_k <= tol; the default tol is
   max(1e-3 x the last radius, 2^-21 x the largest |coordinate| of the valid targets): below a few float32 ulps of the coordinates
   the re-rounded q jitters and the step never shrinks.  A stage also ends after `iterations` iterations.

max_dist is one radius or a descending sequence of radii (stages), each with its own iteration budget; the next stage starts from
where the last one ended, converged or not.  On the device the target grid is built once with the cell of the largest radius, which
mvd_cloud_nearest_f32's contract allows for every smaller one; the moved source is keyed and sorted before every iteration, which
decides the nearest kernel's speed and never its result (_register_device).  rmse = sqrt(sum |a - b|^2 / N) (plane mode: sqrt(sum r^2 / N), the
point-to-plane residual).  The result's rmse and pairs are those of the last iteration, measured under the last T that was paired
(T before that iteration's update); `converged` is the last stage's.
"""
from dataclasses import dataclass, field

import numpy as np

from .cloud_eval import host_points, nearest_numpy
from .mesh import is_tensor, one_place, place, to_numpy

MODES = ("rigid", "similarity", "plane")
POINT_SUMS, PLANE_SUMS = 18, 28
MIN_PAIRS = {"rigid": 3, "similarity": 3, "plane": 6}
EIGEN_CUT = 1e-9


def affine_parts(transform):
    """(4,4) or (3,4) -> (M (3,3), t (3,)) float64, finite; a (4,4) must end in the row 0 0 0 1."""
    T = np.asarray(to_numpy(transform), dtype=np.float64)
    if T.shape == (4, 4):
        if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError(f"transform: the last row must be 0 0 0 1, got {T[3].tolist()}")
    elif T.shape != (3, 4):
        raise ValueError(f"transform must be (4,4) or (3,4), got {T.shape}")
    if not np.isfinite(T).all():
        raise ValueError("transform must be finite")
    return T[:3, :3].copy(), T[:3, 3].copy()


def _matrix(M, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = M, t
    return T


def _normals(a, n, name="normals"):
    v = np.asarray(to_numpy(a), dtype=np.float32)
    if v.shape != (n, 3):
        raise ValueError(f"{name}: shape {v.shape}, expected {(n, 3)}")
    return v


def _through(M, x, t=None):
    """((M[a,0] x + M[a,1] y) + M[a,2] z) [+ t[a]] per axis, float64, in the definition's order."""
    cols = []
    for a in range(3):
        v = (M[a, 0] * x[:, 0] + M[a, 1] * x[:, 1]) + M[a, 2] * x[:, 2]
        cols.append(v if t is None else v + t[a])
    return np.stack(cols, axis=1) if len(x) else np.zeros((0, 3))


def transform_numpy(points, transform, normals=None):
    """Definition 1 -> q (n,3) float32, or (q, normals (n,3) float32) when normals are given."""
    p = host_points(points, "points")
    M, t = affine_parts(transform)
    with np.errstate(all="ignore"):
        q = _through(M, p.astype(np.float64), t).astype(np.float32)
        bad = ~(np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1))
        q[bad] = np.float32(np.nan)
        if normals is None:
            return q
        v = _normals(normals, len(p))
        w = _through(M, v.astype(np.float64))
        length = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        ok = np.isfinite(v).all(axis=1) & (length > 0) & np.isfinite(length)
        out = np.zeros((len(p), 3), dtype=np.float32)
        out[ok] = (w[ok] / length[ok, None]).astype(np.float32)
    return q, out


def pair_terms_numpy(source, transform, index, target, pivot, target_normals=None):
    """Definition 3's terms, one row per pair in the source's order -> (N, 18) or (N, 28) float64 (plane mode: with target_normals)."""
    s, p = host_points(source, "source"), host_points(target, "target")
    j = np.asarray(to_numpy(index)).astype(np.int64).reshape(-1)
    if j.shape != (len(s),):
        raise ValueError(f"index: shape {j.shape}, expected {(len(s),)}")
    c = np.asarray(pivot, dtype=np.float64).reshape(-1)
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError(f"pivot must be 3 finite numbers, got {c.tolist()}")
    q = transform_numpy(s, transform)
    has = (j >= 0) & (j < len(p))
    jj = np.where(has, j, 0)
    if len(p) == 0:
        has[:] = False
        pj = np.zeros((len(s), 3), np.float32)
    else:
        pj = p[jj]
    pair = has & np.isfinite(q).all(axis=1) & np.isfinite(pj).all(axis=1)
    if target_normals is not None:
        nrm = _normals(target_normals, len(p), "target_normals")
        u = nrm[jj] if len(p) else np.zeros((len(s), 3), np.float32)
        pair &= np.isfinite(u).all(axis=1) & (u != 0).any(axis=1)
        u = u[pair].astype(np.float64)
    a = q[pair].astype(np.float64) - c
    b = pj[pair].astype(np.float64) - c
    d = a - b
    sq = lambda v: (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    if target_normals is None:
        cols = [a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2]]
        cols += [a[:, r] * b[:, k] for r in range(3) for k in range(3)]
        cols += [sq(a), sq(b), sq(d)]
    else:
        r = (d[:, 0] * u[:, 0] + d[:, 1] * u[:, 1]) + d[:, 2] * u[:, 2]
        J = [a[:, 1] * u[:, 2] - a[:, 2] * u[:, 1], a[:, 2] * u[:, 0] - a[:, 0] * u[:, 2], a[:, 0] * u[:, 1] - a[:, 1] * u[:, 0],
             u[:, 0], u[:, 1], u[:, 2]]
        cols = [J[i] * J[k] for i in range(6) for k in range(i, 6)] + [J[k] * r for k in range(6)] + [r * r]
    return np.stack(cols, axis=1) if len(a) else np.zeros((0, len(cols)))


def pair_sums_numpy(source, transform, index, target, pivot, target_normals=None):
    """Definition 3 -> (N int, sums (18,) or (28,) float64)."""
    terms = pair_terms_numpy(source, transform, index, target, pivot, target_normals)
    return len(terms), terms.sum(axis=0)


def _rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def solve_point(N, sums, pivot, similarity=False):
    """Definition 4, rigid / similarity -> (M (3,3), t (3,)) of Delta, from the point-mode sums."""
    sums, c = np.asarray(sums, dtype=np.float64), np.asarray(pivot, dtype=np.float64)
    if sums.shape != (POINT_SUMS,) or N < MIN_PAIRS["rigid"]:
        raise ValueError(f"solve_point: {POINT_SUMS} sums over at least {MIN_PAIRS['rigid']} pairs, got {sums.shape} over {N}")
    mu_a, mu_b = sums[0:3] / N, sums[3:6] / N
    C = sums[6:15].reshape(3, 3).T / N - np.outer(mu_b, mu_a)
    U, D, Vt = np.linalg.svd(C)
    S = np.array([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    R = (U * S) @ Vt
    s = 1.0
    if similarity:
        var_a = sums[15] / N - float(mu_a @ mu_a)
        s = float((D * S).sum() / var_a) if var_a > 0 else 1.0
    M = s * R
    return M, c + mu_b - M @ (c + mu_a)


def solve_plane(N, sums, pivot):
    """Definition 4, plane -> (M, t) of Delta, from the plane-mode sums."""
    sums, c = np.asarray(sums, dtype=np.float64), np.asarray(pivot, dtype=np.float64)
    if sums.shape != (PLANE_SUMS,) or N < MIN_PAIRS["plane"]:
        raise ValueError(f"solve_plane: {PLANE_SUMS} sums over at least {MIN_PAIRS['plane']} pairs, got {sums.shape} over {N}")
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[:21]
    A = A + np.triu(A, 1).T
    g = sums[21:27]
    lam, V = np.linalg.eigh(A)
    keep = lam > EIGEN_CUT * lam.max() if lam.max() > 0 else np.zeros(6, dtype=bool)
    x = -(V[:, keep] * (1.0 / lam[keep])) @ (V[:, keep].T @ g)
    M = _rodrigues(x[:3])
    return M, c - M @ c + x[3:]


@dataclass
class Registration:
    """transform (4,4) float64: source -> target; scale = det(M)^(1/3); rmse, pairs: of the last iteration (module docstring);
    iterations: over all stages; converged, reason ("converged", "iterations", "too few pairs"); history: one
    (radius, pairs, rmse, step) per iteration (step NaN where no update was made)."""
    transform: np.ndarray
    scale: float
    rmse: float
    pairs: int
    iterations: int
    converged: bool
    reason: str
    history: list = field(default_factory=list)

    def apply(self, points, normals=None):
        """points (n,3) (and normals) through the transform: numpy arrays by transform_numpy, GPU tensors by ops.cloud_transform."""
        if place(points) == "host":
            return transform_numpy(points, self.transform, normals)
        from . import ops
        return ops.cloud_transform(points, self.transform, normals)


def check_radii(max_dist):
    r = np.atleast_1d(np.asarray(max_dist, dtype=np.float32))
    if r.ndim != 1 or len(r) == 0 or not (np.isfinite(r).all() and (r > 0).all()):
        raise ValueError(f"max_dist must be one or more finite radii > 0, got {max_dist}")
    if (np.diff(r) > 0).any():
        raise ValueError(f"max_dist: the radii must descend, got {r.tolist()}")
    return [float(v) for v in r]


def _box_corners(lo, hi):
    return np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)


def _iterate(pair_sums, begin_stage, radii, mode, init, iterations, tol, source_box, target_box):
    """Definitions 4 and 5 around a backend: pair_sums(M, t, radius) -> (N, sums), begin_stage(M, t, radius).  source_box /
    target_box: (2,3) float64 min and max over the valid points, or None."""
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError(f"iterations must be at least 1, got {iterations}")
    M, t = init
    pivot = np.zeros(3) if target_box is None else 0.5 * (target_box[0] + target_box[1])
    if tol is None:
        tol = max(1e-3 * radii[-1], 2.0 ** -21 * (0.0 if target_box is None else float(np.abs(target_box).max())))
    tol = float(tol)
    if not tol >= 0:
        raise ValueError(f"tol must be >= 0, got {tol}")
    corners = None if source_box is None else _box_corners(source_box[0], source_box[1])
    history, converged, reason, N, rmse = [], False, "iterations", 0, float("nan")
    for radius in radii:
        begin_stage(M, t, radius)
        converged = False
        for _ in range(iterations):
            N, sums = pair_sums(M, t, radius, pivot)
            rmse = float(np.sqrt(max(sums[-1], 0.0) / N)) if N > 0 else float("nan")
            if N < MIN_PAIRS[mode] or corners is None:
                history.append((radius, N, rmse, float("nan")))
                return _result(M, t, rmse, N, False, "too few pairs", history)
            dM, dt = solve_plane(N, sums, pivot) if mode == "plane" else solve_point(N, sums, pivot, mode == "similarity")
            at = corners @ M.T + t
            step = float(np.linalg.norm(at @ dM.T + dt - at, axis=1).max())
            M, t = dM @ M, dM @ t + dt
            history.append((radius, N, rmse, step))
            if step <= tol:
                converged = True
                break
    return _result(M, t, rmse, N, converged, "converged" if converged else reason, history)


def _result(M, t, rmse, N, converged, reason, history):
    return Registration(_matrix(M, t), float(np.cbrt(np.linalg.det(M))), rmse, int(N), len([h for h in history if h[3] == h[3]]),
                        converged, reason, history)


def _valid_box(p):
    ok = np.isfinite(p).all(axis=1)
    return np.stack([p[ok].min(axis=0), p[ok].max(axis=0)]).astype(np.float64) if ok.any() else None


def _check_mode(mode, target_normals):
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    if mode == "plane" and target_normals is None:
        raise ValueError("mode 'plane' needs target_normals")


def register_numpy(source, target, max_dist, mode="rigid", init=None, target_normals=None, iterations=50, tol=None):
    """The definition on host arrays -> Registration; the pairs are nearest_numpy's in float64."""
    _check_mode(mode, target_normals)
    s, p = host_points(source, "source"), host_points(target, "target")
    nrm = _normals(target_normals, len(p), "target_normals") if mode == "plane" else None
    radii = check_radii(max_dist)
    M0, t0 = affine_parts(np.eye(4) if init is None else init)

    def pair_sums(M, t, radius, pivot):
        T = _matrix(M, t)
        _, index = nearest_numpy(transform_numpy(s, T), p, radius)
        return pair_sums_numpy(s, T, index, p, pivot, nrm)

    return _iterate(pair_sums, lambda M, t, radius: None, radii, mode, (M0, t0), iterations, tol, _valid_box(s), _valid_box(p))


def _register_device(source, target, max_dist, mode, init, target_normals, iterations, tol, resort=True):
    """The same loop on GPU tensors: per iteration the records of the moved source, the nearest kernel and the pair sums (three
    calls) and one read of 256 bytes.  The order of the queries decides the speed of the nearest kernel, never its result: a
    query that has left the cell it was sorted by makes its wave visit that cell's neighbourhood as well.  resort=True keys and
    sorts the moved source before every iteration (two launches and torch.sort); False: at the start of every stage only, which
    was 40 % slower on profiles/cloud_register.txt's clouds and gives the same bits."""
    import torch
    from . import ops
    _check_mode(mode, target_normals)
    s = ops.cloud_points(source, "source")
    dev = s.device
    p = ops.cloud_points(target, "target", dev)
    nrm = None
    if mode == "plane":
        nrm = target_normals if is_tensor(target_normals) else torch.from_numpy(np.ascontiguousarray(target_normals, dtype=np.float32)).to(dev)
        nrm = ops.L.as_f32(nrm, "target_normals", (p.shape[0], 3), dev)
    radii = check_radii(max_dist)
    M0, t0 = affine_parts(np.eye(4) if init is None else init)
    source_box, target_box = ops.cloud_extent(s), ops.cloud_extent(p)
    origin = [0.0, 0.0, 0.0] if target_box is None else target_box[0].tolist()
    grid = ops.cloud_grid(p, origin, radii[0] * ops.CLOUD_CELL_MARGIN)
    state = {}

    def sort(M, t):
        moved = ops.cloud_transform(s, _matrix(M, t))
        state["perm"] = ops.cloud_sorted(moved, grid.origin, grid.inv)[1]

    def pair_sums(M, t, radius, pivot):
        T = _matrix(M, t)
        if resort:
            sort(M, t)
        records = ops.cloud_transform_records(s, state["perm"], T)
        _, index = ops.cloud_nearest_records(records, grid, radius)
        return ops.cloud_pair_sums_read(ops.cloud_pair_sums(s, T, index, p, pivot, nrm), mode == "plane")

    begin_stage = (lambda M, t, radius: None) if resort else (lambda M, t, radius: sort(M, t))
    return _iterate(pair_sums, begin_stage, radii, mode, (M0, t0), iterations, tol, source_box, target_box)


def register_clouds(source, target, max_dist, mode="rigid", init=None, target_normals=None, iterations=50, tol=None):
    """Registers source (n,3) onto target (m,3) -> Registration (module docstring).

        reg = register_clouds(pred_points, gt_points, max_dist=(0.04, 0.02, 0.01), mode="rigid")
        aligned = reg.apply(pred_points)

    max_dist: one radius or descending radii (stages); mode: "rigid", "similarity" or "plane" (point to plane: needs target_normals
    (m,3)); init: a (4,4) start (default: the identity); iterations: per stage; tol: on the step (default: definition 5).  Clouds on the
    GPU run the HIP kernels, clouds on the host the numpy specification; a mixed pair raises instead of being moved silently (the
    normals follow the target)."""
    for name, a in (("source", source), ("target", target)):
        if len(getattr(a, "shape", ())) == 2 and a.shape[0] >= 2 ** 31:  # before anything is copied or made contiguous
            raise ValueError(f"{name}: {a.shape[0]} points, supported below 2^31")
    if one_place(source, target, what="source and the target cloud") == "host":
        return register_numpy(source, target, max_dist, mode, init, target_normals, iterations, tol)
    return _register_device(source, target, max_dist, mode, init, target_normals, iterations, tol)

