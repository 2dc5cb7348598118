"""Point-cloud evaluation: score a predicted cloud (DepthFusion's points) against a ground-truth cloud the way the MVSNet family is
judged: DTU's mean accuracy / completeness / overall distance and Tanks and Temples' / ETH3D's precision / recall / F-score at
distance thresholds, on a voxel-thinned prediction.  The reference has no such component (it stops at the per-view depth map); the
definition is this docstring, the numpy functions below (the readable specification and the CPU path) and include/mvd.h.

A point with a non-finite coordinate is INVALID.  All coordinates, max_dist, the thresholds and the voxel are taken as float32.

1. Truncated nearest neighbour.  Queries Q (n,3), targets P (m,3), max_dist > 0:
       dist[i]  = min(max_dist, min over valid j of |Q_i - P_j|)    (max_dist when Q_i is invalid or no valid target exists)
       index[i] = the j that attains the minimum when that minimum is < max_dist (strict), else -1
   |q - p| = sqrt(dx^2 + dy^2 + dz^2) of the coordinate DIFFERENCES, never |q|^2 + |p|^2 - 2 q.p: at coordinates around 10^3 and
   distances around 10^-2 the expansion loses every digit (which is why the matrix cores have nothing to offer here).  Ties:
   among targets whose dx^2 + dy^2 + dz^2, as the device computed it, is equal, the smallest original index wins (nearest_numpy:
   the first minimum).  n = 0 gives empty outputs, m = 0 truncates every query.  No atomic decides a value: two calls give the
   same bits.

2. Scores of a predicted cloud against a ground-truth cloud, thresholds t_1..t_T (T <= 8, each <= max_dist), from
   d_pred = dist(pred -> gt) and d_gt = dist(gt -> pred), each over its VALID queries only:
       accuracy = mean(d_pred)    completeness = mean(d_gt)    overall = (accuracy + completeness) / 2
       precision[t] = share of d_pred < t_t (strict)    recall[t] = share of d_gt < t_t
       fscore[t] = 2 P R / (P + R)   (0 when P + R = 0)
   Means are float64 sums of the float32 distances in a fixed order over int64 counts; a mean or share over no point is NaN.

3. Voxel down-sampling.  Per point i_a = floor((float64(x_a) - o_a) * inv) for a in x, y, z, with inv = 1.0 / float64(voxel) formed
   once on the host and handed to the device as a double: numpy and the device run the same IEEE operations and agree on membership
   bit for bit.  The origin o is the caller's, by default the per-axis minimum over the valid points.  Each index must be in
   [0, 2^21 - 1) (else ValueError: the all-ones key is kept for the invalid points); key = i_x << 42 | i_y << 21 | i_z.  Output: one
   point per occupied voxel in ascending key order, the float64 mean of the voxel's points rounded to float32, colours likewise,
   and the voxel's number of points; invalid points are dropped.

The same keys, with cell edge max_dist * (1 + 2^-10) in place of the voxel, sort both clouds into the uniform grid of the device's
nearest-neighbour search (csrc/cloud_eval.hip: ops.cloud_grid, ops.cloud_nearest, ops.cloud_scores, ops.voxel_downsample).
PointCloudEvaluation picks the host or the device by where its inputs are.
"""
from dataclasses import dataclass

import numpy as np

from .depth_fusion import DepthFusion
from .mesh import is_tensor, one_place, place, to_numpy

MAX_THRESHOLDS = 8
INDEX_LIMIT = (1 << 21) - 1


def host_points(a, name):
    p = np.asarray(to_numpy(a), dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"{name} must be (n,3), got {p.shape}")
    return p


def check_thresholds(thresholds, max_dist):
    """-> (thresholds (T,) float32, max_dist float32), validated; max_dist None = 4 x the largest threshold."""
    th = np.atleast_1d(np.asarray(thresholds, dtype=np.float32))
    if th.ndim != 1 or not 1 <= len(th) <= MAX_THRESHOLDS:
        raise ValueError(f"{th.size} thresholds, supported 1..{MAX_THRESHOLDS}")
    if not (np.isfinite(th).all() and (th > 0).all()):
        raise ValueError(f"thresholds must be finite and > 0, got {th.tolist()}")
    md = np.float32(4.0) * th.max() if max_dist is None else np.float32(max_dist)
    if not (md > 0 and np.isfinite(md)):
        raise ValueError(f"max_dist must be finite and > 0, got {max_dist}")
    if (th > md).any():
        raise ValueError(f"thresholds {th.tolist()} above max_dist {float(md):g}: a distance is truncated there")
    return th, md


def nearest_numpy(query, target, max_dist, dtype=np.float64):
    """Definition 1 as chunked brute force -> (dist (n,) of dtype, index (n,) int32).  dtype=np.float32 evaluates the same chain
    (differences, (dx^2 + dy^2) + dz^2, sqrt) in float32: the gap between the two is what tests/test_hip_cloud_eval.py derives its
    band from.  max_dist=np.inf gives the untruncated distance (inf without a valid target)."""
    ft = np.dtype(dtype).type
    q, p = host_points(query, "query").astype(ft), host_points(target, "target").astype(ft)
    md = ft(np.float32(max_dist))
    if not md > 0:
        raise ValueError(f"max_dist must be > 0, got {max_dist}")
    n, m = len(q), len(p)
    dist, index = np.full(n, md, dtype=ft), np.full(n, -1, dtype=np.int32)
    p_bad = ~np.isfinite(p).all(axis=1)
    q_ok = np.isfinite(q).all(axis=1)
    if n == 0 or m == 0 or p_bad.all():
        return dist, index
    step = max(1, (1 << 22) // m)
    with np.errstate(all="ignore"):
        for b in range(0, n, step):
            d = q[b:b + step, None, :] - p[None, :, :]
            d = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
            d[:, p_bad] = np.inf
            d[~q_ok[b:b + step]] = np.inf
            j = np.argmin(d, axis=1)  # the first minimum: the smallest index among equals
            dm = d[np.arange(len(j)), j]
            found = dm < md
            dist[b:b + step] = np.where(found, dm, md)
            index[b:b + step] = np.where(found, j, -1)
    return dist, index


@dataclass
class CloudScore:
    """accuracy, completeness, overall: floats; precision, recall, fscore: (T,) float64 over the thresholds; n_pred, n_gt: the valid
    points of the evaluated prediction (after thinning) and of the ground truth; dist_pred (n,), dist_gt (m,) float32: the truncated
    distances per point, for colouring an error cloud (GPU tensors on the device path); pred_points, pred_colors: the evaluated
    prediction, i.e. the thinned (and, with align, registered) cloud that dist_pred belongs to; registration: the
    cloud_register.Registration that aligned it, or None; n_removed: the points that clean= took out of the thinned prediction."""
    accuracy: float
    completeness: float
    overall: float
    precision: np.ndarray
    recall: np.ndarray
    fscore: np.ndarray
    n_pred: int
    n_gt: int
    dist_pred: object
    dist_gt: object
    thresholds: np.ndarray
    max_dist: float
    pred_points: object = None
    pred_colors: object = None
    registration: object = None
    n_removed: int = 0


def combine_scores(sum_p, n_p, cnt_p, sum_g, n_g, cnt_g, **fields):
    """Definition 2 from the two directions' float64 sums, valid counts and per-threshold counts."""
    with np.errstate(all="ignore"):
        acc = np.float64(sum_p) / np.float64(n_p)
        comp = np.float64(sum_g) / np.float64(n_g)
        P = np.asarray(cnt_p, dtype=np.float64) / np.float64(n_p)
        R = np.asarray(cnt_g, dtype=np.float64) / np.float64(n_g)
        F = np.where(P + R == 0, 0.0, 2 * P * R / (P + R))
    return CloudScore(float(acc), float(comp), float((acc + comp) / 2), P, R, F, int(n_p), int(n_g), **fields)


def _direction_numpy(q, p, th, md, ft):
    d, _ = nearest_numpy(q, p, md, ft)
    ok = np.isfinite(q).all(axis=1)
    dv = d[ok]
    return d, float(np.sum(dv.astype(np.float64))), int(ok.sum()), np.array([(dv < ft(t)).sum() for t in th], dtype=np.int64)


def cloud_scores_numpy(pred, gt, thresholds, max_dist, dtype=np.float64):
    """Definition 2 -> CloudScore, with the distances of nearest_numpy(dtype=dtype) (dist_pred / dist_gt are returned in float32)."""
    ft = np.dtype(dtype).type
    th, md = check_thresholds(thresholds, max_dist)
    pred, gt = host_points(pred, "pred"), host_points(gt, "gt")
    dp, sp, np_, cp = _direction_numpy(pred, gt, th, md, ft)
    dg, sg, ng, cg = _direction_numpy(gt, pred, th, md, ft)
    return combine_scores(sp, np_, cp, sg, ng, cg, dist_pred=dp.astype(np.float32), dist_gt=dg.astype(np.float32), thresholds=th,
                    max_dist=float(md), pred_points=pred)


def voxel_keys_numpy(points, voxel, origin=None):
    """Definition 3's keys -> (keys (n,) int64 with INT64_MAX for invalid points, origin (3,) float64).  ValueError when an index
    leaves [0, 2^21 - 1)."""
    p = host_points(points, "points")
    voxel = np.float32(voxel)
    if not (voxel > 0 and np.isfinite(voxel)):
        raise ValueError(f"voxel must be finite and > 0, got {voxel}")
    ok = np.isfinite(p).all(axis=1)
    if origin is None:
        origin = p[ok].min(axis=0).astype(np.float64) if ok.any() else np.zeros(3)
    origin = np.asarray(origin, dtype=np.float64).reshape(-1)
    if origin.shape != (3,) or not np.isfinite(origin).all():
        raise ValueError(f"origin must be 3 finite numbers, got {origin.tolist()}")
    inv = 1.0 / np.float64(voxel)
    keys = np.full(len(p), np.iinfo(np.int64).max, dtype=np.int64)
    if ok.any():
        idx = np.floor((p[ok].astype(np.float64) - origin) * inv)
        if idx.min() < 0 or idx.max() >= INDEX_LIMIT:
            raise ValueError(f"voxel_downsample: the points span {p[ok].min(axis=0).tolist()} .. {p[ok].max(axis=0).tolist()} from origin "
                             f"{origin.tolist()}, which at an edge of {float(voxel):g} gives indices {idx.min():.0f} .. {idx.max():.0f}; "
                             f"each must be in [0, {INDEX_LIMIT})")
        idx = idx.astype(np.int64)
        keys[ok] = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    return keys, origin


def voxel_downsample_numpy(points, voxel, colors=None, origin=None):
    """Definition 3 -> (xyz (k,3) float32, rgb (k,3) float32 or None, counts (k,) int32), voxels in ascending key order."""
    p = host_points(points, "points")
    col = None
    if colors is not None:
        col = np.asarray(to_numpy(colors), dtype=np.float32)
        if col.shape != p.shape:
            raise ValueError(f"colors: shape {col.shape}, expected {p.shape}")
    keys, _ = voxel_keys_numpy(p, voxel, origin)
    order = np.argsort(keys, kind="stable")
    order = order[:int((keys != np.iinfo(np.int64).max).sum())]
    if len(order) == 0:
        return np.zeros((0, 3), np.float32), None if col is None else np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
    sk = keys[order]
    heads = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    counts = np.diff(np.concatenate([heads, [len(sk)]]))
    mean = lambda a: (np.add.reduceat(a[order].astype(np.float64), heads, axis=0) / counts[:, None]).astype(np.float32)
    return mean(p), None if col is None else mean(col), counts.astype(np.int32)


class PointCloudEvaluation:
    """Scores a predicted point cloud against a ground-truth cloud (module docstring).

        evaluation = PointCloudEvaluation(thresholds=(0.005, 0.01), voxel=0.002)     # or create_evaluation("cloud", ...)
        score = evaluation(out.points, gt_points, out.colors)                       # out = DepthFusion(...).reconstruct(...)
        score.fscore, score.accuracy, score.dist_pred

    max_dist defaults to 4 x the largest threshold.  With voxel, the prediction is thinned first (its colours with it).
    align = "rigid", "similarity" or "plane": the thinned prediction is registered onto the ground truth first
    (cloud_register.register_clouds, at the radii align_max_dist, by default (4, 2, 1) x max_dist; "plane" needs gt_normals (m,3), given
    here or per call) and the ALIGNED prediction is scored; the score's `registration` tells how it went.
    gt_normals="estimate": the ground truth's normals are estimated (cloud_clean.estimate_normals) from its neighbours within
    normal_radius, by default 4 x the largest threshold: a scan read without normals can serve align="plane".
    clean=dict(...): cloud_clean.remove_outliers' keywords; the prediction is filtered after the thinning and before registration and
    scoring, and the score's n_removed tells how many points that took."""

    def __init__(self, thresholds, max_dist=None, voxel=None, align=None, align_max_dist=None, gt_normals=None, clean=None,
                 normal_radius=None):
        self.thresholds, self.max_dist = check_thresholds(thresholds, max_dist)
        if voxel is not None and not (np.float32(voxel) > 0 and np.isfinite(np.float32(voxel))):
            raise ValueError(f"voxel must be finite and > 0, got {voxel}")
        self.voxel = None if voxel is None else float(np.float32(voxel))
        self.align, self.align_max_dist, self.gt_normals = align, None, gt_normals
        if align is not None:
            from .cloud_register import MODES, check_radii
            if align not in MODES:
                raise ValueError(f"align must be None or one of {MODES}, got {align!r}")
            self.align_max_dist = check_radii([4.0 * self.max_dist, 2.0 * self.max_dist, self.max_dist] if align_max_dist is None
                                         else align_max_dist)
        elif align_max_dist is not None or gt_normals is not None:
            raise ValueError("align_max_dist and gt_normals belong to align=...")
        if isinstance(gt_normals, str) and gt_normals != "estimate":
            raise ValueError(f"gt_normals must be (m,3) normals or 'estimate', got {gt_normals!r}")
        if normal_radius is not None and not (isinstance(gt_normals, str) and np.float32(normal_radius) > 0
                                              and np.isfinite(np.float32(normal_radius))):
            raise ValueError(f"normal_radius must be finite and > 0 and belongs to gt_normals='estimate', got {normal_radius}")
        self.normal_radius = float(np.float32(4.0) * self.thresholds.max() if normal_radius is None else np.float32(normal_radius))
        self.clean = None
        if clean is not None:
            from .cloud_clean import _outlier_rule
            self.clean = dict(clean)
            unknown = sorted(set(self.clean) - {"radius", "min_neighbours", "k", "std_ratio", "max_dist"})
            if unknown:
                raise ValueError(f"clean: unexpected {unknown}")
            _outlier_rule(*[self.clean.get(a) for a in ("radius", "min_neighbours", "k", "std_ratio", "max_dist")])

    def _clean(self, pred, colors):
        """-> (the filtered prediction, its colours, the points removed), or the inputs and 0 without clean"""
        if self.clean is None:
            return pred, colors, 0
        from .cloud_clean import remove_outliers
        out = remove_outliers(pred, colors, **self.clean)
        return out.points, out.colors, int(pred.shape[0] - out.points.shape[0])

    def _register(self, pred, gt, gt_normals):
        """-> (the aligned prediction, the Registration), or (pred, None) without align"""
        if self.align is None:
            if gt_normals is not None:
                raise ValueError("gt_normals belong to align=...")
            return pred, None
        from .cloud_register import register_clouds
        normals = self.gt_normals if gt_normals is None else gt_normals
        if self.align == "plane" and normals is None:
            raise ValueError("align='plane' needs gt_normals")
        if isinstance(normals, str):  # "estimate": only the plane mode reads them
            normals = None
            if self.align == "plane":
                from .cloud_clean import estimate_normals
                normals, _ = estimate_normals(gt, radius=self.normal_radius)
        if normals is not None and place(normals) != place(gt):
            if place(gt) == "host":
                normals = to_numpy(normals)
            else:
                import torch
                normals = torch.as_tensor(to_numpy(normals), dtype=torch.float32).to(gt.device)
        reg = register_clouds(pred, gt, self.align_max_dist, mode=self.align, target_normals=normals if self.align == "plane" else None)
        return reg.apply(pred), reg

    def __call__(self, pred_points, gt_points, pred_colors=None, gt_normals=None):
        """pred_points (n,3), gt_points (m,3), pred_colors (n,3) or None: numpy arrays or torch tensors.  Clouds on the GPU run the HIP
        kernels and the result's dist_pred / dist_gt / pred_points are GPU tensors; clouds on the host run the numpy specification.
        Both clouds must be in the same place: a mixed pair raises instead of being moved silently (colours follow the points)."""
        host = one_place(pred_points, gt_points, what="predicted and the ground-truth cloud") == "host"
        return (self._run_host if host else self._run_device)(pred_points, gt_points, pred_colors, gt_normals)

    def _run_host(self, pred, gt, colors, gt_normals=None):
        pred, gt = host_points(pred, "pred_points"), host_points(gt, "gt_points")
        if self.voxel is not None:
            pred, colors, _ = voxel_downsample_numpy(pred, self.voxel, colors)
        pred, colors, removed = self._clean(pred, colors)
        pred, reg = self._register(pred, gt, gt_normals)
        score = cloud_scores_numpy(pred, gt, self.thresholds, self.max_dist)
        score.pred_colors, score.registration, score.n_removed = colors, reg, removed
        return score

    def _run_device(self, pred, gt, colors, gt_normals=None):
        import torch
        from . import ops
        dev = pred.device
        for name, a in (("pred_points", pred), ("gt_points", gt)):
            if a.dim() != 2 or a.shape[1] != 3:
                raise ValueError(f"{name} must be (n,3), got {tuple(a.shape)}")
        if colors is not None:
            colors = colors.to(dev) if is_tensor(colors) else torch.from_numpy(np.ascontiguousarray(colors, dtype=np.float32)).to(dev)
        if self.voxel is not None:
            pred, colors, _ = ops.voxel_downsample(pred, self.voxel, colors)
        pred, gt = ops.cloud_points(pred, "pred_points"), ops.cloud_points(gt, "gt_points", dev)
        pred, colors, removed = self._clean(pred, colors)
        pred, reg = self._register(pred, gt, gt_normals)
        md, T = float(self.max_dist), len(self.thresholds)
        cell = md * ops.CLOUD_CELL_MARGIN
        # one grid for both clouds: each is sorted once and serves as the queries of one direction and the targets of the other
        extents = [e for e in (ops.cloud_extent(pred), ops.cloud_extent(gt)) if e is not None]
        origin = np.min([e[0] for e in extents], axis=0).tolist() if extents else [0.0, 0.0, 0.0]
        gp, gg = ops.cloud_grid(pred, origin, cell), ops.cloud_grid(gt, origin, cell)
        th = torch.from_numpy(self.thresholds).to(dev)
        dp, ip = ops.cloud_nearest(gp, gg, md)
        dg, ig = ops.cloud_nearest(gg, gp, md)
        blocks = torch.empty((2, 10), dtype=torch.int64, device=dev)
        ops.cloud_scores(dp, ip, th, pred, result=blocks[0])
        ops.cloud_scores(dg, ig, th, gt, result=blocks[1])
        blocks = blocks.cpu()  # the one read of the evaluation
        sp, np_, cp = ops.cloud_scores_read(blocks[0], T)
        sg, ng, cg = ops.cloud_scores_read(blocks[1], T)
        return combine_scores(sp, np_, cp, sg, ng, cg, dist_pred=dp, dist_gt=dg, thresholds=self.thresholds, max_dist=md, pred_points=pred,
                        pred_colors=colors, registration=reg, n_removed=removed)


def evaluate_scene(model, images, intrinsics, poses, gt_points, fusion=None, num_sources=None, evaluation=None, gt_normals=None,
                   **evaluation_args):
    """model -> depth maps -> fused cloud -> CloudScore: DepthFusion.reconstruct chained into PointCloudEvaluation, so that a registered
    model reaches the fusion and the scoring kernels end to end.  images, intrinsics, poses, num_sources: reconstruct's; fusion: a
    DepthFusion (default DepthFusion()); evaluation: a PointCloudEvaluation, or its arguments as keywords (thresholds=..., voxel=...,
    align=..., align_max_dist=..., clean=...); gt_normals: the ground truth's normals for align="plane", or "estimate".
    The scene is fused where reconstruct puts it (the model's GPU; a ground truth that is a GPU tensor asks for its device) and the
    ground truth is taken there."""
    if evaluation is None:
        if "thresholds" not in evaluation_args:
            raise ValueError("evaluate_scene needs evaluation=PointCloudEvaluation(...) or thresholds=...")
        evaluation = PointCloudEvaluation(**evaluation_args)
    elif evaluation_args:
        raise ValueError(f"evaluation is given: unexpected {sorted(evaluation_args)}")
    fusion = DepthFusion() if fusion is None else fusion
    device = gt_points.device if place(gt_points) != "host" else None
    out = fusion.reconstruct(model, images, intrinsics, poses, num_sources=num_sources, device=device)
    if place(out.points) == "host":
        gt_points = to_numpy(gt_points)
    elif place(gt_points) != place(out.points):
        import torch
        gt_points = torch.as_tensor(to_numpy(gt_points), dtype=torch.float32).to(out.points.device)
    return evaluation(out.points, gt_points, out.colors, gt_normals=gt_normals)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path, normals=False, faces=False):
    """-> (points (n,3) float32, colors (n,3) float32 in 0..255 or None): the counterpart of depth_fusion.write_ply.  Reads ASCII and
    binary little-endian files whose first element is `vertex`; x / y / z may be float or double; uchar red / green / blue are the
    colours when all three are there; other scalar vertex properties and later elements (faces) are skipped.
    normals=True -> (points, colors, normals (n,3) float32 or None): nx / ny / nz, float or double, when all three are there.
    faces=True appends faces (T,3) int32 or None to the result: the second element where it is `face` with the one property
    `list <count type> <index type> vertex_indices` (or vertex_index), every face a triangle."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, count, props, elements, face_count, face_list = None, None, [], 0, None, None
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            w = line.decode("ascii", errors="replace").split()
            if not w or w[0] in ("comment", "obj_info"):
                continue
            if w[0] == "end_header":
                break
            if w[0] == "format":
                fmt = w[1]
            elif w[0] == "element":
                elements += 1
                if elements == 1:
                    if w[1] != "vertex":
                        raise ValueError(f"{path}: the first element is {w[1]!r}, expected 'vertex'")
                    count = int(w[2])
                elif elements == 2 and w[1] == "face":
                    face_count = int(w[2])
            elif w[0] == "property" and elements == 2 and face_count is not None:
                if face_list is not None or len(w) != 5 or w[1] != "list" or w[2] not in _PLY_TYPES or w[3] not in _PLY_TYPES:
                    face_list = ()  # not the one list property: no faces to read
                else:
                    face_list = (_PLY_TYPES[w[2]], _PLY_TYPES[w[3]])
            elif w[0] == "property" and elements == 1:
                if w[1] == "list" or w[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: unsupported vertex property {' '.join(w[1:])!r}")
                props.append((w[2], _PLY_TYPES[w[1]]))
        if fmt not in ("ascii", "binary_little_endian") or count is None:
            raise ValueError(f"{path}: format {fmt!r} (supported: ascii, binary_little_endian) or no vertex element")
        names = [n for n, _ in props]
        if len(set(names)) != len(names) or not all(a in names for a in "xyz"):
            raise ValueError(f"{path}: vertex properties {names} must hold x, y, z once each")
        want_faces = faces and bool(face_list)
        tri = None
        if fmt == "ascii":
            lines = [ln for ln in f.read().decode("ascii", errors="replace").splitlines() if ln.strip()]
            rows = np.loadtxt(lines[:count], dtype=np.float64, ndmin=2) if count else np.zeros((0, len(props)))
            if want_faces:
                tri = np.loadtxt(lines[count:count + face_count], dtype=np.int64, ndmin=2) if face_count else np.zeros((0, 4), np.int64)
                if tri.shape != (face_count, 4) or (tri[:, 0] != 3).any():
                    raise ValueError(f"{path}: expected {face_count} triangles")
                tri = tri[:, 1:].astype(np.int32)
            if rows.shape != (count, len(props)):
                raise ValueError(f"{path}: expected {count} vertices of {len(props)} values, got {rows.shape}")
            column = lambda name: rows[:, names.index(name)]
        else:
            dt = np.dtype([(n, "<" + t) for n, t in props])
            rec = np.frombuffer(f.read(count * dt.itemsize), dtype=dt)
            if len(rec) != count:
                raise ValueError(f"{path}: {len(rec)} of {count} vertices")
            column = lambda name: rec[name]
            if want_faces:
                ft = np.dtype([("n", "<" + face_list[0]), ("v", "<" + face_list[1], (3,))])
                frec = np.frombuffer(f.read(face_count * ft.itemsize), dtype=ft)
                if len(frec) != face_count or (frec["n"] != 3).any():
                    raise ValueError(f"{path}: expected {face_count} triangles")
                tri = frec["v"].astype(np.int32)
    points = np.stack([column(a) for a in "xyz"], axis=1).astype(np.float32)
    colors = None
    if all(c in names and dict(props)[c] == "u1" for c in ("red", "green", "blue")):
        colors = np.stack([column(c) for c in ("red", "green", "blue")], axis=1).astype(np.float32)
    out = (points, colors)
    if normals:
        have = all(c in names and dict(props)[c] in ("f4", "f8") for c in ("nx", "ny", "nz"))
        out += (np.stack([column(c) for c in ("nx", "ny", "nz")], axis=1).astype(np.float32) if have else None,)
    return out + (tri,) if faces else out
