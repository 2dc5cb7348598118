"""Multi-view depth fusion: cross-check the depth maps of several views against each other and turn the pixels on which enough
views agree into one 3-D point set, along the lines of MVSNet's depth filtering and fusion.  The reference has no such component;
the definition is this docstring, fuse_numpy (the readable specification and the CPU path) and include/mvd.h.

For a key view (depth d (H,W), intrinsics Kk, world-to-view pose Tk) and V <= 32 source views of the same size the host composes,
in float64, per source
    A  = Ks R  Kk^-1,  b  = Ks t     with [R |t ] = Ts Tk^-1      (key pixel and depth -> source pixel)
    A' = Kk R' Ks^-1,  b' = Kk t'    with [R'|t'] = Tk Ts^-1      (source pixel and depth -> key pixel)
and for key pixel (x, y) and source s:
  1. Q = d A (x,y,1) + b, (u,v) = (Qx/Qz, Qy/Qz); valid when d is finite and > 0, Qz > 0, 0 <= u <= W-1 and 0 <= v <= H-1.
  2. ds = the bilinear blend of the source depth in the cell x0 = min(floor(u), W-2), y0 = min(floor(v), H-2) with weights u-x0 and
     v-y0; invalid when one of the four taps is not finite or <= 0.
  3. Q' = ds A' (u,v,1) + b', (x',y') = (Q'x/Q'z, Q'y/Q'z), d' = Q'z, err = hypot(x'-x, y'-y), rel = |d'-d| / d.
  4. consistent = valid and err < max_reproj_error and rel < max_rel_depth_diff (both strict).
view_bits has bit s set where source s is consistent, count = popcount(view_bits), fused = (d + sum of the consistent d') /
(count + 1) (0 where d is invalid), mask = count >= min_consistent_views (default min(3, V)) and, when an uncertainty map and
max_uncertainty are given, uncertainty <= max_uncertainty (false for a NaN).  The uncertainty filters the key pixel only.

The point cloud is the masked pixels in row-major (np.nonzero) order, X = Tk^-1 (fused Kk^-1 (x,y,1)), with the pixel's colour.

Normals (normals=True; normals_numpy).  With B the 3x3 of compose_backprojection, P(x,y) = depth(x,y) B (x,y,1): the world point
without the camera centre c, which cancels in the differences below and would only cost digits at world coordinates far from the
origin.  n = (P(x+1,y) - P(x-1,y)) x (P(x,y+1) - P(x,y-1)), normalised, and negated when n . B (x,y,1) > 0, so that it points towards
the camera.  The normal is (0,0,0), which means invalid, on the image border, where one of the five depths is not finite or <= 0, and
where the cross product's length is zero or not finite.  There is no depth-discontinuity guard: a stencil that straddles an edge gives
a normal of neither surface; the consistency mask removes most of those pixels.

Merge mode (merge=True; merge_numpy): one point per surface sample instead of one per view that sees it, fusibile-style.  Every view i
has a byte map claimed[i], all zero at the start, and the views are processed in index order.  For view i, view_bits, count and fused
are fuse_numpy's, unchanged; mask = fuse_numpy's mask and not claimed[i], with claimed[i] as it is before view i runs.  For every
pixel with mask set and every consistent source s, which is view j, the target is the source pixel (tx, ty) = (rint(u), rint(v)),
half to even: it is one of the four bilinear taps, so it is inside the image and has a valid depth.  claimed[j][ty,tx] is set; the
pixel and its targets are the members of the merged point.  merged_rgb = (the pixel's colour + the targets' colours in source order)
/ (count + 1); merged_normal = the normalised sum of the members' normals (an invalid one is zero and adds nothing), (0,0,0) when no
member has a valid normal or the sum has zero length.  Both are 0 where mask is 0.  A later view still uses a claimed pixel's depth
for its consistency checks and its means: only the emission is suppressed.  A view among its own sources is refused, because
claimed[i] must not change while view i runs.  THE RESULT DEPENDS ON THE ORDER OF THE VIEWS, by design: the first view that sees a
surface sample emits it, at its own pixel.  normals=True without merge gives each point its key view's own normal.

Two implementations: fuse_numpy / points_numpy / normals_numpy / merge_numpy on the host, and the HIP kernels of csrc/depth_fusion.hip
(ops.geo_consistency, ops.compact_points, ops.depth_normals, ops.geo_merge) for maps that are GPU tensors.  DepthFusion picks by where
its inputs are.
"""
from dataclasses import dataclass

import numpy as np

from .mesh import is_tensor, one_place, to_numpy

MAX_SOURCES = 32


def _inv_pose(T):
    R, t = T[:3, :3], T[:3, 3]
    out = np.eye(4)
    out[:3, :3] = R.T
    out[:3, 3] = -R.T @ t
    return out


def pinhole(K, name):
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3) or K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1 or K[0, 0] == 0 or K[1, 1] == 0:
        raise ValueError(f"{name}: expected pinhole intrinsics [[fx, s, cx], [0, fy, cy], [0, 0, 1]], got {K.tolist()}")
    return K


def _pinhole_inv(K):
    fx, s, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    return np.array([[1 / fx, -s / (fx * fy), (s * cy / fy - cx) / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]])


def _pinhole_ratio(Ka, Kb):
    """Ka Kb^-1 in closed form: exactly the identity for Ka == Kb."""
    a = Ka[0, 0] / Kb[0, 0]
    e = Ka[1, 1] / Kb[1, 1]
    b = (Ka[0, 1] - a * Kb[0, 1]) / Kb[1, 1]
    return np.array([[a, b, Ka[0, 2] - a * Kb[0, 2] - b * Kb[1, 2]], [0, e, Ka[1, 2] - e * Kb[1, 2]], [0, 0, 1]])


def _project_into(Ka, Ta, Kb, Tb):
    """(A, b) that take a pixel of view b and its depth to view a: A = Ka R Kb^-1, b = Ka t with [R|t] = Ta Tb^-1.  Formed around
    the identity, R = I + (Ra - Rb) Rb^T and t = (ta - tb) - (Ra - Rb) Rb^T tb, so that a view with b's own intrinsics and pose
    gives A = I and b = 0 exactly: a pixel on the image border then stays on it instead of leaving by one rounding."""
    dR = (Ta[:3, :3] - Tb[:3, :3]) @ Tb[:3, :3].T
    t = (Ta[:3, 3] - Tb[:3, 3]) - dR @ Tb[:3, 3]
    return _pinhole_ratio(Ka, Kb) + Ka @ dR @ _pinhole_inv(Kb), Ka @ t


def compose_matrices(key_K, key_T, src_Ks, src_Ts):
    """-> (V,24) float64: per source A (9, row-major), b (3), A' (9), b' (3).  The device takes them rounded to float32."""
    Kk, Tk = pinhole(key_K, "key intrinsics"), np.asarray(key_T, dtype=np.float64)
    rows = []
    for i, (Ks, Ts) in enumerate(zip(src_Ks, src_Ts)):
        Ks, Ts = pinhole(Ks, f"source intrinsics {i}"), np.asarray(Ts, dtype=np.float64)
        A, b = _project_into(Ks, Ts, Kk, Tk)
        A2, b2 = _project_into(Kk, Tk, Ks, Ts)
        rows.append(np.concatenate([A.ravel(), b, A2.ravel(), b2]))
    return np.stack(rows)


def compose_backprojection(key_K, key_T):
    """-> 12 float64: B = Rk^T Kk^-1 (9, row-major) and c = -Rk^T tk, so that X = depth * B (x,y,1) + c."""
    Tk_inv = _inv_pose(np.asarray(key_T, dtype=np.float64))
    return np.concatenate([(Tk_inv[:3, :3] @ _pinhole_inv(pinhole(key_K, "key intrinsics"))).ravel(), Tk_inv[:3, 3]])


def _check_views(depth, src_depths):
    if depth.ndim != 2 or depth.shape[0] < 2 or depth.shape[1] < 2:
        raise ValueError(f"key depth must be (H,W) with H, W >= 2, got {depth.shape}")
    if not 1 <= len(src_depths) <= MAX_SOURCES:
        raise ValueError(f"{len(src_depths)} source views, supported 1..{MAX_SOURCES}")
    for i, s in enumerate(src_depths):
        if s.shape != depth.shape:
            raise ValueError(f"source depth {i}: shape {s.shape}, expected the key's {depth.shape}")


def fuse_numpy(key_depth, key_K, key_T, src_depths, src_Ks, src_Ts, uncertainty=None, min_consistent_views=None,
               max_reproj_error=1.0, max_rel_depth_diff=0.01, max_uncertainty=None, dtype=np.float64, details=False):
    """The definition of the module docstring as a numpy chain -> dict(view_bits uint32, count uint8, fused, mask uint8), each (H,W).
    dtype=np.float32 evaluates the same chain in float32 on the float32-rounded matrices (what the device is handed): the gap between
    the two is what tests/test_hip_depth_fusion.py derives its bands from.  details=True adds valid, u, v, err, rel, dprime, each (V,H,W)."""
    ft = np.dtype(dtype).type
    d = np.asarray(key_depth).astype(ft)
    srcs = [np.asarray(s).astype(ft) for s in src_depths]
    _check_views(d, srcs)
    H, W = d.shape
    V = len(srcs)
    mats = compose_matrices(key_K, key_T, src_Ks, src_Ts)
    if ft is np.float32:
        mats = mats.astype(np.float32)
    y, x = np.meshgrid(np.arange(H, dtype=ft), np.arange(W, dtype=ft), indexing="ij")
    d_ok = np.isfinite(d) & (d > 0)
    bits = np.zeros((H, W), dtype=np.uint32)
    count = np.zeros((H, W), dtype=np.uint8)
    total = d.copy()
    det = {k: np.zeros((V, H, W), dtype=bool if k == "valid" else ft) for k in ("valid", "u", "v", "err", "rel", "dprime")}
    with np.errstate(all="ignore"):
        for s, (m, src) in enumerate(zip(mats, srcs)):
            A, b, A2, b2 = m[:9].reshape(3, 3), m[9:12], m[12:21].reshape(3, 3), m[21:24]
            q = [d * (A[i, 0] * x + A[i, 1] * y + A[i, 2]) + b[i] for i in range(3)]
            u, v = q[0] / q[2], q[1] / q[2]
            valid = d_ok & (q[2] > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
            x0 = np.where(valid, np.minimum(np.floor(u), W - 2), 0).astype(np.int64)
            y0 = np.where(valid, np.minimum(np.floor(v), H - 2), 0).astype(np.int64)
            fx, fy = u - x0.astype(ft), v - y0.astype(ft)
            t00, t01, t10, t11 = src[y0, x0], src[y0, x0 + 1], src[y0 + 1, x0], src[y0 + 1, x0 + 1]
            for t in (t00, t01, t10, t11):
                valid &= np.isfinite(t) & (t > 0)
            one = ft(1)
            ds = (one - fx) * (one - fy) * t00 + fx * (one - fy) * t01 + (one - fx) * fy * t10 + fx * fy * t11
            q2 = [ds * (A2[i, 0] * u + A2[i, 1] * v + A2[i, 2]) + b2[i] for i in range(3)]
            dprime = q2[2]
            err = np.hypot(q2[0] / dprime - x, q2[1] / dprime - y)
            rel = np.abs(dprime - d) / d
            ok = valid & (err < ft(max_reproj_error)) & (rel < ft(max_rel_depth_diff))
            bits |= ok.astype(np.uint32) << np.uint32(s)
            count += ok
            total = total + np.where(ok, dprime, ft(0))
            if details:
                det["valid"][s], det["u"][s], det["v"][s] = valid, u, v
                det["err"][s], det["rel"][s], det["dprime"][s] = err, rel, dprime
        fused = np.where(d_ok, total / (count.astype(ft) + ft(1)), ft(0))
        min_views = min(3, V) if min_consistent_views is None else int(min_consistent_views)
        mask = count >= min_views
        if uncertainty is not None and max_uncertainty is not None:
            unc = np.asarray(uncertainty).astype(ft)
            if unc.shape != d.shape:
                raise ValueError(f"uncertainty: shape {unc.shape}, expected {d.shape}")
            mask &= unc <= ft(max_uncertainty)
    out = {"view_bits": bits, "count": count, "fused": fused, "mask": mask.astype(np.uint8)}
    if details:
        out.update(det)
    return out


def points_numpy(mask, fused, key_K, key_T, image=None):
    """The masked pixels in np.nonzero order -> (xyz (M,3) float64, rgb (M,3) or None); image: planar (3,H,W)."""
    bp = compose_backprojection(key_K, key_T)
    ys, xs = np.nonzero(mask)
    ray = bp[:9].reshape(3, 3) @ np.stack([xs, ys, np.ones_like(xs)]).astype(np.float64)
    xyz = (np.asarray(fused, dtype=np.float64)[ys, xs] * ray).T + bp[9:]
    rgb = np.asarray(image)[:, ys, xs].T if image is not None else None
    return xyz, rgb


def normals_numpy(depth, K, T, dtype=np.float64):
    """World-frame normals (3,H,W) of one depth map, the module docstring's definition as a numpy chain; (0,0,0) where invalid.
    dtype=np.float32 evaluates the same chain in float32 on the float32-rounded B, as fuse_numpy does for its chain."""
    ft = np.dtype(dtype).type
    d = np.asarray(depth).astype(ft)
    if d.ndim != 2:
        raise ValueError(f"depth must be (H,W), got {d.shape}")
    H, W = d.shape
    out = np.zeros((3, H, W), dtype=ft)
    if H < 3 or W < 3:
        return out
    B = compose_backprojection(K, T)[:9].reshape(3, 3).astype(ft)
    y, x = np.meshgrid(np.arange(1, H - 1, dtype=ft), np.arange(1, W - 1, dtype=ft), indexing="ij")
    ray = lambda x, y: [B[i, 0] * x + B[i, 1] * y + B[i, 2] for i in range(3)]
    one = ft(1)
    dc, dl, dr, du, dd = d[1:-1, 1:-1], d[1:-1, :-2], d[1:-1, 2:], d[:-2, 1:-1], d[2:, 1:-1]
    with np.errstate(all="ignore"):
        rc, rl, rr, ru, rd = ray(x, y), ray(x - one, y), ray(x + one, y), ray(x, y - one), ray(x, y + one)
        a = [dr * rr[i] - dl * rl[i] for i in range(3)]
        b = [dd * rd[i] - du * ru[i] for i in range(3)]
        n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        length = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        ok = np.isfinite(length) & (length > 0)
        for t in (dc, dl, dr, du, dd):
            ok &= np.isfinite(t) & (t > 0)
        towards = n[0] * rc[0] + n[1] * rc[1] + n[2] * rc[2]
        scale = np.where(towards > 0, -length, length)
        for i in range(3):
            out[i, 1:-1, 1:-1] = np.where(ok, n[i] / scale, ft(0))
    return out


def default_sources(N):
    return [[j for j in range(N) if j != i] for i in range(N)]


def merge_numpy(depths, Ks, Ts, sources=None, uncertainties=None, images=None, normals=False, min_consistent_views=None,
                max_reproj_error=1.0, max_rel_depth_diff=0.01, max_uncertainty=None, dtype=np.float64, details=False):
    """Merge mode for a whole scene, the module docstring's definition as a numpy chain; the result depends on the order of the views.
    depths N x (H,W); sources: per view the indices of its source views (default: all others); images N x (3,H,W) or None.
    -> dict of lists of N maps: view_bits, count, fused (fuse_numpy's), mask (uint8, the claimed pixels taken out), merged_rgb
    (3,H,W) or None without images, merged_normal (3,H,W) or None without normals, normals (every view's normals_numpy, or None) and
    claimed (uint8, after the last view).  details=True adds claimed_before: claimed[i] as it was when view i ran."""
    ft = np.dtype(dtype).type
    N = len(depths)
    sources = default_sources(N) if sources is None else [list(s) for s in sources]
    for i, src in enumerate(sources):
        if i in src:
            raise ValueError(f"view {i} is among its own sources {src}: merge mode reads claimed[{i}] while it writes its sources' maps")
    depths = [np.asarray(d) for d in depths]
    imgs = None if images is None else [np.asarray(im).astype(ft) for im in images]
    nrm = [normals_numpy(depths[i], Ks[i], Ts[i], dtype) for i in range(N)] if normals else None
    claimed = [np.zeros(d.shape, dtype=np.uint8) for d in depths]
    out = {k: [] for k in ("view_bits", "count", "fused", "mask", "merged_rgb", "merged_normal", "claimed_before")}
    for i, src in enumerate(sources):
        r = fuse_numpy(depths[i], Ks[i], Ts[i], [depths[j] for j in src], [Ks[j] for j in src], [Ts[j] for j in src],
                       None if uncertainties is None else uncertainties[i], min_consistent_views, max_reproj_error, max_rel_depth_diff,
                       max_uncertainty, dtype=dtype, details=True)
        out["claimed_before"].append(claimed[i].copy())
        mask = r["mask"] & (claimed[i] == 0)
        ys, xs = np.nonzero(mask)
        rgb = nsum = None
        if imgs is not None:
            rgb = np.zeros((3,) + mask.shape, dtype=ft)
            rgb[:, ys, xs] = imgs[i][:, ys, xs]
        if nrm is not None:
            nsum = np.zeros((3,) + mask.shape, dtype=ft)
            nsum[:, ys, xs] = nrm[i][:, ys, xs]
        for s, j in enumerate(src):
            member = ((r["view_bits"][ys, xs] >> np.uint32(s)) & np.uint32(1)).astype(bool)
            py, px = ys[member], xs[member]
            tx, ty = np.rint(r["u"][s][py, px]).astype(np.int64), np.rint(r["v"][s][py, px]).astype(np.int64)
            claimed[j][ty, tx] = 1
            if rgb is not None:
                rgb[:, py, px] += imgs[j][:, ty, tx]  # the (py, px) are distinct pixels: a plain indexed sum
            if nsum is not None:
                nsum[:, py, px] += nrm[j][:, ty, tx]
        if rgb is not None:
            rgb[:, ys, xs] /= r["count"][ys, xs].astype(ft) + ft(1)
        if nsum is not None:
            with np.errstate(all="ignore"):
                length = np.sqrt(nsum[0] * nsum[0] + nsum[1] * nsum[1] + nsum[2] * nsum[2])
                nsum = np.where(np.isfinite(length) & (length > 0), nsum / length, ft(0))
        for k, v in (("view_bits", r["view_bits"]), ("count", r["count"]), ("fused", r["fused"]), ("mask", mask.astype(np.uint8)),
                     ("merged_rgb", rgb), ("merged_normal", nsum)):
            out[k].append(v)
    out["claimed"], out["normals"] = claimed, nrm
    if imgs is None:
        out["merged_rgb"] = None
    if nrm is None:
        out["merged_normal"] = None
    if not details:
        del out["claimed_before"]
    return out


def write_ply(path, points, colors=None, normals=None, faces=None):
    """Binary little-endian PLY: float32 x y z, with normals float32 nx ny nz, and with colors uchar red green blue.  colors: (M,3)
    in 0..255 (rounded and clipped).  faces: (T,3) vertex indices (a Mesh's triangles), written as `element face` with
    `property list uchar int vertex_indices`."""
    pts = np.asarray(to_numpy(points), dtype="<f4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        nrm = np.asarray(to_numpy(normals), dtype="<f4").reshape(-1, 3)
        if len(nrm) != len(pts):
            raise ValueError(f"{len(nrm)} normals for {len(pts)} points")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        col = np.clip(np.rint(np.asarray(to_numpy(colors), dtype=np.float64).reshape(-1, 3)), 0, 255).astype(np.uint8)
        if len(col) != len(pts):
            raise ValueError(f"{len(col)} colours for {len(pts)} points")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.empty(len(pts), dtype=fields)
    rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if normals is not None:
        rec["nx"], rec["ny"], rec["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if colors is not None:
        rec["red"], rec["green"], rec["blue"] = col[:, 0], col[:, 1], col[:, 2]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(pts)}", "property float x", "property float y",
              "property float z"]
    if normals is not None:
        header += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    if faces is not None:
        tri = np.asarray(to_numpy(faces)).reshape(-1, 3)
        if len(tri) and (tri.min() < 0 or tri.max() >= len(pts)):
            raise ValueError(f"faces index outside the {len(pts)} points")
        frec = np.empty(len(tri), dtype=[("n", "u1"), ("v", "<i4", (3,))])
        frec["n"], frec["v"] = 3, tri
        header += [f"element face {len(tri)}", "property list uchar int vertex_indices"]
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rec.tobytes())
        if faces is not None:
            f.write(frec.tobytes())


def map2d(a, name):
    """One (H,W) map from (H,W), (1,H,W) or (1,1,H,W), numpy or torch."""
    if a.ndim < 2 or int(np.prod(a.shape[:-2])) != 1:
        raise ValueError(f"{name}: expected one (H,W) map, got {tuple(a.shape)}")
    return a.reshape(a.shape[-2], a.shape[-1])


@dataclass
class FusionResult:
    """Per view (lists of N maps, GPU tensors on the device path): mask uint8, fused_depth, num_consistent uint8, view_bits uint32
    (bit j of view i = the j-th entry of sources[i] is consistent).  Concatenated in view order: points (M,3) float32, colors (M,3)
    or None, view_index (M,) int64.  normals (M,3) float32 unit vectors ((0,0,0): invalid) or None; claimed: in merge mode the N byte
    maps after the last view, else None.  In merge mode mask has the pixels an earlier view claimed taken out, and colors / normals
    are the means over each point's members."""
    mask: list
    fused_depth: list
    num_consistent: list
    view_bits: list
    points: object
    colors: object
    view_index: object
    sources: list
    normals: object = None
    claimed: list = None


class DepthFusion:
    """Geometric-consistency filter and point-cloud fusion of N views' depth maps (module docstring).

        fusion = DepthFusion(max_uncertainty=0.5)
        out = fusion(depths, intrinsics, poses, uncertainties=unc, images=images)
        write_ply("scene.ply", out.points, out.colors)

    merge=True emits every surface sample once, by the first view that sees it, with the mean colour of the pixels merged into it
    (the result depends on the order of the views); normals=True adds world-frame normals (write_ply(..., normals=out.normals)).
    """

    def __init__(self, min_consistent_views=None, max_reproj_error=1.0, max_rel_depth_diff=0.01, max_uncertainty=None, merge=False,
                 normals=False):
        self.merge = bool(merge)
        self.normals = bool(normals)
        self.min_consistent_views = min_consistent_views
        self.max_reproj_error = float(max_reproj_error)
        self.max_rel_depth_diff = float(max_rel_depth_diff)
        self.max_uncertainty = max_uncertainty

    def __call__(self, depths, intrinsics, poses, uncertainties=None, images=None, sources=None):
        """depths: N x (H,W) (or (1,H,W), (1,1,H,W)); intrinsics N x (3,3); poses N x (4,4) world-to-view; uncertainties: N x (H,W) or
        None; images: N x (3,H,W) or None; sources: per view the indices of its source views (default: all other views).  numpy
        arrays or torch tensors; maps on the GPU run the HIP kernels, maps on the host run fuse_numpy.  All depth and uncertainty
        maps must be in the same place (the host, or one GPU): a mixed list raises instead of being moved silently.  Images only
        colour the points and are taken to where the maps are."""
        N = len(depths)
        if N < 2:
            raise ValueError(f"{N} views: fusion needs at least 2")
        if not (len(intrinsics) == len(poses) == N):
            raise ValueError(f"{N} depth maps, {len(intrinsics)} intrinsics, {len(poses)} poses")
        for name, opt in (("uncertainties", uncertainties), ("images", images)):
            if opt is not None and len(opt) != N:
                raise ValueError(f"{len(opt)} {name} for {N} views")
        sources = default_sources(N) if sources is None else [list(s) for s in sources]
        if len(sources) != N:
            raise ValueError(f"{len(sources)} source lists for {N} views")
        for i, s in enumerate(sources):
            if not 1 <= len(s) <= MAX_SOURCES:
                raise ValueError(f"view {i}: {len(s)} source views, supported 1..{MAX_SOURCES}")
            if any(not 0 <= j < N for j in s):
                raise ValueError(f"view {i}: source index out of range in {s}")
            if self.merge and i in s:
                raise ValueError(f"view {i} is among its own sources {s}: merge mode cannot claim pixels of the view it is emitting")
        Ks = [to_numpy(K).astype(np.float64).reshape(3, 3) for K in intrinsics]
        Ts = [to_numpy(T).astype(np.float64).reshape(4, 4) for T in poses]
        host = one_place(*depths, *(uncertainties or []), what="depth and uncertainty maps") == "host"
        run = self._run_host if host else self._run_device
        return run([map2d(d, f"depths[{i}]") for i, d in enumerate(depths)], Ks, Ts,
                   None if uncertainties is None else [map2d(u, f"uncertainties[{i}]") for i, u in enumerate(uncertainties)],
                   images, sources)

    def _run_host(self, depths, Ks, Ts, uncs, images, sources):
        depths = [to_numpy(d) for d in depths]
        uncs = None if uncs is None else [to_numpy(u) for u in uncs]
        images = None if images is None else [to_numpy(im) for im in images]
        for i, im in enumerate(images or []):
            if im.shape != (3,) + depths[i].shape:
                raise ValueError(f"images[{i}]: shape {im.shape}, expected {(3,) + depths[i].shape}")
        thresholds = (self.min_consistent_views, self.max_reproj_error, self.max_rel_depth_diff, self.max_uncertainty)
        if self.merge:
            r = merge_numpy(depths, Ks, Ts, sources, uncs, images, self.normals, *thresholds)
            colours, normals = r["merged_rgb"], r["merged_normal"]
        else:
            per_view = [fuse_numpy(depths[i], Ks[i], Ts[i], [depths[j] for j in src], [Ks[j] for j in src], [Ts[j] for j in src],
                                   None if uncs is None else uncs[i], *thresholds) for i, src in enumerate(sources)]
            r = {k: [v[k] for v in per_view] for k in ("mask", "fused", "count", "view_bits")}
            colours = images
            normals = [normals_numpy(depths[i], Ks[i], Ts[i]) for i in range(len(depths))] if self.normals else None
        out = FusionResult(r["mask"], [f.astype(np.float32) for f in r["fused"]], r["count"], r["view_bits"], None, None, None, sources,
                           claimed=r.get("claimed"))
        pts, cols, nrms, idx = [], [], [], []
        for i, mask in enumerate(out.mask):
            xyz, rgb = points_numpy(mask, out.fused_depth[i], Ks[i], Ts[i], None if colours is None else colours[i])
            pts.append(xyz.astype(np.float32))
            idx.append(np.full(len(xyz), i, dtype=np.int64))
            if rgb is not None:
                cols.append(rgb.astype(np.float32))
            if normals is not None:
                ys, xs = np.nonzero(mask)
                nrms.append(normals[i][:, ys, xs].T.astype(np.float32))
        out.points, out.view_index = np.concatenate(pts), np.concatenate(idx)
        out.colors = np.concatenate(cols) if images is not None else None
        out.normals = np.concatenate(nrms) if normals is not None else None
        return out

    def _run_device(self, depths, Ks, Ts, uncs, images, sources):
        import torch
        from . import _lib as L
        from . import ops
        dev = depths[0].device
        N = len(depths)
        up = lambda a: a.to(dev) if is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        depths = [up(d) for d in depths]
        uncs = None if uncs is None or self.max_uncertainty is None else [up(u) for u in uncs]
        images = None if images is None else [up(im) for im in images]
        # one upload for every view's tables: (V,24) matrices, then the 12 floats of the back-projection
        tables, offsets = [], []
        for i, src in enumerate(sources):
            m = compose_matrices(Ks[i], Ts[i], [Ks[j] for j in src], [Ts[j] for j in src]).ravel()
            offsets.append(sum(len(t) for t in tables))
            tables += [m, compose_backprojection(Ks[i], Ts[i])]
        table = torch.from_numpy(np.concatenate(tables).astype(np.float32)).to(dev)
        out = FusionResult([], [], [], [], None, None, None, sources)
        backproject = lambda i: table[offsets[i] + 24 * len(sources[i]):offsets[i] + 24 * len(sources[i]) + 12]
        normals = [ops.depth_normals(depths[i], backproject(i)) for i in range(N)] if self.normals else None
        if self.merge:
            # the merge kernel gathers the sources' colours: every image as the kernel takes it, once
            images = None if images is None else [L.as_f32(im, f"images[{i}]", (3,) + tuple(depths[i].shape), dev)
                                                  for i, im in enumerate(images)]
            out.claimed = [torch.zeros(d.shape, dtype=torch.uint8, device=dev) for d in depths]
        thresholds = (self.min_consistent_views, self.max_reproj_error, self.max_rel_depth_diff, self.max_uncertainty)
        # one set of H*W-point buffers for all views: each view's points are copied out at their exact size after the one
        # 8-byte read of its count, so that the call holds M points and one set, not N sets
        buffers, pts, cols, nrms, m = None, [], [], [], []
        for i, src in enumerate(sources):
            V, o = len(src), offsets[i]
            args = (depths[i], [depths[j] for j in src], table[o:o + 24 * V].view(V, 24))
            unc = None if uncs is None else uncs[i]
            if self.merge:
                pick = lambda maps: (None, None) if maps is None else (maps[i], [maps[j] for j in src])
                bits, fused, mask, count, colour, normal = ops.geo_merge(*args, out.claimed[i], [out.claimed[j] for j in src], unc,
                                                                         *thresholds, *pick(images), *pick(normals))
            else:
                bits, fused, mask, count = ops.geo_consistency(*args, unc, *thresholds)
                colour, normal = None if images is None else images[i], None if normals is None else normals[i]
            xyz, rgb, n, *nrm = ops.compact_points(mask, fused, backproject(i), colour, out=buffers, normals=normal)
            buffers = (xyz, rgb, *nrm)
            m.append(int(n.item()))
            pts.append(xyz[:m[-1]].clone())
            if rgb is not None:
                cols.append(rgb[:m[-1]].clone())
            if nrm:
                nrms.append(nrm[0][:m[-1]].clone())
            out.mask.append(mask); out.fused_depth.append(fused); out.num_consistent.append(count); out.view_bits.append(bits)
        out.points = torch.cat(pts)
        out.colors = torch.cat(cols) if images is not None else None
        out.normals = torch.cat(nrms) if normals is not None else None
        out.view_index = torch.repeat_interleave(torch.arange(N, device=dev), torch.tensor(m, device=dev))
        return out

    def reconstruct(self, model, images, intrinsics, poses, num_sources=None, device=None, **fusion_inputs):
        """Runs model.run once per view as the key view and fuses the predictions.  images: N x (3,H,W) numpy; intrinsics N x (3,3) of
        those images; poses N x (4,4) world-to-view.  Each run gets the views ordered key first, then its sources (the num_sources
        nearest by index distance; default: all others), with the model protocol's key-relative poses T_i T_k^-1.  pred["depth"] and,
        where present, aux["depth_uncertainty"] are taken at the prediction's size: K is rescaled to it (the fx/cx row by
        w_pred / w_img, the fy/cy row by h_pred / h_img) and the images are resized to it for the colours.  fusion_inputs go to
        __call__ (sources=...).
        Where the fusion runs: the models of this package answer in numpy (their output adapter), so the predictions are uploaded to
        `device`, by default the GPU that holds the model's parameters, and fused by the HIP kernels; the result holds GPU tensors.
        Without a GPU model and without `device` the maps stay where the model left them (numpy: fuse_numpy on the host);
        device="cpu" asks for the host path."""
        N = len(images)
        if not (len(intrinsics) == len(poses) == N) or N < 2:
            raise ValueError(f"{N} images, {len(intrinsics)} intrinsics, {len(poses)} poses; at least 2 views are needed")
        Ks = [to_numpy(K).astype(np.float64).reshape(3, 3) for K in intrinsics]
        Ts = [to_numpy(T).astype(np.float64).reshape(4, 4) for T in poses]
        depths, uncs, Ks_pred, colours = [], [], [], []
        for k in range(N):
            others = sorted((j for j in range(N) if j != k), key=lambda j: (abs(j - k), j))
            order = [k] + (others if num_sources is None else others[:num_sources])
            Tk_inv = _inv_pose(Ts[k])
            pred, aux = model.run(images=[images[j] for j in order], keyview_idx=0,
                                  poses=[(Ts[j] @ Tk_inv).astype(np.float32) for j in order],
                                  intrinsics=[Ks[j].astype(np.float32) for j in order])
            depth = map2d(pred["depth"], "pred['depth']")
            depths.append(depth)
            unc = (aux or {}).get("depth_uncertainty")
            uncs.append(None if unc is None else map2d(unc, "aux['depth_uncertainty']"))
            img = to_numpy(images[k]).astype(np.float32)
            img = img.reshape(img.shape[-3:])
            (hp, wp), (hi, wi) = depth.shape, img.shape[-2:]
            K = Ks[k].copy()
            K[0] *= wp / wi
            K[1] *= hp / hi
            Ks_pred.append(K)
            colours.append(_resize_nearest(img, hp, wp))
        uncs = uncs if all(u is not None for u in uncs) else None
        device = _model_device(model) if device is None else device
        if device is not None:
            import torch
            device = torch.device(device)
            move = ((lambda a: torch.as_tensor(a).to(device)) if device.type == "cuda" else to_numpy)
            depths = [move(d) for d in depths]
            uncs = None if uncs is None else [move(u) for u in uncs]
        return self(depths, Ks_pred, Ts, uncs, colours, **fusion_inputs)


def _model_device(model):
    """The GPU that holds the model's parameters, or None (no parameters, or on the host)."""
    params = getattr(model, "parameters", None)
    first = next(iter(params()), None) if callable(params) else None
    return first.device if first is not None and first.is_cuda else None


def _resize_nearest(img, h, w):
    """(3,H,W) -> (3,h,w), the pixel whose centre is nearest (the rule of depth_score.resize_index)."""
    from .depth_score import resize_index
    return np.ascontiguousarray(img[:, resize_index(img.shape[1], h)][:, :, resize_index(img.shape[2], w)])
