"""Cases for the mesh-rendering tests (test_render_cpu.py, test_hip_render.py): the meshes, the cameras, the constructed small cases, a
brute-force renderer written straight from the definition, and the reference for the device test derived from render_numpy alone.
Everything is built once (treat the arrays as read-only).

Meshes.  "sphere": extract_numpy of tsdf_cases.sphere_volume() at origin (-0.83, -0.86, 2.2), voxel 0.1: 1502 vertices and 3000
triangles (no multiple of 64 or 256), each about one pixel at these sizes.  "sphere+plane": the sphere plus the quad (+-9, +-9) on
the plane z = 4 + (x + y) / 90 behind it, two triangles far larger than the image: box clamping, the large path and occlusion.
Cameras: fusion_cases.intrinsics and the first three of fusion_cases.poses(), sizes fusion_cases.SIZES.  Colours: a field linear in
the world position, so that a perspective-correct rendering returns the field at the back-projected pixel.
"""
import functools

import numpy as np

import fusion_cases as FC
import tsdf_cases as TC
from robustmvd_amd import render as R
from robustmvd_amd import tsdf as TS

SPHERE_ORIGIN, SPHERE_VOXEL = (-0.83, -0.86, 2.2), 0.1
SPHERE_CENTRE = tuple(o + SPHERE_VOXEL * c for o, c in zip(SPHERE_ORIGIN, TC.SPHERE[1]))
NUM_VIEWS = 3
MAX_EXCLUDED_SHARE = 0.01
COLOR_A = np.array([[40.0, 5.0, -3.0], [-7.0, 30.0, 2.0], [4.0, -6.0, 25.0]])
COLOR_B = np.array([100.0, 120.0, 60.0])


def color_field(X):
    """(..., 3) world positions -> (..., 3) colours, float64"""
    return np.asarray(X, dtype=np.float64) @ COLOR_A.T + COLOR_B


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> (vertices (M,3) float32, triangles (T,3) int32, colors (M,3) float32)"""
    assert name in ("sphere", "sphere+plane")
    F, Wt = TC.sphere_volume()
    v, _, t = TS.extract_numpy(F, Wt, None, SPHERE_ORIGIN, SPHERE_VOXEL)
    v = v.astype(np.float32)
    assert v.shape == (1502, 3) and t.shape == (3000, 3)
    if name == "sphere+plane":
        quad = np.array([[-9, -9, 3.8], [9, -9, 4.0], [9, 9, 4.2], [-9, 9, 4.0]], dtype=np.float32)
        t = np.concatenate([t, np.array([[0, 2, 1], [0, 3, 2]], dtype=np.int32) + len(v)])  # the quad faces the cameras
        v = np.concatenate([v, quad])
    return v, t.astype(np.int32), color_field(v).astype(np.float32)


def cameras(H, W, V=NUM_VIEWS):
    """-> (Ks, Ts): V views, fusion_cases' cameras cycled"""
    Ts = FC.poses()
    return [FC.intrinsics(H, W)] * V, [Ts[i % len(Ts)] for i in range(V)]


def plane_depth(K, T, H, W, corners):
    """The analytic view-z of the plane through the three corners (3,3) along each pixel's ray, float64 (H,W).  The quad's float32
    corners are not exactly coplanar (3.8 and 4.2 are rounded), so each of its two triangles has its own plane."""
    p = np.asarray(corners, dtype=np.float64)
    PLANE_N = np.cross(p[1] - p[0], p[2] - p[0])
    PLANE_D = PLANE_N @ p[0]
    R_, C = T[:3, :3], -T[:3, :3].T @ T[:3, 3]
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.einsum("ij,jhw->ihw", R_.T @ np.linalg.inv(K), np.stack([x, y, np.ones_like(x)]))
    return (PLANE_D - PLANE_N @ C) / np.einsum("i,ihw->hw", PLANE_N, rays)


def backproject(K, T, depth):
    """(H,W) view-z -> (H,W,3) world positions of the pixels' rays at that depth"""
    H, W = depth.shape
    R_, C = T[:3, :3], -T[:3, :3].T @ T[:3, 3]
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.einsum("ij,jhw->hwi", R_.T @ np.linalg.inv(K), np.stack([x, y, np.ones_like(x)]))
    return C + depth[..., None] * rays


# ---- constructed small cases ---------------------------------------------------------------------------------------------------------
SMALL_SIZE = (9, 11)
SMALL_K = np.array([[4.0, 0, 5], [0, 4.0, 4], [0, 0, 1]])  # at z = 2: x = 2 X + 5, y = 2 Y + 4, exact integers for half-integer X, Y
_A, _B, _C, _D = (-2, -1.5, 2), (2, -1.5, 2), (-2, 1.5, 2), (2, 1.5, 2)  # pixels (1,1), (9,1), (1,7), (9,7)


def small_cases():
    """name -> (vertices, triangles): rendered with SMALL_K, the identity pose and SMALL_SIZE.  Every screen coordinate is an exact
    integer or half-integer in float32 and float64 alike, so that the two chains and the device agree on every verdict."""
    f, i = (lambda a: np.array(a, dtype=np.float32).reshape(-1, 3)), (lambda a: np.array(a, dtype=np.int32).reshape(-1, 3))
    return {
        "empty": (f([_A, _B, _C]), i([])),
        "one": (f([_A, _B, _C]), i([[0, 1, 2]])),
        "duplicate": (f([_A, _B, _C]), i([[0, 1, 2], [0, 1, 2]])),
        "behind": (f([_A, _B, (-2, 1.5, -1), _C]), i([[0, 1, 2], [1, 3, 0]])),  # the first has a vertex behind the camera
        "zero_area": (f([_A, (0, -1.5, 2), _B, _C]), i([[0, 1, 2], [0, 0, 3], [0, 2, 3]])),  # collinear; a repeated index; a real one
        "off_image": (f([(10, 0, 2), (12, 0, 2), (10, 2, 2), _A, _B, _C]), i([[0, 1, 2], [3, 4, 5]])),
        # two triangles that share the edge (9,1)-(1,7), which passes exactly through pixel (5,4); all on pixel centres
        "shared_edge": (f([_A, _B, _C, _D]), i([[0, 1, 2], [1, 3, 2]])),
    }


def small_views():
    return [SMALL_K], [np.eye(4)]


# ---- brute force -----------------------------------------------------------------------------------------------------------------------
def brute_force(vertices, triangles, K, T, size, cull=None, near=0.0):
    """One view, straight from the definition in float64: every triangle against every pixel of the image, no boxes, a python loop
    over the triangles -> (depth, triangle, bary (3,H,W), cover count (H,W))."""
    H, W = size
    P = (np.asarray(K, dtype=np.float64) @ np.asarray(T, dtype=np.float64)[:3])
    X = np.asarray(vertices, dtype=np.float64)
    with np.errstate(all="ignore"):
        q = [P[r, 0] * X[:, 0] + P[r, 1] * X[:, 1] + P[r, 2] * X[:, 2] + P[r, 3] for r in range(3)]
        x, y, z = q[0] / q[2], q[1] / q[2], q[2]
    valid = (z > near) & np.isfinite(x) & np.isfinite(y)
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth, index = np.full((H, W), np.inf), np.full((H, W), -1, dtype=np.int32)
    bary, count = np.zeros((3, H, W)), np.zeros((H, W), dtype=np.int64)

    def edge(i, j):
        a, b = min(i, j), max(i, j)
        e = (x[b] - x[a]) * (py - y[a]) - (y[b] - y[a]) * (px - x[a])
        return e if i < j else -e

    for n, (i0, i1, i2) in enumerate(np.asarray(triangles).tolist()):
        if not (valid[i0] and valid[i1] and valid[i2]):
            continue
        A = (x[i1] - x[i0]) * (y[i2] - y[i0]) - (y[i1] - y[i0]) * (x[i2] - x[i0])
        if not (A < 0 or A > 0) or (cull == "back" and A > 0) or (cull == "front" and A < 0):
            continue
        sgn = -1.0 if A < 0 else 1.0
        w = [sgn * edge(i1, i2), sgn * edge(i2, i0), sgn * edge(i0, i1)]
        s = (w[0] + w[1]) + w[2]
        with np.errstate(all="ignore"):
            b = [wk / s for wk in w]
            d = 1 / ((b[0] / z[i0] + b[1] / z[i1]) + b[2] / z[i2])
        cov = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0) & (s > 0) & np.isfinite(d)
        count += cov
        win = cov & (d < depth)  # a later triangle wins only with a strictly smaller z: ties stay with the lower index
        depth[win], index[win] = d[win], n
        for k in range(3):
            bary[k][win] = b[k][win]
    return np.where(index >= 0, depth, 0.0), index, bary, count


# ---- the reference of the device test ---------------------------------------------------------------------------------------------------
def _gap(a, b, keep):
    """the largest |a - b| over per-view maps (H,W) or (3,H,W) on the kept pixels"""
    return max((float(np.abs(x - y)[..., k].max()) if k.any() else 0.0) for x, y, k in zip(a, b, keep))


def reference_of(vertices, triangles, colors, Ks, Ts, size, cull=None, near=0.0):
    """render_numpy in float64 and the same chain in float32 on the float32-rounded P, and what the device test derives from the two
    alone.  band["xy"]: four times the largest gap of the projected x, y in pixels; band["z"]: four times the largest relative gap of
    z, over the projected vertices and over the rendered depth where the two chains agree on the winner (the kernel's chain may order
    its operations differently, each of the order of one more float32 rounding of the same chain).  A pixel is excluded when some
    triangle that covers or nearly covers it (every normalised edge distance >= -band) with z <= the winner's z (1 + zband) has an
    edge line within the band of the pixel, or when the two chains disagree on its winner.  On the rest the triangle maps must be
    equal; the bands of bary, colors and normals are four times their own float64-float32 gap on the kept pixels."""
    H, W = size
    kw = dict(colors=colors, normals=True, bary=True, cull=cull, near=near, details=True)
    r64, d64 = R.render_numpy(vertices, triangles, Ks, Ts, size, **kw)
    r32, d32 = R.render_numpy(vertices, triangles, Ks, Ts, size, dtype=np.float32, **kw)
    V = len(Ks)
    gap_xy, gap_z = 0.0, 0.0
    for v in range(V):
        both = d64["valid"][v] & d32["valid"][v]
        assert np.array_equal(d64["valid"][v], d32["valid"][v])  # no vertex within a rounding of the near plane
        if both.any():
            gap_xy = max(gap_xy, float(np.abs(d64["x"][v] - d32["x"][v])[both].max()), float(np.abs(d64["y"][v] - d32["y"][v])[both].max()))
            gap_z = max(gap_z, float((np.abs(d64["z"][v] - d32["z"][v]) / d64["z"][v])[both].max()))
        same = (r64.triangle[v] == r32.triangle[v]) & r64.mask[v]
        if same.any():
            gap_z = max(gap_z, float((np.abs(r64.depth[v] - r32.depth[v].astype(np.float64))[same] / r64.depth[v][same]).max()))
    band = {"xy": 4.0 * gap_xy, "z": 4.0 * gap_z}
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    excluded = []
    for v in range(V):
        x, y, z, valid = d64["x"][v], d64["y"][v], d64["z"][v], d64["valid"][v]
        ex = r64.triangle[v] != r32.triangle[v]
        if len(tri):
            i0, i1, i2 = tri[:, 0], tri[:, 1], tri[:, 2]
            with np.errstate(all="ignore"):
                A = (x[i1] - x[i0]) * (y[i2] - y[i0]) - (y[i1] - y[i0]) * (x[i2] - x[i0])
            ok = valid[i0] & valid[i1] & valid[i2] & (A != 0) & np.isfinite(A)
            if cull == "back":
                ok &= A < 0
            elif cull == "front":
                ok &= A > 0
            xs, ys = np.stack([x[i0], x[i1], x[i2]])[:, ok], np.stack([y[i0], y[i1], y[i2]])[:, ok]
            kept = np.nonzero(ok)[0]
            clamp = lambda a, hi: np.clip(a, -1, hi + 1).astype(np.int64)
            x0, x1 = np.maximum(clamp(np.floor(xs.min(axis=0) - band["xy"]), W), 0), np.minimum(clamp(np.ceil(xs.max(axis=0) + band["xy"]), W), W - 1)
            y0, y1 = np.maximum(clamp(np.floor(ys.min(axis=0) - band["xy"]), H), 0), np.minimum(clamp(np.ceil(ys.max(axis=0) + band["xy"]), H), H - 1)
            there = (x0 <= x1) & (y0 <= y1)
            kept, x0, x1, y0, y1 = kept[there], x0[there], x1[there], y0[there], y1[there]
            which, px, py = R.box_pairs(x0, x1, y0, y1)
            t = tri[kept[which]]
            sgn = np.where(A[kept[which]] < 0, -1.0, 1.0)
            fx, fy = px.astype(np.float64), py.astype(np.float64)
            dist, w = [], []
            for a, b in ((1, 2), (2, 0), (0, 1)):
                e = sgn * R.oriented_edge(t[:, a], t[:, b], x, y, fx, fy)
                w.append(e)
                dist.append(e / np.hypot(x[t[:, a]] - x[t[:, b]], y[t[:, a]] - y[t[:, b]]))
            dist = np.stack(dist)
            with np.errstate(all="ignore"):
                s = (w[0] + w[1]) + w[2]
                zz = 1 / ((w[0] / s / z[t[:, 0]] + w[1] / s / z[t[:, 1]]) + w[2] / s / z[t[:, 2]])
            zw = np.where(r64.mask[v], r64.depth[v], np.inf)[py, px]
            near_cover = (dist >= -band["xy"]).all(axis=0)
            with np.errstate(invalid="ignore"):
                risky = near_cover & ~(zz > zw * (1 + band["z"])) & (np.abs(dist).min(axis=0) <= band["xy"])
            ex[py[risky], px[risky]] = True
        excluded.append(ex)
    keep = [~e for e in excluded]
    span = float(np.ptp(colors)) if colors is not None and len(colors) else 1.0
    gap = {"xy": gap_xy, "z": gap_z, "bary": _gap(r64.bary, r32.bary, keep), "normals": _gap(r64.normals, r32.normals, keep),
           "colors": _gap(r64.colors, r32.colors, keep) / span if colors is not None else 0.0}
    for k in ("bary", "normals", "colors"):
        band[k] = 4.0 * gap[k]
    return {"r64": r64, "r32": r32, "gap": gap, "band": band, "excluded": excluded, "span": span,
            "share": float(np.mean([e.mean() for e in excluded])), "chains_agree": all(np.array_equal(a, b) for a, b in zip(r64.triangle, r32.triangle))}


@functools.lru_cache(maxsize=None)
def reference(name, H, W, cull=None, near=0.0, V=NUM_VIEWS):
    v, t, c = mesh(name)
    Ks, Ts = cameras(H, W, V)
    return reference_of(v, t, c, Ks, Ts, (H, W), cull, near)


def check_against_reference(ref, got, what=""):
    """got: per-view numpy maps of a device rendering, dict depth, triangle, bary, colors, normals (None: not compared).  Prints the
    figures, then asserts the device test's comparison."""
    r64, keep = ref["r64"], [~e for e in ref["excluded"]]
    tri_diffs = sum(int((g != r)[k].sum()) for g, r, k in zip(got["triangle"], r64.triangle, keep))
    covered = [k & m for k, m in zip(keep, r64.mask)]
    z_gap = max((float((np.abs(g - r)[k] / r[k]).max()) if k.any() else 0.0) for g, r, k in zip(got["depth"], r64.depth, covered))
    empty_ok = all(bool((g[k & ~m] == 0).all()) for g, k, m in zip(got["depth"], keep, r64.mask))
    gaps = {n: (_gap(got[n], getattr(r64, n), keep) / (ref["span"] if n == "colors" else 1.0) if got.get(n) is not None else None)
            for n in ("bary", "colors", "normals")}
    print(f"\n{what}: gap xy {ref['gap']['xy']:.2e} px, z {ref['gap']['z']:.2e}; excluded {100 * ref['share']:.3f} %; chains agree "
          f"{ref['chains_agree']}; device: triangle diffs {tri_diffs}, max rel |z - f64| {z_gap:.2e} (band {ref['band']['z']:.2e}), "
          + ", ".join(f"{n} {g:.2e} (band {ref['band'][n]:.2e})" for n, g in gaps.items() if g is not None))
    assert ref["share"] <= MAX_EXCLUDED_SHARE
    assert tri_diffs == 0 and empty_ok
    assert z_gap <= ref["band"]["z"]
    for n, g in gaps.items():
        assert g is None or g <= ref["band"][n], n
