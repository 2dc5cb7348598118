"""Mesh rendering: a triangle mesh rasterised into pinhole views, giving per view a depth map, a triangle-index map and, on request,
barycentric, colour and normal maps.  It closes the reconstruction chain (depth maps -> DepthFusion -> TSDFVolume -> Mesh) back into
a camera.  The reference has no such component; the definition is this docstring, render_numpy (the readable specification and the
CPU path) and include/mvd.h.

Inputs.  vertices (M,3) float32 in world coordinates, triangles (T,3) int32 into them, optional colors (M,3) float32; per view pinhole
intrinsics K and a world-to-view pose T; one image size (H,W) for all views.  Pixel (px,py) is sampled at the image point (px,py), an
integer: the convention of depth_fusion and tsdf.

  1. Projection matrix.  The host composes P = K T[:3] in float64 and hands its 12 values to the device as float32.
  2. Vertex.  (qx,qy,qz) = P (X,1), each row summed left to right.  The vertex is valid iff qz > near (default 0) and x = qx / qz,
     y = qy / qz are finite; z = qz.  The screen vertex is a function of the vertex and the view alone, so every triangle that shares
     it sees the same bits.
  3. Triangle (i0,i1,i2).  Skipped if a vertex is invalid (there is no near-plane clipping).  Skipped unless its signed area
     A = (x1-x0)(y2-y0) - (y1-y0)(x2-x0) is < 0 or > 0 (zero, and NaN from an overflow, are skipped).  Skipped if its pixel bounding
     box [ceil(min x), floor(max x)] x [ceil(min y), floor(max y)], clamped to the image, is empty.  Front-facing iff A < 0: with x
     right, y down and z forward, a winding normal (p1-p0) x (p2-p0) that points at the camera projects to negative area.
     cull="back" skips A > 0, cull="front" skips A < 0, cull=None (the default) keeps both.
  4. Edge value.  For the vertex pair a < b, ordered by index, e_ab(p) = (x_b-x_a)(p_y-y_a) - (y_b-y_a)(p_x-x_a), evaluated as
     written with one rounding per operation (no FMA contraction).  A triangle's oriented edge (i,j) uses +e_ij when i < j and -e_ji
     otherwise.  w0, w1, w2 are the oriented edges (i1,i2), (i2,i0), (i0,i1), the ones opposite i0, i1, i2, multiplied by sign(A).
     The pixel is covered iff w0 >= 0, w1 >= 0, w2 >= 0 and s = (w0 + w1) + w2 > 0 (s = 0 only for a sliver whose edge values all
     round to zero at the pixel).  Two triangles that share an edge compute the same bits with opposite sign: no pixel between them
     is lost, and a pixel exactly on the edge belongs to both.  That is what renders a watertight mesh without cracks.
  5. Depth.  b_k = w_k / s, u_k = b_k / z_k, z = 1 / ((u0 + u1) + u2): exact for a planar triangle.  A pixel whose z is not finite
     is not covered.
  6. Winner.  Per pixel the covered triangle with the smallest z wins, ties go to the smallest triangle index: the order of the
     64-bit key (float bits of z) << 32 | index.
  7. Outputs per view.  depth (H,W) float32: the winner's z, 0 where nothing covers the pixel.  triangle (H,W) int32: the winner's
     index, or -1.  On request bary (3,H,W) float32: b0, b1, b2;  colors (3,H,W): perspective-correct, z ((u0 c0 + u1 c1) + u2 c2),
     0 where nothing covers;  normals (3,H,W): the winner's unit world-frame winding normal n / |n|, n = (p1-p0) x (p2-p0),
     |n| = sqrt((nx nx + ny ny) + nz nz), or (0,0,0) where |n| is zero or not finite, or the pixel empty.

  8. Smooth normals (render_mesh(normals="vertex")).  The vertex normals (mesh_clean.py, step 5; a Mesh's own `normals` where it has
     them) go through step 7's colour interpolation as a per-vertex attribute, and the interpolated vector v is renormalised per pixel:
     v / sqrt((vx vx + vy vy) + vz vz), (0,0,0) where that length is zero or not finite or the pixel empty.

Left out: near-plane clipping (a triangle with a vertex at or behind the near plane is dropped whole) and anti-aliasing.

Two implementations: render_numpy on the host and the HIP kernels of csrc/mesh_render.hip (ops.mesh_render) for a mesh on a GPU.
render_mesh picks by where the vertices live.
"""
from dataclasses import dataclass

import numpy as np

from .depth_fusion import pinhole
from .mesh import check_mesh, one_place, split_mesh, to_numpy

MAX_VIEWS = 32  # views per launch (MVD_MAX_VIEWS)
CULL = {None: 0, "none": 0, "back": 1, "front": 2}
_PAIR_BUDGET = 1 << 22  # (triangle, pixel) pairs evaluated at a time by render_numpy


def compose_projection(K, T):
    """-> 12 float64, row-major 3x4: P = K T[:3], which takes (X,1) to (qx,qy,qz)."""
    K, T = pinhole(K, "intrinsics"), np.asarray(T, dtype=np.float64).reshape(4, 4)
    return (K @ T[:3]).ravel()


def check_colors(colors, M):
    """The renderer takes exactly three channels, of any dtype (both paths convert)."""
    if colors is not None and tuple(colors.shape) != (M, 3):
        raise ValueError(f"colors: shape {tuple(colors.shape)}, expected {(M, 3)}")


def check_views(intrinsics, poses, size):
    """-> (V, H, W)"""
    V = len(intrinsics)
    if len(poses) != V:
        raise ValueError(f"{V} intrinsics, {len(poses)} poses")
    if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
        raise ValueError(f"size must be (H,W) with H, W >= 1, got {size}")
    H, W = int(size[0]), int(size[1])
    if H * W * max(V, 1) >= 2 ** 31:
        raise ValueError(f"H W V = {H * W * V} must be below 2^31")
    return V, H, W


def check_cull(cull):
    if cull not in CULL:
        raise ValueError(f"cull must be None, 'back' or 'front', got {cull!r}")
    return CULL[cull]


def edge_value(xa, ya, xb, yb, px, py):
    """e_ab(p) of the module docstring, one rounding per operation."""
    return (xb - xa) * (py - ya) - (yb - ya) * (px - xa)


def oriented_edge(i, j, x, y, px, py):
    """The oriented edge (i,j) at p: +e_ij where i < j, -e_ji otherwise.  i, j: index arrays; x, y: the screen vertices."""
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    e = edge_value(x[lo], y[lo], x[hi], y[hi], px, py)
    return np.where(i < j, e, -e)


def project_numpy(vertices, P, near, ft):
    """Step 2 for one view -> (x, y, z, valid) of dtype ft."""
    X = [vertices[:, c].astype(ft) for c in range(3)]
    with np.errstate(all="ignore"):
        q = [P[4 * r] * X[0] + P[4 * r + 1] * X[1] + P[4 * r + 2] * X[2] + P[4 * r + 3] for r in range(3)]
        x, y = q[0] / q[2], q[1] / q[2]
        valid = (q[2] > ft(near)) & np.isfinite(x) & np.isfinite(y)
    return x, y, q[2], valid


def setup_numpy(tri, x, y, valid, H, W, cull):
    """Step 3 for one view -> (kept triangle indices, sign(A) of each, its clamped box x0, x1, y0, y1 as int64)."""
    ft = x.dtype.type
    i0, i1, i2 = tri[:, 0], tri[:, 1], tri[:, 2]
    with np.errstate(all="ignore"):
        A = (x[i1] - x[i0]) * (y[i2] - y[i0]) - (y[i1] - y[i0]) * (x[i2] - x[i0])
        ok = valid[i0] & valid[i1] & valid[i2] & ((A < 0) | (A > 0))
        if cull == 1:
            ok &= ~(A > 0)
        elif cull == 2:
            ok &= ~(A < 0)
        xs, ys = np.stack([x[i0], x[i1], x[i2]]), np.stack([y[i0], y[i1], y[i2]])
        # clamped as floats first: a box far outside the image stays representable
        x0 = np.minimum(np.maximum(np.ceil(xs.min(axis=0)), ft(0)), ft(W))
        x1 = np.minimum(np.maximum(np.floor(xs.max(axis=0)), ft(-1)), ft(W - 1))
        y0 = np.minimum(np.maximum(np.ceil(ys.min(axis=0)), ft(0)), ft(H))
        y1 = np.minimum(np.maximum(np.floor(ys.max(axis=0)), ft(-1)), ft(H - 1))
        ok &= (x0 <= x1) & (y0 <= y1)  # NaN never gets here: the vertices are valid
    keep = np.nonzero(ok)[0]
    box = [np.where(ok, b, 0).astype(np.int64)[keep] for b in (x0, x1, y0, y1)]
    return keep, np.where(A[keep] < 0, ft(-1), ft(1)), box


def cover_numpy(tri, sgn, x, y, z, px, py):
    """Steps 4 and 5 for (triangle, pixel) pairs: tri (n,3) indices, sgn (n,), px, py (n,) of the views' dtype ->
    (covered, w (3,n), s, b (3,n), u (3,n), depth)."""
    i0, i1, i2 = tri[:, 0], tri[:, 1], tri[:, 2]
    with np.errstate(all="ignore"):
        w = np.stack([sgn * oriented_edge(i1, i2, x, y, px, py), sgn * oriented_edge(i2, i0, x, y, px, py),
                      sgn * oriented_edge(i0, i1, x, y, px, py)])
        s = (w[0] + w[1]) + w[2]
        b = w / s
        u = np.stack([b[0] / z[i0], b[1] / z[i1], b[2] / z[i2]])
        depth = 1 / ((u[0] + u[1]) + u[2])
        covered = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0) & (s > 0) & np.isfinite(depth)
    return covered, w, s, b, u, depth


def box_pairs(x0, x1, y0, y1):
    """Every pixel of every box, boxes in order and pixels row-major -> (box index, px, py) int64"""
    bw = x1 - x0 + 1
    n = bw * (y1 - y0 + 1)
    which = np.repeat(np.arange(len(n), dtype=np.int64), n)
    local = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    return which, x0[which] + local % bw[which], y0[which] + local // bw[which]


def normals_of(vertices, tri, ft):
    """The unit winding normal of each triangle (n,3) in dtype ft, (0,0,0) where its length is zero or not finite."""
    p = [vertices[tri[:, k]].astype(ft) for k in range(3)]
    a, b = p[1] - p[0], p[2] - p[0]
    with np.errstate(all="ignore"):
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]],
                     axis=1)
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        good = (length > 0) & np.isfinite(length)
        return np.where(good[:, None], n / length[:, None], ft(0))


@dataclass
class RenderResult:
    """Per view (lists of V maps; numpy arrays from the host path, GPU tensors from the device path): depth (H,W) float32, 0 where
    nothing covers the pixel; triangle (H,W) int32, -1 there; mask (H,W) bool, triangle >= 0; bary, colors and normals (3,H,W)
    float32 where requested, else None.  render_numpy gives the maps in its dtype."""
    depth: list
    triangle: list
    mask: list
    bary: list = None
    colors: list = None
    normals: list = None


def render_numpy(vertices, triangles, intrinsics, poses, size, colors=None, normals=False, bary=False, cull=None, near=0.0,
                 dtype=np.float64, details=False):
    """The definition of the module docstring as a numpy chain -> RenderResult with maps of `dtype` (triangle int32).
    dtype=np.float32 evaluates the same chain in float32 on the float32-rounded P (what the device is handed): the gap between the
    two is what tests/render_cases.py derives its bands from.  details=True adds a second result, a dict of per-view arrays: x, y, z
    (M,) and valid (M,), the screen vertices."""
    ft = np.dtype(dtype).type
    vertices = np.asarray(to_numpy(vertices), dtype=np.float32)
    tri = np.asarray(to_numpy(triangles))
    colors = None if colors is None else np.asarray(to_numpy(colors), dtype=np.float32)
    M, T = check_mesh(vertices, tri, dtypes=False)
    check_colors(colors, M)
    V, H, W = check_views(intrinsics, poses, size)
    cull = check_cull(cull)
    tri = tri.astype(np.int64)
    out = RenderResult([], [], [], [] if bary else None, [] if colors is not None else None, [] if normals else None)
    det = {n: [] for n in ("x", "y", "z", "valid")}
    for v in range(V):
        P = compose_projection(intrinsics[v], poses[v])
        P = (P.astype(np.float32) if ft is np.float32 else P).astype(ft)
        x, y, z, valid = project_numpy(vertices, P, near, ft)
        keep, sgn, (x0, x1, y0, y1) = setup_numpy(tri, x, y, valid, H, W, cull)
        cum = np.cumsum((x1 - x0 + 1) * (y1 - y0 + 1))
        sign_of = np.zeros(T, dtype=ft)
        sign_of[keep] = sgn
        cand = [(np.zeros(0, np.int64), np.zeros(0, ft), np.zeros(0, np.int64))]
        start = 0
        while start < len(keep):  # runs of triangles whose boxes hold at most _PAIR_BUDGET pixels together (at least one triangle)
            done = int(cum[start - 1]) if start else 0
            stop = max(start + 1, int(np.searchsorted(cum, done + _PAIR_BUDGET, side="right")))
            which, px, py = box_pairs(x0[start:stop], x1[start:stop], y0[start:stop], y1[start:stop])
            t = keep[start:stop][which]
            covered, _, _, _, _, d = cover_numpy(tri[t], sgn[start:stop][which], x, y, z, px.astype(ft), py.astype(ft))
            cand.append((py[covered] * W + px[covered], d[covered], t[covered]))
            start = stop
        pix, d, t = (np.concatenate(c) for c in zip(*cand))
        order = np.lexsort((t, d, pix))  # by pixel, then z, then index: the first of each pixel wins
        pix, d, t = pix[order], d[order], t[order]
        first = np.ones(len(pix), dtype=bool)
        first[1:] = pix[1:] != pix[:-1]
        pix, d, t = pix[first], d[first], t[first]
        depth, index = np.zeros(H * W, dtype=ft), np.full(H * W, -1, dtype=np.int32)
        depth[pix], index[pix] = d, t
        out.depth.append(depth.reshape(H, W))
        out.triangle.append(index.reshape(H, W))
        out.mask.append((index >= 0).reshape(H, W))
        if bary or colors is not None:
            _, _, _, b, u, dw = cover_numpy(tri[t], sign_of[t], x, y, z, (pix % W).astype(ft), (pix // W).astype(ft))
            if bary:
                m = np.zeros((3, H * W), dtype=ft)
                m[:, pix] = b
                out.bary.append(m.reshape(3, H, W))
            if colors is not None:
                c = [colors[tri[t, k]].astype(ft) for k in range(3)]
                m = np.zeros((3, H * W), dtype=ft)
                for ch in range(3):
                    m[ch, pix] = dw * ((u[0] * c[0][:, ch] + u[1] * c[1][:, ch]) + u[2] * c[2][:, ch])
                out.colors.append(m.reshape(3, H, W))
        if normals:
            m = np.zeros((3, H * W), dtype=ft)
            m[:, pix] = normals_of(vertices, tri[t], ft).T
            out.normals.append(m.reshape(3, H, W))
        for name, a in (("x", x), ("y", y), ("z", z), ("valid", valid)):
            det[name].append(a)
    return (out, det) if details else out


def _renormalise(m):
    """(3,H,W) interpolated vectors -> unit vectors, (0,0,0) where the length is zero or not finite: numpy in float64, rounded to
    float32; a GPU tensor in float32."""
    if isinstance(m, np.ndarray):
        v = m.astype(np.float64)
        with np.errstate(all="ignore"):
            length = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            good = (length > 0) & np.isfinite(length)
            return np.where(good, v / np.where(good, length, 1.0), 0.0).astype(np.float32)
    import torch
    length = torch.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    good = (length > 0) & torch.isfinite(length)
    return torch.where(good, m / torch.where(good, length, torch.ones_like(length)), torch.zeros_like(m))


def _render_smooth(mesh, intrinsics, poses, size, triangles, colors, bary, cull, near, max_small):
    """Step 8: the vertex normals through the colour path, a second rendering when colours are wanted too."""
    from .mesh_clean import vertex_normals
    vertices, tri, colors = split_mesh(mesh, triangles, colors)
    vn = getattr(mesh, "normals", None)
    if vn is None:
        vn = vertex_normals(vertices, tri)
    kw = dict(cull=cull, near=near, max_small=max_small)
    smooth = render_mesh(vertices, intrinsics, poses, size, triangles=tri, colors=vn, bary=bary and colors is None, **kw)
    out = smooth if colors is None else render_mesh(vertices, intrinsics, poses, size, triangles=tri, colors=colors, bary=bary, **kw)
    out.normals = [_renormalise(m) for m in smooth.colors]
    if colors is None:
        out.colors = None
    return out


def render_mesh(mesh, intrinsics, poses, size, triangles=None, colors=None, normals=False, bary=False, cull=None, near=0.0,
                max_small=None):
    """Renders a mesh into V views of one size (module docstring) -> RenderResult.  normals: False, True for the winning triangle's
    face normal, or "vertex" for interpolated vertex normals (step 8).

    mesh: a Mesh (tsdf.extract_mesh's), a pair (vertices, triangles), or the vertices with triangles=.  colors: None, the (M,3)
    vertex colours, or True for a Mesh's own.  intrinsics V x (3,3), poses V x (4,4) world-to-view, size (H,W).  Vertices on a GPU
    run the HIP kernels on that device, in launches of up to 32 views, and the maps are GPU tensors; vertices on the host run
    render_numpy (float64, maps returned as float32).  max_small (device only): csrc/mesh_render.hip's threshold between its two
    rasterisation paths; every value gives the same bits."""
    if isinstance(normals, str):
        if normals != "vertex":
            raise ValueError(f"normals must be False, True or 'vertex', got {normals!r}")
        return _render_smooth(mesh, intrinsics, poses, size, triangles, colors, bary, cull, near, max_small)
    vertices, triangles, colors = split_mesh(mesh, triangles, colors)
    if one_place(*(a for a in (vertices, triangles, colors) if a is not None), what="mesh arrays") == "host":
        r = render_numpy(vertices, triangles, intrinsics, poses, size, colors, normals, bary, cull, near)
        f32 = lambda maps: None if maps is None else [m.astype(np.float32) for m in maps]
        return RenderResult(f32(r.depth), r.triangle, r.mask, f32(r.bary), f32(r.colors), f32(r.normals))
    import torch
    from . import ops
    M, T = check_mesh(vertices, triangles, dtypes=False)  # the index range: one reduction for all the launches
    check_colors(colors, M)
    V, H, W = check_views(intrinsics, poses, size)
    check_cull(cull)
    table = torch.from_numpy(np.stack([compose_projection(to_numpy(K), to_numpy(P)) for K, P in zip(intrinsics, poses)])
                             .astype(np.float32).reshape(V, 12)).to(vertices.device) if V else None
    out = RenderResult([], [], [], [] if bary else None, [] if colors is not None else None, [] if normals else None)
    per = max(1, min(MAX_VIEWS, (2 ** 32 - 1) // max(T, 1)))  # views per launch: views x triangles stays below 2^32
    for start in range(0, V, per):
        r = ops.mesh_render(vertices, triangles, table[start:start + per], (H, W), colors, normals, bary, cull, near, max_small,
                            check_indices=False)
        for name in ("depth", "triangle", "bary", "colors", "normals"):
            if r[name] is not None:
                getattr(out, name).extend(r[name].unbind(0))
    out.mask = [t >= 0 for t in out.triangle]
    return out
