"""TSDF volume fusion and triangle-mesh extraction: the depth maps of all views averaged into one truncated signed distance volume,
and the surface of that volume as a triangle mesh (marching tetrahedra).  The reference has no such component; the definition is this
docstring, integrate_numpy / extract_numpy (the readable specification and the CPU path) and include/mvd.h.

Volume.  dims = (nx, ny, nz), origin = the world position of voxel (0,0,0), voxel = the edge length s: voxel (i,j,k) sits at
origin + s (i,j,k).  The state is dense, x fastest: tsdf (nz,ny,nx) float32, weight (nz,ny,nx) float32 and, with colour, color
(3,nz,ny,nx) float32, planar.  All of it starts at zero.  nx ny nz < 2^31.

Integration of one view (integrate_numpy): depth d (H,W), intrinsics K, world-to-view pose T, an optional per-pixel weight map w (H,W),
1 by default, and an optional image (3,H,W).
  1. The host composes in float64 M = K T[:3] [[s I, origin], [0, 1]], the 3x4 matrix that takes (i,j,k,1) to (Qx,Qy,Qz), and hands
     its 12 values to the device as float32.
  2. The voxel is skipped unless Qz > 0.
  3. u = Qx / Qz, v = Qy / Qz; px = rint(u), py = rint(v), half to even; skipped unless 0 <= px <= W-1 and 0 <= py <= H-1.
  4. dm = d[py,px], wm = w[py,px]; skipped unless dm is finite and > 0 and wm is finite and > 0.
  5. sdf = dm - Qz, projective along the view's z axis; skipped if sdf < -trunc.  f = min(1, sdf / trunc).
  6. W' = W + wm;  F' = (F W + f wm) / W';  C' = (C W + c wm) / W' per channel, when the volume has colour and an image is given;
     then W' = min(W', max_weight) when max_weight is set.
A skipped voxel keeps its bits.  Views are applied in list order, and the result is by definition that of applying them one at a
time.  trunc defaults to 3 s.

Extraction (extract_numpy): marching tetrahedra on the Kuhn subdivision of every cell.
  A voxel is OBSERVED when weight >= min_weight (default 1.0) and INSIDE when tsdf < 0.  tsdf == 0 counts as outside: that puts
  vertices on grid corners and yields zero-area triangles; they are not special-cased, welded or removed.
  Edge kinds 0..6, from the owner voxel p to p + delta: delta = (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1).
  Vertices.  An edge carries a vertex iff both endpoints are in the grid, both are observed and exactly one is inside.  With a the
  owner and b the other end, t = Fa / (Fa - Fb), position = origin + s (p + t delta), colour = Ca + t (Cb - Ca).  Vertices are ordered
  by (the owner's linear index (k ny + j) nx + i, kind).
  Cells (i,j,k) with i < nx-1, j < ny-1, k < nz-1 contribute iff all 8 corners are observed.  A cell is cut into 6 tetrahedra: for the
  permutations (a,b,c) of the axes (0,1,2) in lexicographic order, v0 = 0, v1 = e_a, v2 = e_a + e_b, v3 = (1,1,1).  Per tetrahedron
  the inside mask m has bit n set when v_n is inside; m = 0 and m = 15 give nothing.  A lone vertex l (the one inside, or the one
  outside) with the other three p < q < r in tetra-local order gives the triangle (e(l,p), e(l,q), e(l,r)).  Two inside a < b and two
  outside c < d give (e(a,c), e(a,d), e(b,d)) and then (e(a,c), e(b,d), e(b,c)).  e(x,y) is the vertex on that edge of the
  tetrahedron; every such edge is one of the 7 kinds, owned by its lower endpoint.
  Orientation.  With the triangle's vertices placed at the edge midpoints of the unit cell, n = (p1 - p0) x (p2 - p0); the last two
  indices are swapped when n . (mean of the outside corners of the tetrahedron - mean of the inside ones) < 0, so that every normal
  points out of the surface.  The rule is a table per (tetrahedron, m): tri_table() here, and csrc/tsdf_tables.h for the kernel,
  which kernel_tables_header() writes from the same table (python -m robustmvd_amd.tsdf > robustmvd_amd/csrc/tsdf_tables.h).
  Triangles are ordered by (the cell's linear index, tetrahedron, slot).  The result is vertices (M,3) float32, triangles (T,3) int32
  and colors (M,3) or None.  A vertex that no triangle references can occur, on an edge none of whose cells is fully observed; it
  stays: the vertex list is also the volume's surface point cloud.

Two implementations: integrate_numpy / extract_numpy on the host and the HIP kernels of csrc/tsdf.hip (ops.tsdf_integrate,
ops.tsdf_extract) for a volume on a GPU.  TSDFVolume picks by its `device`.
"""
import functools
import itertools

import numpy as np

from .depth_fusion import map2d, pinhole
from .mesh import Mesh, is_tensor, one_place, place, to_numpy  # noqa: F401  (tsdf.Mesh stays importable)

MAX_VIEWS = 32  # views per launch (MVD_MAX_VIEWS)
EDGE_KINDS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
# the four corners (dx,dy,dz) of each of the six tetrahedra of a cell
TETRAHEDRA = tuple(((0, 0, 0), tuple(int(n == a) for n in range(3)), tuple(int(n in (a, b)) for n in range(3)), (1, 1, 1))
                   for a, b, _ in itertools.permutations(range(3)))


def case_triangles(m):
    """The triangles of inside mask m before orientation: each a triple of tetra-local vertex pairs (the edges they sit on)."""
    inside = [n for n in range(4) if (m >> n) & 1]
    outside = [n for n in range(4) if not (m >> n) & 1]
    if not inside or not outside:
        return []
    if len(inside) == 1 or len(outside) == 1:
        lone = (inside if len(inside) == 1 else outside)[0]
        p, q, r = [n for n in range(4) if n != lone]
        return [((lone, p), (lone, q), (lone, r))]
    (a, b), (c, d) = inside, outside
    return [((a, c), (a, d), (b, d)), ((a, c), (b, d), (b, c))]


def flip_bit(tet, m, tri):
    """The orientation rule of the module docstring for one triangle of tetrahedron `tet` (its four corners) under mask m."""
    corners = np.asarray(tet, dtype=np.float64)
    p = [(corners[x] + corners[y]) / 2 for x, y in tri]
    inside = [n for n in range(4) if (m >> n) & 1]
    outside = [n for n in range(4) if not (m >> n) & 1]
    outward = corners[outside].mean(axis=0) - corners[inside].mean(axis=0)
    return bool(np.dot(np.cross(p[1] - p[0], p[2] - p[0]), outward) < 0)


@functools.lru_cache(maxsize=None)
def tri_table():
    """[tetrahedron][m] -> the oriented triangles, each three (owner corner (dx,dy,dz), kind): the vertex on the edge of that kind
    owned by the cell's corner voxel at that offset."""
    table = []
    for tet in TETRAHEDRA:
        row = []
        for m in range(16):
            tris = []
            for tri in case_triangles(m):
                if flip_bit(tet, m, tri):
                    tri = (tri[0], tri[2], tri[1])
                edges = []
                for x, y in tri:
                    lo, hi = tet[min(x, y)], tet[max(x, y)]  # the corners of a tetrahedron ascend along its path
                    edges.append((lo, EDGE_KINDS.index(tuple(h - l for h, l in zip(hi, lo)))))
                tris.append(tuple(edges))
            row.append(tuple(tris))
        table.append(tuple(row))
    return tuple(table)


def flip_table():
    """(6,16) uint8: bit `slot` set where the orientation rule swaps triangle `slot` of (tetrahedron, m)."""
    out = np.zeros((6, 16), dtype=np.uint8)
    for t, tet in enumerate(TETRAHEDRA):
        for m in range(16):
            for slot, tri in enumerate(case_triangles(m)):
                out[t, m] |= int(flip_bit(tet, m, tri)) << slot
    return out


def kernel_tables_header():
    """The text of csrc/tsdf_tables.h: tri_table() packed for the kernel.  One 32-bit word per triangle; vertex n takes bits
    6n .. 6n+5: the owner corner dx | dy << 1 | dz << 2, then the kind << 3.  A (tetrahedron, m) has popcount-many triangles: 0 for
    m = 0 and 15, 2 for two bits set, else 1."""
    lines = ["// Written by robustmvd_amd/tsdf.py (python -m robustmvd_amd.tsdf > robustmvd_amd/csrc/tsdf_tables.h) from tri_table(), the",
             "// orientation rule of that module's docstring; tests/test_tsdf_cpu.py compares this file with the generator.  Do not edit.",
             "// TSDF_TRI[tetrahedron][inside mask][slot]: vertex n in bits 6n .. 6n+5 = owner corner (dx | dy << 1 | dz << 2) | kind << 3.",
             "#pragma once",
             "namespace mvd {",
             "static __device__ const unsigned TSDF_TRI[6][16][2] = {"]
    for row in tri_table():
        words = []
        for tris in row:
            w = [0, 0]
            for slot, tri in enumerate(tris):
                for n, ((dx, dy, dz), kind) in enumerate(tri):
                    w[slot] |= (dx | dy << 1 | dz << 2 | kind << 3) << (6 * n)
            words.append("{0x%05xu, 0x%05xu}" % tuple(w))
        lines.append("    {" + ", ".join(words[:8]) + ",")
        lines.append("     " + ", ".join(words[8:]) + "},")
    lines += ["};", "}  // namespace mvd", ""]
    return "\n".join(lines)


def compose_matrix(K, T, origin, voxel):
    """-> 12 float64, row-major 3x4: M = K T[:3] [[s I, origin], [0, 1]], which takes (i,j,k,1) to (Qx,Qy,Qz)."""
    K, T = pinhole(K, "intrinsics"), np.asarray(T, dtype=np.float64).reshape(4, 4)
    G = np.eye(4)
    G[:3, :3] *= float(voxel)
    G[:3, 3] = np.asarray(origin, dtype=np.float64).reshape(3)
    return (K @ T[:3] @ G).ravel()


def _check_state(tsdf, weight, color):
    if tsdf.ndim != 3 or weight.shape != tsdf.shape:
        raise ValueError(f"tsdf must be (nz,ny,nx) and weight of its shape, got {tuple(tsdf.shape)} and {tuple(weight.shape)}")
    if color is not None and tuple(color.shape) != (3,) + tuple(tsdf.shape):
        raise ValueError(f"color: shape {tuple(color.shape)}, expected {(3,) + tuple(tsdf.shape)}")
    if int(np.prod(tsdf.shape, dtype=np.int64)) >= 2 ** 31:
        raise ValueError(f"volume {tuple(tsdf.shape)}: nx ny nz must be below 2^31")


def integrate_numpy(tsdf, weight, color, depths, intrinsics, poses, origin, voxel, trunc=None, max_weight=None, weights=None,
                    images=None, dtype=np.float64, details=False):
    """The integration of the module docstring as a numpy chain: the views are applied to (tsdf, weight, color) in list order.
    Returns new arrays (tsdf, weight, color or None) of `dtype`; the arguments are not changed.  color may be None.  Views of
    different sizes may be mixed.  dtype=np.float32 evaluates the same chain in float32 on the float32-rounded matrices (what the
    device is handed): the gap between the two is what tests/tsdf_cases.py derives its bands from.  details=True adds a fourth
    result, a dict of per-view arrays (V,nz,ny,nx): u, v, qz, sdf (dm - Qz where the pixel is in bounds, else NaN), px, py (int64, 0
    where out of bounds), inb (Qz > 0 and the pixel in bounds) and updated."""
    ft = np.dtype(dtype).type
    F, Wt = np.array(tsdf, dtype=ft), np.array(weight, dtype=ft)
    C = None if color is None else np.array(color, dtype=ft)
    _check_state(F, Wt, C)
    V = len(depths)
    if not (len(intrinsics) == len(poses) == V):
        raise ValueError(f"{V} depth maps, {len(intrinsics)} intrinsics, {len(poses)} poses")
    for name, opt in (("weights", weights), ("images", images)):
        if opt is not None and len(opt) != V:
            raise ValueError(f"{len(opt)} {name} for {V} views")
    s = float(voxel)
    trunc = ft(3.0 * s if trunc is None else trunc)
    if not trunc > 0:
        raise ValueError(f"trunc must be positive, got {trunc}")
    nz, ny, nx = F.shape
    k, j, i = np.meshgrid(np.arange(nz, dtype=ft), np.arange(ny, dtype=ft), np.arange(nx, dtype=ft), indexing="ij")
    det = {n: [] for n in ("u", "v", "qz", "sdf", "px", "py", "inb", "updated")}
    one = ft(1)
    for n in range(V):
        d = np.asarray(to_numpy(depths[n])).astype(ft)
        if d.ndim != 2:
            raise ValueError(f"depths[{n}] must be (H,W), got {d.shape}")
        H, W = d.shape
        w = np.ones((H, W), dtype=ft) if weights is None else np.asarray(to_numpy(weights[n])).astype(ft)
        if w.shape != d.shape:
            raise ValueError(f"weights[{n}]: shape {w.shape}, expected {d.shape}")
        img = None
        if images is not None and C is not None:
            img = np.asarray(to_numpy(images[n])).astype(ft)
            if img.shape != (3, H, W):
                raise ValueError(f"images[{n}]: shape {img.shape}, expected {(3, H, W)}")
        m = compose_matrix(intrinsics[n], poses[n], origin, s)
        m = (m.astype(np.float32) if ft is np.float32 else m).astype(ft)
        with np.errstate(all="ignore"):
            q = [m[4 * r] * i + m[4 * r + 1] * j + m[4 * r + 2] * k + m[4 * r + 3] for r in range(3)]
            u, v = q[0] / q[2], q[1] / q[2]
            px, py = np.rint(u), np.rint(v)
            inb = (q[2] > 0) & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
            ix, iy = np.where(inb, px, 0).astype(np.int64), np.where(inb, py, 0).astype(np.int64)
            dm, wm = d[iy, ix], w[iy, ix]
            sdf = dm - q[2]
            upd = inb & np.isfinite(dm) & (dm > 0) & np.isfinite(wm) & (wm > 0) & ~(sdf < -trunc)
            f = np.minimum(one, sdf / trunc)
            Wn = Wt + wm
            F = np.where(upd, (F * Wt + f * wm) / Wn, F)
            if img is not None:
                for c in range(3):
                    C[c] = np.where(upd, (C[c] * Wt + img[c][iy, ix] * wm) / Wn, C[c])
            if max_weight is not None:
                Wn = np.minimum(Wn, ft(max_weight))
            Wt = np.where(upd, Wn, Wt)
        if details:
            for name, a in (("u", u), ("v", v), ("qz", q[2]), ("sdf", np.where(inb, sdf, ft(np.nan))), ("px", ix), ("py", iy),
                            ("inb", inb), ("updated", upd)):
                det[name].append(a)
    if details:
        return F, Wt, C, {n: np.stack(a) if a else np.zeros((0, nz, ny, nx)) for n, a in det.items()}
    return F, Wt, C


def extract_numpy(tsdf, weight, color=None, origin=(0.0, 0.0, 0.0), voxel=1.0, min_weight=1.0, dtype=np.float64):
    """The extraction of the module docstring as a numpy chain -> (vertices (M,3), colors (M,3) or None, triangles (T,3) int32).
    The observed and inside verdicts are taken on the float32 state as it is; t, the positions and the colours are formed in `dtype`
    (float32: on the float32-rounded origin and voxel, what the device is handed)."""
    ft = np.dtype(dtype).type
    F32, W32 = np.asarray(to_numpy(tsdf), dtype=np.float32), np.asarray(to_numpy(weight), dtype=np.float32)
    C = None if color is None else np.asarray(to_numpy(color), dtype=np.float32).astype(ft)
    _check_state(F32, W32, C)
    nz, ny, nx = F32.shape
    N = nx * ny * nz
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    o = (o.astype(np.float32) if ft is np.float32 else o).astype(ft)
    s = ft(np.float32(voxel)) if ft is np.float32 else ft(voxel)
    with np.errstate(invalid="ignore"):
        obs, ins = W32 >= np.float32(min_weight), F32 < 0
    F = F32.astype(ft)

    has = np.zeros((nz, ny, nx, 7), dtype=bool)
    for q, (dx, dy, dz) in enumerate(EDGE_KINDS):
        a = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        b = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        has[a + (q,)] = obs[a] & obs[b] & (ins[a] != ins[b])
    has = has.reshape(N, 7)
    lin, kind = np.nonzero(has)  # row-major: by (owner's linear index, kind)
    vid = (np.cumsum(has.ravel(), dtype=np.int64) - 1).reshape(N, 7)
    if len(lin) >= 2 ** 31:
        raise ValueError(f"{len(lin)} vertices: the mesh must have fewer than 2^31")
    idx = [lin % nx, (lin // nx) % ny, lin // (nx * ny)]
    delta = np.asarray(EDGE_KINDS, dtype=np.int64)[kind]
    other = lin + (delta[:, 2] * ny + delta[:, 1]) * nx + delta[:, 0]
    Fa, Fb = F.ravel()[lin], F.ravel()[other]
    t = Fa / (Fa - Fb)
    vertices = np.stack([o[c] + s * (idx[c].astype(ft) + t * delta[:, c].astype(ft)) for c in range(3)], axis=1).reshape(-1, 3)
    colors = None
    if C is not None:
        Cf = C.reshape(3, N)
        colors = np.stack([Cf[c][lin] + t * (Cf[c][other] - Cf[c][lin]) for c in range(3)], axis=1).reshape(-1, 3)

    keys, tris = [np.zeros(0, dtype=np.int64)], [np.zeros((0, 3), dtype=np.int64)]
    cz, cy, cx = nz - 1, ny - 1, nx - 1
    if min(cz, cy, cx) > 0:
        corner = lambda d: (slice(d[2], d[2] + cz), slice(d[1], d[1] + cy), slice(d[0], d[0] + cx))
        full = np.ones((cz, cy, cx), dtype=bool)
        for d in itertools.product((0, 1), repeat=3):
            full &= obs[corner(d)]
        cell = np.arange(N, dtype=np.int64).reshape(nz, ny, nx)[:cz, :cy, :cx]
        table = tri_table()
        for tn, tet in enumerate(TETRAHEDRA):
            m = np.zeros((cz, cy, cx), dtype=np.int64)
            for n in range(4):
                m |= ins[corner(tet[n])].astype(np.int64) << n
            m[~full] = 0
            for mv in range(1, 15):
                at = cell[m == mv]
                if not len(at):
                    continue
                for slot, tri in enumerate(table[tn][mv]):
                    tris.append(np.stack([vid[at + (dz * ny + dy) * nx + dx, q] for (dx, dy, dz), q in tri], axis=1))
                    keys.append((at * 6 + tn) * 2 + slot)
    order = np.argsort(np.concatenate(keys), kind="stable")
    triangles = np.concatenate(tris)[order]
    if len(triangles) >= 2 ** 31:
        raise ValueError(f"{len(triangles)} triangles: the mesh must have fewer than 2^31")
    return vertices, colors, triangles.astype(np.int32)


def bounds_from_points(points, voxel, margin=0.0):
    """-> (origin (3,) float64, dims (nx,ny,nz)) of the smallest volume of edge `voxel`, its origin on the voxel lattice through 0,
    that holds every finite point of the (M,3) cloud (DepthFusion's, for one) with `margin` around it."""
    p = np.asarray(to_numpy(points), dtype=np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    if not len(p):
        raise ValueError("bounds_from_points: no finite point")
    if not voxel > 0 or margin < 0:
        raise ValueError(f"bounds_from_points: voxel {voxel} must be positive and margin {margin} non-negative")
    lo = np.floor((p.min(axis=0) - margin) / voxel)
    hi = np.ceil((p.max(axis=0) + margin) / voxel)
    return lo * voxel, tuple(int(n) for n in (hi - lo + 1))


class TSDFVolume:
    """A dense TSDF volume (module docstring) on the host (device=None: the numpy forms) or on one GPU (the HIP kernels).

        origin, dims = bounds_from_points(cloud.points, 0.01, margin=0.05)
        volume = TSDFVolume(origin, 0.01, dims, color=True, device="cuda")
        volume.integrate(depths, intrinsics, poses, images=images)
        mesh = volume.extract_mesh()
        write_ply("scene.ply", mesh.vertices, mesh.colors, faces=mesh.triangles)

    The state arrays are the attributes tsdf, weight (nz,ny,nx) and color (3,nz,ny,nx) or None: float32 numpy arrays on the host, GPU
    tensors on a GPU."""

    def __init__(self, origin, voxel, dims, trunc=None, max_weight=None, color=False, device=None):
        self._setup(origin, voxel, trunc, max_weight, device)
        nx, ny, nz = (int(n) for n in dims)
        if min(nx, ny, nz) < 1:
            raise ValueError(f"dims {tuple(dims)}: every dimension must be at least 1")
        if nx * ny * nz >= 2 ** 31:  # before anything is allocated
            raise ValueError(f"dims {(nx, ny, nz)}: nx ny nz = {nx * ny * nz} must be below 2^31")
        shape = (nz, ny, nx)
        if self.device is None:
            zeros = lambda sh: np.zeros(sh, dtype=np.float32)
        else:
            import torch
            zeros = lambda sh: torch.zeros(sh, dtype=torch.float32, device=self.device)
        self.tsdf, self.weight = zeros(shape), zeros(shape)
        self.color = zeros((3,) + shape) if color else None

    def _setup(self, origin, voxel, trunc, max_weight, device):
        self.origin = np.asarray(origin, dtype=np.float64).reshape(3).copy()
        self.voxel = float(voxel)
        if not self.voxel > 0 or not np.isfinite(self.origin).all():
            raise ValueError(f"voxel {voxel} must be positive and origin {self.origin.tolist()} finite")
        self.trunc = 3.0 * self.voxel if trunc is None else float(trunc)
        if not self.trunc > 0:
            raise ValueError(f"trunc must be positive, got {trunc}")
        self.max_weight = None if max_weight is None else float(max_weight)
        if self.max_weight is not None and not self.max_weight > 0:
            raise ValueError(f"max_weight must be positive, got {max_weight}")
        self.device = None
        if device is not None and str(device) != "cpu":
            import torch
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise ValueError(f"device {device}: a volume lives on the host (None) or on a cuda (ROCm) device")
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())

    @classmethod
    def from_arrays(cls, tsdf, weight, color=None, origin=(0.0, 0.0, 0.0), voxel=1.0, trunc=None, max_weight=None):
        """A volume around existing state: numpy arrays give a host volume (float32 copies), GPU tensors one on their device (taken
        as they are where they are contiguous float32)."""
        arrays = [a for a in (tsdf, weight, color) if a is not None]
        where = one_place(*arrays, what="state arrays")
        self = cls.__new__(cls)
        self._setup(origin, voxel, trunc, max_weight, None if where == "host" else where)
        _check_state(tsdf, weight, color)
        if self.device is None:
            take = lambda a: np.array(to_numpy(a), dtype=np.float32)
        else:
            import torch
            take = lambda a: a.to(torch.float32).contiguous()
        self.tsdf, self.weight = take(tsdf), take(weight)
        self.color = None if color is None else take(color)
        return self

    @property
    def dims(self):
        nz, ny, nx = self.tsdf.shape
        return int(nx), int(ny), int(nz)

    def integrate(self, depths, intrinsics, poses, weights=None, images=None):
        """Applies the views in list order.  depths: N x (H,W) (or (1,H,W), (1,1,H,W)); intrinsics N x (3,3); poses N x (4,4)
        world-to-view; weights: N x (H,W) per-pixel weights (uint8 masks are taken as 0 / 1 weights) or None; images: N x (3,H,W)
        or None (read only by a volume with colour).  numpy arrays or torch tensors.  A volume on a GPU runs consecutive views of
        one size in launches of up to 32 views; maps on the host are uploaded to it, maps on another device raise.  A volume on the
        host takes host maps only."""
        N = len(depths)
        if not (len(intrinsics) == len(poses) == N):
            raise ValueError(f"{N} depth maps, {len(intrinsics)} intrinsics, {len(poses)} poses")
        for name, opt in (("weights", weights), ("images", images)):
            if opt is not None and len(opt) != N:
                raise ValueError(f"{len(opt)} {name} for {N} views")
        if N == 0:
            return self
        Ks = [to_numpy(K).astype(np.float64).reshape(3, 3) for K in intrinsics]
        Ts = [to_numpy(T).astype(np.float64).reshape(4, 4) for T in poses]
        depths = [map2d(d, f"depths[{i}]") for i, d in enumerate(depths)]
        weights = None if weights is None else [map2d(w, f"weights[{i}]") for i, w in enumerate(weights)]
        mine = "host" if self.device is None else str(self.device)
        for name, maps in (("depths", depths), ("weights", weights), ("images", images)):
            for i, a in enumerate(maps or []):
                if place(a) not in ("host", mine):
                    raise ValueError(f"{name}[{i}] is on {place(a)}, the volume on {mine}: move the maps to the volume's device first")
        for i, d in enumerate(depths):
            if weights is not None and tuple(weights[i].shape) != tuple(d.shape):
                raise ValueError(f"weights[{i}]: shape {tuple(weights[i].shape)}, expected {tuple(d.shape)}")
            if images is not None and tuple(images[i].shape) != (3,) + tuple(d.shape):
                raise ValueError(f"images[{i}]: shape {tuple(images[i].shape)}, expected {(3,) + tuple(d.shape)}")
        if self.device is None:
            # one view at a time, the float32 state between them: the result does not depend on how the views are split into calls
            for i in range(N):
                F, W, C = integrate_numpy(self.tsdf, self.weight, self.color, depths[i:i + 1], Ks[i:i + 1], Ts[i:i + 1], self.origin,
                                          self.voxel, self.trunc, self.max_weight, None if weights is None else weights[i:i + 1],
                                          images[i:i + 1] if images is not None and self.color is not None else None)
                self.tsdf, self.weight = F.astype(np.float32), W.astype(np.float32)
                self.color = None if C is None else C.astype(np.float32)
            return self
        import torch
        from . import ops
        up = lambda a: (a if is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(self.device)
        table = torch.from_numpy(np.stack([compose_matrix(Ks[i], Ts[i], self.origin, self.voxel) for i in range(N)])
                                 .astype(np.float32)).to(self.device)
        use_images = images is not None and self.color is not None
        start = 0
        while start < N:
            stop = start + 1
            while stop < N and stop - start < MAX_VIEWS and tuple(depths[stop].shape) == tuple(depths[start].shape):
                stop += 1
            ops.tsdf_integrate(self.tsdf, self.weight, self.color, [up(d) for d in depths[start:stop]], table[start:stop],
                               self.trunc, self.max_weight,
                               None if weights is None else [up(w) for w in weights[start:stop]],
                               [up(im) for im in images[start:stop]] if use_images else None)
            start = stop
        return self

    def integrate_fusion(self, result, intrinsics, poses, images=None):
        """Integrates a FusionResult: every view's fused_depth with its mask as the weights, so that only the pixels that passed
        the consistency check count."""
        return self.integrate(result.fused_depth, intrinsics, poses, weights=result.mask, images=images)

    def extract_mesh(self, min_weight=1.0, clean=None, simplify=None):
        """-> Mesh: the surface between the observed voxels (weight >= min_weight), module docstring.  clean: None, or a dict of
        mesh_clean.clean_mesh's keywords min_triangles, min_area, keep_largest and remove_unreferenced, applied to the mesh; any
        other keyword raises, so that the result is always a Mesh (for attributes or the remaps call mesh.clean yourself).
        simplify: None, or a dict of mesh_simplify.simplify_mesh's keywords cell (required), placement, regularisation, origin,
        unique and remove_unreferenced, applied after clean."""
        extra = set(clean or ()) - {"min_triangles", "min_area", "keep_largest", "remove_unreferenced"}
        if extra:
            raise ValueError(f"extract_mesh: clean takes min_triangles, min_area, keep_largest and remove_unreferenced, got {sorted(extra)}")
        if simplify is not None:
            extra = set(simplify) - {"cell", "placement", "regularisation", "origin", "unique", "remove_unreferenced"}
            if extra or "cell" not in simplify:
                raise ValueError("extract_mesh: simplify takes cell (required), placement, regularisation, origin, unique and "
                                 f"remove_unreferenced, got {sorted(simplify)}")
        if self.device is None:
            v, c, t = extract_numpy(self.tsdf, self.weight, self.color, self.origin, self.voxel, min_weight)
            mesh = Mesh(v.astype(np.float32), t, None if c is None else c.astype(np.float32))
        else:
            from . import ops
            v, t, c = ops.tsdf_extract(self.tsdf, self.weight, self.color, self.origin, self.voxel, min_weight)
            mesh = Mesh(v, t, c)
        if clean is not None:
            mesh = mesh.clean(**clean)
        return mesh if simplify is None else mesh.simplify(**simplify)

    def render(self, intrinsics, poses, size, min_weight=1.0, **kw):
        """-> RenderResult: extract_mesh(min_weight).render(...), the volume's surface seen from V views: per view the denoised and
        hole-filled depth map with, on request, a normal and a colour per pixel."""
        return self.extract_mesh(min_weight).render(intrinsics, poses, size, **kw)


if __name__ == "__main__":
    print(kernel_tables_header(), end="")
