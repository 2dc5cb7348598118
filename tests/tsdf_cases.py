"""Cases for the TSDF tests (test_tsdf_cpu.py, test_hip_tsdf.py): the scenes of fusion_cases.py integrated into a small volume, the
reference for the device test derived from integrate_numpy alone, analytic sphere volumes and the mesh checks both tests share.
Everything is built once (treat the arrays as read-only).

All five views of a scene go into a volume with origin (-1.4, -1.0, 2.2): voxel 0.1 and dims (29,21,25) for the 37 x 53 maps, voxel
0.05 and dims (57,41,47) for the 96 x 131 maps, trunc = 3 voxel.  The odd nx gives ragged rows, a volume size that is no multiple of
four (so the colour planes are not 16-byte aligned) and a partial last chunk.
"""
import functools

import numpy as np

import fusion_cases as FC
from robustmvd_amd import tsdf as TS

ORIGIN = (-1.4, -1.0, 2.2)
VOLUMES = {FC.SIZES[0]: (0.1, (29, 21, 25)), FC.SIZES[1]: (0.05, (57, 41, 47))}
MAX_EXCLUDED_SHARE = 0.01


def volume_of(H, W):
    """-> (voxel, dims (nx,ny,nz), trunc)"""
    voxel, dims = VOLUMES[(H, W)]
    return voxel, dims, 3 * voxel


def zeros(dims, color=True):
    nx, ny, nz = dims
    return (np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32),
            np.zeros((3, nz, ny, nx), np.float32) if color else None)


VARIANTS = (None, "masks", "max_weight", "holes", "facing_away")


@functools.lru_cache(maxsize=None)
def inputs(name, H, W, variant=None):
    """-> dict(depths, Ks, Ts, images, weights, max_weight) of a scene's five views.  Variants: "masks": every view's consistency mask
    (fuse_numpy against the other four) as its weight map; "max_weight": a cap of 2; "holes": patches of 0, NaN, inf and negative
    depth in four of the maps (placed for the 37 x 53 size); "facing_away": view 1 turned by half a turn about its y axis, so that the volume is behind it."""
    assert variant in VARIANTS
    sc = FC.scene(name, H, W)
    out = {"depths": list(sc["depths"]), "Ks": sc["Ks"], "Ts": list(sc["Ts"]), "images": sc["images"], "weights": None, "max_weight": None}
    if variant == "masks":
        out["weights"] = [FC.reference(name, H, W, key)["f64"]["mask"] for key in range(5)]
    elif variant == "max_weight":
        out["max_weight"] = 2.0
    elif variant == "holes":
        for i, (bad, rows, cols) in enumerate(((0.0, slice(3, 12), slice(5, 20)), (np.nan, slice(10, 25), slice(20, 41)),
                                               (np.inf, slice(0, 9), slice(30, 53)), (-1.5, slice(20, 30), slice(2, 17)))):
            d = out["depths"][i].copy()
            d[rows, cols] = bad
            out["depths"][i] = d
    elif variant == "facing_away":
        out["Ts"][1] = np.diag([-1.0, 1.0, -1.0, 1.0]) @ out["Ts"][1]
    return out


@functools.lru_cache(maxsize=None)
def reference(name, H, W, variant=None):
    """integrate_numpy in float64 and the same chain in float32 on the float32-rounded matrices, with colour, and what the device test
    derives from the two alone: the largest gaps in u, v and Qz over the voxels in bounds in both, the bands (four times each gap: the
    kernel's chain may contract to FMAs, order its operations differently and use a 1-ulp reciprocal, each of the order of one more
    float32 rounding of the same chain), the voxels excluded from the comparison, and the gaps in F and colour on the rest.  A voxel
    is excluded when for some view the fractional part of u or v is within the band of 1/2 with the pixel within one pixel of the
    image (which covers the border tests px >= 0 and px <= W-1: they are decided at half-integer u), |Qz| is within its band of 0,
    sdf + trunc is within Qz's band of 0, or the two numpy chains disagree on the pixel or on the update verdict."""
    sc = inputs(name, H, W, variant)
    voxel, dims, trunc = volume_of(H, W)
    args = (*zeros(dims), sc["depths"], sc["Ks"], sc["Ts"], ORIGIN, voxel, trunc, sc["max_weight"], sc["weights"], sc["images"])
    F64, W64, C64, d64 = TS.integrate_numpy(*args, details=True)
    F32, W32, C32, d32 = TS.integrate_numpy(*args, dtype=np.float32, details=True)
    both = d64["inb"] & d32["inb"]
    gap = {k: float(np.abs(d64[k] - d32[k])[both].max()) for k in ("u", "v", "qz")}
    band = {k: 4.0 * g for k, g in gap.items()}
    with np.errstate(invalid="ignore"):
        near_image = ((d64["u"] >= -1.5) & (d64["u"] <= W + 0.5) & (d64["v"] >= -1.5) & (d64["v"] <= H + 0.5))
        half = lambda a, b: np.abs(a - np.floor(a) - 0.5) <= b
        excluded = (near_image & (half(d64["u"], band["u"]) | half(d64["v"], band["v"]))) | (np.abs(d64["qz"]) <= band["qz"])
        excluded |= np.abs(d64["sdf"] + trunc) <= band["qz"]  # NaN (out of bounds): false
    excluded |= (d64["inb"] != d32["inb"]) | (d64["px"] != d32["px"]) | (d64["py"] != d32["py"]) | (d64["updated"] != d32["updated"])
    excluded = excluded.any(axis=0)
    keep = ~excluded
    span = float(max(im.max() for im in sc["images"]) - min(im.min() for im in sc["images"]))
    gap["F"] = float(np.abs(F64 - F32)[keep].max())
    gap["C"] = float(np.abs(C64 - C32)[:, keep].max()) / span
    band["F"], band["C"] = 4.0 * gap["F"], 4.0 * gap["C"]
    observed = W64 >= 1
    return {"F": F64, "W": W64, "C": C64, "F32": F32, "W32": W32, "d64": d64, "d32": d32, "gap": gap, "band": band, "excluded": excluded,
            "share": float(excluded.mean()), "w_equal": bool(np.array_equal(W64[keep], W32[keep])), "span": span,
            "observed": float(observed.mean()), "inside": float((F64 < 0)[observed].mean()),
            "skipped_by_all": ~(d64["updated"].any(axis=0) | d32["updated"].any(axis=0))}


# ---- analytic volumes --------------------------------------------------------------------------------------------------------------
SPHERE = (18, (8.3, 8.6, 8.9), 5.2)  # grid, centre, radius: 1502 vertices, 3000 triangles, 4500 edges; with i < 9 observed 746 / 1418


@functools.lru_cache(maxsize=None)
def sphere_volume(n=SPHERE[0], centre=SPHERE[1], radius=SPHERE[2], observed_below_i=None):
    """-> (tsdf, weight) (n,n,n) float32: the signed distance to the sphere in voxel units, weight 1 (0 where i >= observed_below_i)"""
    k, j, i = np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij")
    F = (np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2) - radius).astype(np.float32)
    Wt = np.ones_like(F)
    if observed_below_i is not None:
        Wt[:, :, observed_below_i:] = 0
    return F, Wt


def directed_edges(triangles):
    t = np.asarray(triangles, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def edge_counts(triangles):
    """-> (the undirected edges (E,2), how many triangles hold each, whether some directed edge occurs twice)"""
    e = directed_edges(triangles)
    und, counts = np.unique(np.sort(e, axis=1), axis=0, return_counts=True)
    return und, counts, len(np.unique(e, axis=0)) != len(e)


def check_closed_surface(vertices, triangles, centre):
    """A watertight, consistently oriented sphere-like surface: every undirected edge in exactly two triangles, once per direction,
    Euler characteristic 2, every normal pointing away from `centre`, no unreferenced vertex."""
    v, t = np.asarray(vertices, dtype=np.float64), np.asarray(triangles, dtype=np.int64)
    und, counts, repeated = edge_counts(t)
    assert (counts == 2).all() and not repeated
    assert len(v) - len(und) + len(t) == 2
    p = v[t]
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert ((normal * (p.mean(axis=1) - np.asarray(centre))).sum(axis=1) > 0).all()
    assert len(np.unique(t)) == len(v)


def extract_reference(tsdf, weight, color=None, origin=(0.0, 0.0, 0.0), voxel=1.0, min_weight=1.0):
    """extract_numpy in float64 and float32 on one float32 volume -> (vertices64, colors64, triangles, vertex band, colour band): the
    bands are four times the largest float64-float32 gap of the positions and of the colours (the triangles and the counts are equal
    in both, which is asserted)."""
    v64, c64, t64 = TS.extract_numpy(tsdf, weight, color, origin, voxel, min_weight)
    v32, c32, t32 = TS.extract_numpy(tsdf, weight, color, origin, voxel, min_weight, dtype=np.float32)
    assert v32.dtype == np.float32 and np.array_equal(t64, t32) and v64.shape == v32.shape
    vband = 4.0 * float(np.abs(v64 - v32).max()) if len(v64) else 0.0
    cband = 4.0 * float(np.abs(c64 - c32).max()) if c64 is not None and len(c64) else 0.0
    return v64, c64, t64, vband, cband
