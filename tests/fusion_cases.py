"""Analytic scenes for the depth-fusion tests (test_depth_fusion_cpu.py, test_hip_depth_fusion.py).  Depth is the closed-form
ray-plane intersection, nearest hit, 0 where nothing is hit; every scene is built once and shared (treat the arrays as read-only).

  scene A   background plane n = (0.05, -0.1, 1), n.X = 4, and an occluding patch z = 2.6 over world x in (-0.5, 0.4), y in (-0.3, 0.5);
            multiplicative Gaussian depth noise, sigma = 0.004, fixed seed, so that a useful share of the pairs lands near both thresholds
  scene B   the background plane alone, noise-free
Five cameras with one K: f = 1.1 W, fy = 1.02 f, c = (W/2 - 0.3, H/2 + 0.4); rotations of a few hundredths of a radian about x and y,
camera centres 0.25-0.35 from the first one.  Maps are float32.
"""
import functools

import numpy as np

from robustmvd_amd import depth_fusion as DF

SIZES = ((37, 53), (96, 131))  # odd with partial tiles and a partial wave; several workgroups with a ragged last tile both ways
PLANE_N, PLANE_D = np.array([0.05, -0.1, 1.0]), 4.0
PATCH_Z, PATCH_X, PATCH_Y = 2.6, (-0.5, 0.4), (-0.3, 0.5)
NOISE_SIGMA, NOISE_SEED = 0.004, 20240607
# (rotation about x, rotation about y, camera centre) per camera
CAMERAS = ((0.0, 0.0, (0.0, 0.0, 0.0)),
           (0.02, -0.03, (0.30, 0.02, 0.01)),
           (-0.025, 0.035, (-0.28, 0.05, -0.02)),
           (0.03, 0.015, (0.04, 0.27, 0.03)),
           (-0.015, -0.02, (-0.10, -0.32, 0.02)))


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float64)


def pose(R, centre):
    """world-to-view [R | -R C]"""
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ np.asarray(centre, dtype=np.float64)
    return T


def intrinsics(H, W):
    f = 1.1 * W
    return np.array([[f, 0, W / 2 - 0.3], [0, 1.02 * f, H / 2 + 0.4], [0, 0, 1]], dtype=np.float64)


def poses():
    return [pose(rot_x(ax) @ rot_y(ay), c) for ax, ay, c in CAMERAS]


def render(K, T, H, W, patch):
    """float64 depth (view z) of the nearest hit of each pixel's ray, 0 where there is none"""
    R, C = T[:3, :3], -T[:3, :3].T @ T[:3, 3]
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.einsum("ij,jhw->ihw", R.T @ np.linalg.inv(K), np.stack([x, y, np.ones_like(x)]))  # view z of a ray = its parameter
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = (PLANE_D - PLANE_N @ C) / np.einsum("i,ihw->hw", PLANE_N, rays)
        depth = np.where(np.isfinite(lam) & (lam > 0), lam, 0.0)
        if patch:
            lp = (PATCH_Z - C[2]) / rays[2]
            X = C[:, None, None] + lp * rays
            hit = (np.isfinite(lp) & (lp > 0) & (X[0] > PATCH_X[0]) & (X[0] < PATCH_X[1]) & (X[1] > PATCH_Y[0]) & (X[1] < PATCH_Y[1]))
            depth = np.where(hit & ((depth == 0) | (lp < depth)), lp, depth)
    return depth


@functools.lru_cache(maxsize=None)
def scene(name, H, W):
    """-> dict(depths 5 x (H,W) float32, K (3,3), Ks, Ts 5 x (4,4) float64, images 5 x (3,H,W) float32, H, W)"""
    assert name in ("A", "B")
    K, Ts = intrinsics(H, W), poses()
    rng = np.random.default_rng(NOISE_SEED)
    depths = []
    for T in Ts:
        d = render(K, T, H, W, patch=name == "A")
        if name == "A":
            d = d * (1.0 + NOISE_SIGMA * rng.standard_normal(d.shape))
        depths.append(d.astype(np.float32))
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    images = [np.stack([x + 1000 * i, y, np.full_like(x, 7.0 * i)]) for i in range(len(Ts))]
    return {"depths": depths, "K": K, "Ks": [K] * len(Ts), "Ts": Ts, "images": images, "H": H, "W": W}


def key_and_sources(sc, key, src=None):
    """The positional arguments of fuse_numpy for view `key` against views `src` (default: all others)."""
    src = [j for j in range(len(sc["Ts"])) if j != key] if src is None else list(src)
    return (sc["depths"][key], sc["Ks"][key], sc["Ts"][key], [sc["depths"][j] for j in src], [sc["Ks"][j] for j in src],
            [sc["Ts"][j] for j in src])


def on_plane_residual(points):
    """|n.X - 4| / 4 of (M,3) points: 0 on the background plane"""
    return np.abs(np.asarray(points, dtype=np.float64) @ PLANE_N - PLANE_D) / PLANE_D


@functools.lru_cache(maxsize=None)
def reference(name, H, W, key, src=None):
    """fuse_numpy in float64 and the same chain in float32 on the float32-rounded matrices, with details, and what the device test
    derives from the two alone: the largest gaps in err, rel and d'/d over the pairs valid in both, the bands (four times the gaps:
    the kernel's chain may contract to FMAs, order its sums differently and use a 1-ulp reciprocal, each of the order of one more
    float32 rounding of the same chain), and the pairs excluded from the bit-for-bit comparison."""
    sc = scene(name, H, W)
    args = key_and_sources(sc, key, src)
    r64 = DF.fuse_numpy(*args, details=True)
    r32 = DF.fuse_numpy(*args, dtype=np.float32, details=True)
    both = r64["valid"] & r32["valid"]
    d = args[0].astype(np.float64)
    with np.errstate(all="ignore"):
        gap = {"err": np.abs(r64["err"] - r32["err"])[both].max(), "rel": np.abs(r64["rel"] - r32["rel"])[both].max(),
               "dd": (np.abs(r64["dprime"] - r32["dprime"]) / d)[both].max()}
    band = {k: 4.0 * float(v) for k, v in gap.items()}
    excluded = ((np.abs(r64["err"] - 1.0) <= band["err"]) | (np.abs(r64["rel"] - 0.01) <= band["rel"])
                | (r64["valid"] != r32["valid"]))
    return {"f64": r64, "f32": r32, "gap": gap, "band": band, "excluded": excluded, "share": float(excluded.mean())}


class StubModel:
    """A model of the run protocol that returns scene B's analytic depth of the key view at half resolution.  It finds the key view
    from the order of the calls (reconstruct runs the views in order) and records what it was handed.  By default it answers in numpy,
    as the output adapters of the package's models do."""

    def __init__(self, H, W, to_tensor=None, with_uncertainty=False, param=None):
        self.H, self.W, self.h, self.w = H, W, H // 2, W // 2
        self.Ts = poses()
        self.K_pred = intrinsics(H, W)
        self.K_pred[0] *= self.w / W
        self.K_pred[1] *= self.h / H
        self.to_tensor = to_tensor or (lambda a: a)
        self.with_uncertainty = with_uncertainty
        self.calls = []
        self.param = param  # what parameters() yields: where a real model's weights are

    def parameters(self):
        return iter(() if self.param is None else (self.param,))

    def run(self, images, keyview_idx, poses, intrinsics):
        k = len(self.calls)
        self.calls.append({"images": images, "keyview_idx": keyview_idx, "poses": poses, "intrinsics": intrinsics})
        depth = render(self.K_pred, self.Ts[k], self.h, self.w, patch=False).astype(np.float32)
        aux = {}
        if self.with_uncertainty:
            aux["depth_uncertainty"] = self.to_tensor(np.full((1, self.h, self.w), 0.25 * k, dtype=np.float32))
        return {"depth": self.to_tensor(depth[None])}, aux
