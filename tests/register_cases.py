"""Clouds for the registration tests (test_cloud_register_cpu.py, test_hip_cloud_register.py).  Every case is built once and shared
(treat the arrays as read-only); coordinates are float32, formed in float64 and rounded once.

  scene R   4000 targets on cloud_cases.surface over [-1,1]^2 with their analytic unit normals, at offset 0 and at offset 1000 on all
            axes.  The source: 2000 of the targets taken through the inverse of a known T* (3 degrees about (0.3, -0.5, 0.8) through
            the cloud's centre, translation (0.02, -0.01, 0.014), scale 1.03 for "similarity"), then 200 FAR points (1.5 above the
            surface, through the same inverse: they must never pair) and 5 NaN rows.  Radius 0.1.
"""
import functools

import numpy as np

import cloud_cases as CC
from robustmvd_amd import cloud_register as CR

R_RADIUS, R_OFFSETS, R_MODES = 0.1, (0.0, 1000.0), ("rigid", "similarity", "plane")
R_TRUE, R_FAR, R_NAN = 2000, 200, 5
R_AXIS, R_ANGLE, R_SHIFT, R_SCALE = (0.3, -0.5, 0.8), 3.0, (0.02, -0.01, 0.014), 1.03


def surface_normals(xy):
    g = np.stack([-0.6 * np.cos(2 * xy[:, 0]) * np.cos(3 * xy[:, 1]), 0.9 * np.sin(2 * xy[:, 0]) * np.sin(3 * xy[:, 1]),
                  np.ones(len(xy))], axis=1)
    return g / np.linalg.norm(g, axis=1, keepdims=True)


def rotation(axis, degrees):
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def t_star(offset, similarity):
    """T*: x -> c + s R (x - c) + shift, c the cloud's centre, as a (4,4) float64."""
    c = np.full(3, float(offset))
    M = (R_SCALE if similarity else 1.0) * rotation(R_AXIS, R_ANGLE)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = M, c - M @ c + np.asarray(R_SHIFT)
    return T


def apply64(T, points):
    """T on float32 points in float64, unrounded: where a transform puts them."""
    T = np.asarray(T, dtype=np.float64)
    return np.asarray(points, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]


@functools.lru_cache(maxsize=None)
def scene_r(offset, similarity=False):
    """-> dict: source (2205,3), target (4000,3), normals (4000,3) float32; t_star (4,4); true / far / nan: the source's row slices"""
    rng = np.random.default_rng(20250317)
    txy = rng.uniform(-1, 1, (4000, 2))
    target = (np.column_stack([txy, CC.surface(txy)]) + offset).astype(np.float32)
    normals = surface_normals(txy).astype(np.float32)
    T = t_star(offset, similarity)
    inv = np.linalg.inv(T)
    chosen = rng.permutation(4000)[:R_TRUE]
    fxy = rng.uniform(-1, 1, (R_FAR, 2))
    far = np.column_stack([fxy, CC.surface(fxy) + 1.5]) + offset
    source = np.concatenate([apply64(inv, target[chosen]), apply64(inv, far), np.full((R_NAN, 3), np.nan)]).astype(np.float32)
    return {"source": source, "target": target, "normals": normals, "t_star": T, "chosen": chosen,
            "true": slice(0, R_TRUE), "far": slice(R_TRUE, R_TRUE + R_FAR), "nan": slice(R_TRUE + R_FAR, None)}


def landing_error(scene, transform):
    """The largest distance between where `transform` and T* put a valid source point (float64)."""
    s = scene["source"][:R_TRUE + R_FAR]
    return float(np.linalg.norm(apply64(transform, s) - apply64(scene["t_star"], s), axis=1).max())


@functools.lru_cache(maxsize=None)
def reference(offset, mode):
    """register_numpy on scene R -> dict: scene, reg (the Registration), err (landing_error of the numpy path itself)"""
    sc = scene_r(offset, mode == "similarity")
    reg = CR.register_numpy(sc["source"], sc["target"], R_RADIUS, mode=mode, target_normals=sc["normals"] if mode == "plane" else None)
    return {"scene": sc, "reg": reg, "err": landing_error(sc, reg.transform)}
