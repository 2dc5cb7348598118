"""Clouds and shared references for the point-cloud clean-up tests (test_cloud_clean_cpu.py, test_hip_cloud_clean.py).  Every case is
built once and shared (treat the arrays as read-only).

  noisy       the 4000 targets of cloud_cases.scene_s(offset), the surface z = 0.3 sin(2x) cos(3y), plus 60 floaters
              default_rng(31).uniform(-1,1,(60,3)) * [1,1,0.5] + [0,0,0.9] + offset, rounded to float32; offsets 0 and 1000, radius 0.08.
              Surface counts within the radius are 2 / 17 / 36 (min / median / max) and no floater has more than 1 neighbour, so
              min_neighbours = 2 removes exactly the floaters.  With k = 8 the largest 8th-neighbour distance on the surface is 0.1106
              and the smallest floater mean 0.175: MAX_DIST_SHORT leaves every floater without a full list, MAX_DIST_LONG gives every
              point one and the floaters fail by the threshold (0.1448 at std_ratio 2).
"""
import functools

import numpy as np

import cloud_cases as CC
from robustmvd_amd import cloud_clean as CL

RADIUS, OFFSETS = 0.08, (0.0, 1000.0)
N_SURFACE, N_FLOATERS = 4000, 60
K, STD_RATIO = 8, 2.0
MAX_DIST_SHORT = 0.12  # above the surface's largest 8th-neighbour distance, below every floater's (test_cloud_clean_cpu.py asserts both)
MAX_DIST_LONG = 4.0    # above the scene's diameter: every point has a full list
SUM_BOUND = 2.0 ** -52  # a float64 sum of c terms is within (c + 16) 2^-52 sum |term| of the exact one, whatever the order


@functools.lru_cache(maxsize=None)
def noisy(offset):
    """-> (4060,3) float32: the surface points first, then the floaters"""
    floaters = np.random.default_rng(31).uniform(-1, 1, (N_FLOATERS, 3)) * [1, 1, 0.5] + [0, 0, 0.9] + offset
    return np.concatenate([CC.scene_s(offset)[1], floaters.astype(np.float32)])


def analytic_normals(points, offset):
    """The unit normals of z = 0.3 sin(2x) cos(3y) at the points' (x, y), with n_z > 0, in float64"""
    x, y = points[:, 0].astype(np.float64) - offset, points[:, 1].astype(np.float64) - offset
    n = np.stack([-0.6 * np.cos(2 * x) * np.cos(3 * y), 0.9 * np.sin(2 * x) * np.sin(3 * y), np.ones_like(x)], axis=1)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def neighbourhood(offset):
    """neighbourhood_numpy of the scene against itself, with the default grid"""
    return CL.neighbourhood_numpy(noisy(offset), RADIUS)


@functools.lru_cache(maxsize=None)
def knn(offset, k, max_dist):
    return CL.knn_numpy(noisy(offset), k, max_dist)


@functools.lru_cache(maxsize=None)
def outliers(offset, rule):
    """remove_outliers_numpy of the scene (with the points as colours and their negatives as normals): rule "density", "short" or "long" """
    p = noisy(offset)
    return CL.remove_outliers_numpy(p, p, -p, **arguments(rule))


def arguments(rule):
    if rule == "density":
        return dict(radius=RADIUS, min_neighbours=2)
    return dict(k=K, std_ratio=STD_RATIO, max_dist=MAX_DIST_SHORT if rule == "short" else MAX_DIST_LONG)


def brute_neighbours(q, p, r, self_query):
    """An independent brute force: per query the list of (d2 float32, j) of its neighbours, in ascending j; plain Python loops over
    numpy float32 scalars, so every operation of the chain is one rounded float32 operation."""
    f = np.float32
    r2 = f(r) * f(r)
    out = []
    for i in range(len(q)):
        row = []
        if np.isfinite(q[i]).all():
            for j in range(len(p)):
                if (self_query and i == j) or not np.isfinite(p[j]).all():
                    continue
                dx, dy, dz = f(q[i, 0] - p[j, 0]), f(q[i, 1] - p[j, 1]), f(q[i, 2] - p[j, 2])
                d2 = f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz))
                if d2 < r2:
                    row.append((d2, j))
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def index_order(offset):
    """(the scene's neighbourhood_numpy with ONE cell for the whole cloud, i.e. the sums in plain index order; sum |term| (n,10) of the
    distance and the nine moments, for the bound (count + 16) 2^-52 sum |term|)"""
    p = noisy(offset)
    plain = CL.neighbourhood_numpy(p, RADIUS, cell=1.0e4)
    r2 = np.float32(RADIUS) * np.float32(RADIUS)
    total = np.zeros((len(p), 10))
    for b in range(0, len(p), 500):
        q = p[b:b + 500]
        d2 = CL._pair_d2(q, p)
        inside = d2 < r2
        inside[np.arange(len(q)), np.arange(b, b + len(q))] = False
        qi, pj = np.nonzero(inside)
        np.add.at(total, qi + b, np.abs(CL._moment_terms(q[qi], p[pj], np.sqrt(d2[qi, pj]))))
    return plain, total
