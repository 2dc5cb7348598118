"""Point clouds for the cloud-evaluation tests (test_cloud_eval_cpu.py, test_hip_cloud_eval.py).  Every case is built once and shared
(treat the arrays as read-only); coordinates are float32, formed in float64 and rounded once.

  scene S     4000 targets on z = 0.3 sin(2x) cos(3y) over [-1,1]^2 and 3000 queries on the same surface plus N(0, 0.004) noise on
              every coordinate, at offset 0 and at offset 1000 on all axes (grid indices around 10^5 / 3); max_dist 0.03, thresholds
              (0.005, 0.01, 0.03): about 20 % of the queries are under 0.01 and about 10 % truncated, so both outcomes occur
  boundary    max_dist = 2^-5; 26 isolated queries on cell corners (base + k 2^-5, base 0 and 100), each with ONE target at
              max_dist (1 - 2^-12) ("-": must be found) or max_dist (1 + 2^-12) ("+": must be truncated) along one of the 26 axis and
              diagonal directions
  clustered   5000 targets and 70 queries inside one cell, and 70 queries with nothing within 3 cells
"""
import functools
import itertools

import numpy as np

from robustmvd_amd import cloud_eval as CE

S_MAX_DIST, S_THRESHOLDS, S_OFFSETS = 0.03, (0.005, 0.01, 0.03), (0.0, 1000.0)
B_MAX_DIST, B_BASES = 2.0 ** -5, (0.0, 100.0)
C_MAX_DIST = 0.05
DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if any(d)]


def surface(xy):
    return 0.3 * np.sin(2 * xy[:, 0]) * np.cos(3 * xy[:, 1])


@functools.lru_cache(maxsize=None)
def scene_s(offset):
    """-> (queries (3000,3), targets (4000,3)) float32"""
    rng = np.random.default_rng(20240911)
    txy = rng.uniform(-1, 1, (4000, 2))
    qxy = rng.uniform(-1, 1, (3000, 2))
    targets = np.column_stack([txy, surface(txy)])
    queries = np.column_stack([qxy, surface(qxy)]) + rng.normal(0, 0.004, (3000, 3))
    return (queries + offset).astype(np.float32), (targets + offset).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(queries_key, max_dist, thresholds=()):
    """queries_key: ("S", offset, direction) with direction "qt" (queries -> targets) or "tq", ("B", base, sign) or ("C",).
    -> dict: q, p; d64, i64 (nearest_numpy in float64); raw64 / raw32: the untruncated distance in float64 and from the same chain in
    float32; gap = max |raw32 - raw64| over the queries untruncated in both; band = 4 gap (the kernel may contract to FMAs, add the
    three squares in another order and use a 1-ulp sqrt, each about one more float32 rounding of the same chain); excluded: the
    queries whose raw64 is within the band of max_dist or of a threshold."""
    q, p = clouds(queries_key)
    md = np.float32(max_dist)
    d64, i64 = CE.nearest_numpy(q, p, md)
    raw64, _ = CE.nearest_numpy(q, p, np.inf)
    raw32, _ = CE.nearest_numpy(q, p, np.inf, dtype=np.float32)
    both = (raw64 < md) & (raw32 < md)
    gap = float(np.abs(raw32.astype(np.float64) - raw64)[both].max()) if both.any() else 0.0
    band = 4.0 * gap
    excluded = np.zeros(len(q), dtype=bool)
    for edge in (md,) + tuple(np.float32(t) for t in thresholds):
        excluded |= np.abs(raw64 - np.float64(edge)) <= band
    return {"q": q, "p": p, "d64": d64, "i64": i64, "raw64": raw64, "raw32": raw32, "gap": gap, "band": band, "excluded": excluded,
            "share": float(excluded.mean()) if len(q) else 0.0, "max_dist": md}


def clouds(key):
    if key[0] == "S":
        q, p = scene_s(key[1])
        return (q, p) if key[2] == "qt" else (p, q)
    if key[0] == "B":
        return boundary(key[1], key[2])
    return clustered()


@functools.lru_cache(maxsize=None)
def boundary(base, sign):
    """-> (queries (26,3), targets (26,3)) float32; target i belongs to query i and is the only one within 7 cells of it.  The
    target's float32 rounding (1 ulp = max_dist 2^-12 at base 100) can carry a diagonal target across max_dist: it is then moved by
    single float32 steps along its direction until the float64 distance of the float32 points is on the intended side, and the
    builder asserts that it stays within max_dist 2^-11 of max_dist."""
    assert sign in ("-", "+")
    md = np.float64(B_MAX_DIST)
    want = md * (1 - 2.0 ** -12) if sign == "-" else md * (1 + 2.0 ** -12)
    queries, targets = [], []
    for i, d in enumerate(DIRECTIONS):
        q = np.array([base + (8 * i + 8) * md, base + 8 * md, base + 8 * md]).astype(np.float32)  # exact in float32
        unit = np.array(d, dtype=np.float64) / np.linalg.norm(d)
        t = (q.astype(np.float64) + unit * want).astype(np.float32)
        dist = lambda t: np.linalg.norm(t.astype(np.float64) - q.astype(np.float64))
        for _ in range(8):
            wrong = dist(t) >= md * (1 - 2.0 ** -14) if sign == "-" else dist(t) <= md * (1 + 2.0 ** -14)
            if not wrong:
                break
            toward = -np.array(d) if sign == "-" else np.array(d)  # "-": nearer to the query
            t = np.where(toward != 0, np.nextafter(t, (t + toward * np.float32(1.0)).astype(np.float32)), t).astype(np.float32)
        assert (dist(t) < md * (1 - 2.0 ** -14)) if sign == "-" else (dist(t) > md * (1 + 2.0 ** -14)), (base, sign, d)
        assert abs(dist(t) - md) <= md * 2.0 ** -11, (base, sign, d, dist(t))
        queries.append(q)
        targets.append(t)
    return np.stack(queries), np.stack(targets)


@functools.lru_cache(maxsize=None)
def clustered():
    """-> (queries (140,3), targets (5000,3)) float32: everything but the last 70 queries inside the cell [0, 0.05)^3 of a grid from
    the origin; the last 70 queries lie 6 to 8 cells away on every axis."""
    rng = np.random.default_rng(77)
    targets = rng.uniform(0.001, 0.049, (5000, 3))
    near = rng.uniform(0.001, 0.049, (70, 3))
    far = rng.uniform(0.3, 0.4, (70, 3))
    return np.concatenate([near, far]).astype(np.float32), targets.astype(np.float32)


def voxel_faces(voxel, n=400, seed=5, negative=False):
    """Points for the voxel tests: a third exactly on voxel faces (k * voxel as float32 products), a third one float32 step below
    a face and the rest random, over [0,1)^3 or [-1,1)^3."""
    rng = np.random.default_rng(seed)
    v = np.float32(voxel)
    lo = -1.0 if negative else 0.0
    pts = rng.uniform(lo, 1.0, (n, 3)).astype(np.float32)
    k = rng.integers(int(lo / voxel) + 1, int(1.0 / voxel), (n, 3)).astype(np.float32)  # no face at the low end: a step below it is outside
    face = k * v
    third = n // 3
    pts[:third] = face[:third]
    pts[third:2 * third] = np.nextafter(face[third:2 * third], np.float32(-10.0))
    return pts
