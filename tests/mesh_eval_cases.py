"""Meshes and queries for the mesh-evaluation tests (test_mesh_eval_cpu.py, test_hip_mesh_eval.py), numpy only.  Every case is built once
and shared (treat the arrays as read-only); coordinates are float32, formed in float64 and rounded once.

  sphere      an icosphere of 3 subdivisions, radius 0.5, 1280 triangles, at offset 0 and at offset 1000 on all axes; 2000 queries, 90 %
              at radius 0.5 + N(0, 0.02) and 10 % at radius 0.5 + U(-0.3, 0.3); max_dist 0.04, thresholds (0.01, 0.02): some 12 % are
              truncated and a third are under 0.01, so every verdict occurs
  boundary    cloud_cases.boundary's 26 queries on cell corners (max_dist 2^-5, base 0 and 100), each with ONE tiny triangle whose
              nearest point is a vertex at max_dist (1 -+ 2^-12) across the corner along one of the 26 directions and which leads away
              from the query from there
  crowded     700 tiny triangles and 70 queries inside one cell (more than two LDS stages of 128 records in a single cell), and 70
              queries with nothing within 3 cells; max_dist 0.05
  quad        one quad of two triangles over 40 x 40 cells of the grid at max_dist 0.04, 600 queries around its plane
  sphere+quad both meshes and both sets of queries: large boxes among small ones, and triangles that many scanned cells list
  degenerate  a triangle that is a line (three collinear vertices), one that is a segment (two equal vertices), one that is a point,
              one proper triangle, and invalid ones (a NaN vertex, an infinite vertex, an index >= M, a negative index)
"""
import functools

import numpy as np

import cloud_cases as CC
from robustmvd_amd import mesh_eval as ME

S_RADIUS, S_MAX_DIST, S_THRESHOLDS, S_OFFSETS = 0.5, 0.04, (0.01, 0.02), (0.0, 1000.0)
B_MAX_DIST, B_BASES = CC.B_MAX_DIST, CC.B_BASES
C_MAX_DIST = 0.05
Q_MAX_DIST, Q_HEIGHT, Q_HALF = 0.04, 0.6, 0.8
D_MAX_DIST = 0.3
MAX_EXCLUDED_SHARE = 0.005


@functools.lru_cache(maxsize=None)
def icosphere(subdivisions=3, radius=S_RADIUS):
    """-> (vertices (M,3) float64 on the sphere, triangles (T,3) int32, outward winding): 20 4^subdivisions triangles"""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in t:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = out
    return np.array(v) * radius, np.array(t, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def sphere(offset):
    """-> (queries (2000,3), vertices (642,3), triangles (1280,3))"""
    v, t = icosphere()
    rng = np.random.default_rng(20250301)
    n = 2000
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = S_RADIUS + rng.normal(0, 0.02, n)
    far = rng.random(n) < 0.1
    r[far] = S_RADIUS + rng.uniform(-0.3, 0.3, int(far.sum()))
    return (u * r[:, None] + offset).astype(np.float32), (v + offset).astype(np.float32), t


@functools.lru_cache(maxsize=None)
def boundary(base, sign):
    """-> (queries (26,3), vertices (78,3), triangles (26,3)): triangle i belongs to query i; its vertex 3 i is cloud_cases.boundary's
    target, and its other two vertices lie max_dist / 16 further along the direction (and a little aside), so that the vertex is the
    triangle's nearest point: (B - A) . (A - q) > 0 and (C - A) . (A - q) > 0."""
    q, p = CC.boundary(base, sign)
    vertices = []
    for i, d in enumerate(CC.DIRECTIONS):
        d = np.array(d, dtype=np.float64)
        aside = np.cross(d, [1.0, 2.0, 3.0])
        aside /= np.linalg.norm(aside)
        other = np.cross(d, aside)
        other /= np.linalg.norm(other)
        step = B_MAX_DIST / 16
        A = p[i].astype(np.float64)
        B, C = A + step * (d + 0.5 * aside), A + step * (d + 0.5 * other)
        B, C = B.astype(np.float32), C.astype(np.float32)
        toward = A - q[i].astype(np.float64)
        assert (B.astype(np.float64) - A) @ toward > 0 and (C.astype(np.float64) - A) @ toward > 0
        vertices += [p[i], B, C]
    return q, np.stack(vertices).astype(np.float32), np.arange(78, dtype=np.int32).reshape(26, 3)


@functools.lru_cache(maxsize=None)
def crowded():
    """-> (queries (140,3), vertices (2100,3), triangles (700,3)): everything but the last 70 queries inside the cell [0, 0.05)^3 of a
    grid from the origin; the last 70 queries lie 6 to 8 cells away on every axis."""
    rng = np.random.default_rng(78)
    centre = rng.uniform(0.006, 0.044, (700, 1, 3))
    vertices = (centre + rng.uniform(-0.004, 0.004, (700, 3, 3))).reshape(-1, 3)
    near, far = rng.uniform(0.001, 0.049, (70, 3)), rng.uniform(0.3, 0.4, (70, 3))
    return np.concatenate([near, far]).astype(np.float32), vertices.astype(np.float32), np.arange(2100, dtype=np.int32).reshape(700, 3)


@functools.lru_cache(maxsize=None)
def quad():
    """-> (queries (600,3), vertices (4,3), triangles (2,3)): the square |x|, |y| <= 0.8 at z = 0.6, 40 cells of 0.04 on a side"""
    rng = np.random.default_rng(79)
    h = Q_HALF
    vertices = np.array([[-h, -h, Q_HEIGHT], [h, -h, Q_HEIGHT], [h, h, Q_HEIGHT], [-h, h, Q_HEIGHT]])
    queries = np.column_stack([rng.uniform(-h - 0.1, h + 0.1, (600, 2)), Q_HEIGHT + rng.normal(0, 0.02, 600)])
    return queries.astype(np.float32), vertices.astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def sphere_quad():
    qs, vs, ts = sphere(0.0)
    qq, vq, tq = quad()
    return np.concatenate([qs, qq]), np.concatenate([vs, vq]), np.concatenate([ts, tq + len(vs)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def degenerate():
    """-> (queries (300,3), vertices (12,3), triangles (9,3)).  Triangle 0: collinear (a line from (0,0,0) to (1,0,0) through (0.4,0,0));
    1: a segment (two equal vertices) from (0,1,0) to (1,1,0); 2: a point at (0.5,0.5,0.5); 3: a proper triangle; 4..8: invalid (a NaN
    vertex, an infinite vertex, an index == M, a large index, a negative index)."""
    vertices = np.array([[0, 0, 0], [1, 0, 0], [0.4, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0.5], [0.2, 0.2, 1], [0.8, 0.2, 1], [0.5, 0.8, 1],
                         [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, 0.25]], dtype=np.float32)
    triangles = np.array([[0, 1, 2], [3, 4, 4], [5, 5, 5], [6, 7, 8], [9, 11, 5], [11, 10, 5], [0, 1, 12], [0, 2 ** 30, 1], [-1, 0, 1]],
                         dtype=np.int32)
    rng = np.random.default_rng(80)
    return rng.uniform(-0.2, 1.2, (300, 3)).astype(np.float32), vertices, triangles


def mesh_case(key):
    """key: ("sphere", offset), ("boundary", base, sign), ("crowded",), ("quad",), ("sphere+quad",) or ("degenerate",)
    -> (queries, vertices, triangles, max_dist, thresholds)"""
    if key[0] == "sphere":
        return sphere(key[1]) + (S_MAX_DIST, S_THRESHOLDS)
    if key[0] == "boundary":
        return boundary(key[1], key[2]) + (B_MAX_DIST, ())
    if key[0] == "crowded":
        return crowded() + (C_MAX_DIST, ())
    if key[0] == "quad":
        return quad() + (Q_MAX_DIST, (0.01, 0.02))
    if key[0] == "sphere+quad":
        return sphere_quad() + (Q_MAX_DIST, (0.01, 0.02))
    assert key[0] == "degenerate"
    return degenerate() + (D_MAX_DIST, ())


@functools.lru_cache(maxsize=None)
def reference(key):
    """-> dict: q, v, t, max_dist, thresholds; d64, i64 (mesh_distance_numpy in float64); raw64 / raw32: the untruncated distance in
    float64 and from the same chain in float32; gap = max |raw32 - raw64| over the queries untruncated in both; band = 4 gap (the
    kernel may contract to FMAs, add the three-term sums in another order and use a 1-ulp sqrt and division, each about one more
    float32 rounding of the same chain); excluded: the queries whose raw64 is within the band of max_dist or of a threshold; share:
    their share, which the tests cap at MAX_EXCLUDED_SHARE on this reference alone."""
    q, v, t, max_dist, thresholds = mesh_case(key)
    md = np.float32(max_dist)
    d64, i64 = ME.mesh_distance_numpy(q, v, t, md)
    raw64, _ = ME.mesh_distance_numpy(q, v, t, np.inf)
    raw32, _ = ME.mesh_distance_numpy(q, v, t, np.inf, dtype=np.float32)
    both = (raw64 < md) & (raw32 < md)
    gap = float(np.abs(raw32.astype(np.float64) - raw64)[both].max()) if both.any() else 0.0
    band = 4.0 * gap
    excluded = np.zeros(len(q), dtype=bool)
    for edge in (md,) + tuple(np.float32(x) for x in thresholds):
        excluded |= np.abs(raw64 - np.float64(edge)) <= band
    return {"q": q, "v": v, "t": t, "d64": d64, "i64": i64, "raw64": raw64, "raw32": raw32, "gap": gap, "band": band, "excluded": excluded,
            "share": float(excluded.mean()) if len(q) else 0.0, "max_dist": md, "thresholds": tuple(np.float32(x) for x in thresholds)}
