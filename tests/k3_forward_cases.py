"""K3 forward on the CPU (numpy): a restatement of the operator with the dtype of the sampling positions and of the blend chosen
separately, a restatement of the tile kernel's PROBE step (which chunks of 8 planes take their taps from the LDS window, which
gather them, which see a plane behind a source camera), and the table of small cases that tests/test_hip_k3_forward.py runs on the
device.  tests/test_k3_forward_cpu.py pins all of it without a GPU; no test lives here.

Restatement.  grid="exact" is the oracle's chain (oracle/mvd_oracle.py homo_warp_grid, grid_sample_zeros, warp_variance), which is
the kernels' chain under exact_grid=True; grid="folded" is `position` of csrc/warp_variance_tile.hip (the default grid): the
composed transform applied to (x, y, 1) first, fused multiply-adds, ix = X/Z * w/(w-1) - 0.5, with an IEEE division where the
kernel multiplies by v_rcp_f32(Z).  Both clamp the position to [-1, w] x [-1, h] (NaN to -1) and read a zero-bordered map, as the
kernels do; for the exact chain that gives the same values as the oracle's in-bounds test of every tap (pinned bit for bit).
`compose` says how the 3x4 transform src_proj @ key_proj_inv is rounded when the positions are float32: "matmul" is the oracle's
float32 numpy product, "fma" the fmaf chain of compose_transforms_kernel (csrc/warp_variance.hip), which is what both kernels read.
With float64 positions the product is taken in float64.

A float32 fused multiply-add on arrays is a float64 product (exact) plus the addend, rounded to float64 and then to float32: the two
roundings differ from one in about 2^-29 of the cases, and nothing asserts bits on the float32 folded grid.  The 12 V B entries of
compose="fma" are rounded once, exactly."""
import functools
from fractions import Fraction

import numpy as np

from test_hip_shapes import mvs_inputs

F32, F64 = np.float32, np.float64
TILE_W, TILE_H, PLANES = 8, 4, 8      # key tile and chunk of the tile kernel
WIN_F32, WIN_F16 = 104, 128           # window pixels of the two product variants (launch_k3)
LABEL_MARGIN_PX = 16                  # a label counts a chunk only this far from the window size ...
LABEL_MARGIN_Z = 1e-3                 # ... or with a corner this far (relative to the depth) behind the camera


# ------------------------------------------------------------------------------------------------ transforms
def _fma32_exact(a, b, c):
    """float32 fmaf(a, b, c) of scalars with ONE rounding (to nearest even), through exact rationals"""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    f = F32(float(x))  # within one float32 step of the result
    best = None
    for cand in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))):
        err = abs(Fraction(float(cand)) - x)
        even = (int(np.asarray(cand, F32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, cand, even)
    return F32(best[1])


def composed_transforms(projs, key_inv, pos_dtype, compose="matmul"):
    """(V, B, 3, 4) rows of src_proj @ key_proj_inv in pos_dtype"""
    V, B = len(projs), key_inv.shape[0]
    if pos_dtype == F64:
        return np.stack([np.matmul(p.astype(F64), key_inv.astype(F64))[:, :3] for p in projs])
    if compose == "matmul":
        return np.stack([np.matmul(p.astype(F32), key_inv.astype(F32)).astype(F32)[:, :3] for p in projs])
    assert compose == "fma", compose
    M = np.zeros((V, B, 3, 4), F32)
    for v in range(V):
        for b in range(B):
            P, Q = projs[v][b].astype(F32), key_inv[b].astype(F32)
            for i in range(3):
                for j in range(4):
                    acc = F32(P[i, 0] * Q[0, j])
                    for k in (1, 2, 3):
                        acc = _fma32_exact(P[i, k], Q[k, j], acc)
                    M[v, b, i, j] = acc
    return M


def _fma(a, b, c, dt):
    if dt == F64:
        return a * b + c
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def _clamp(v, hi):
    """v_med3_f32(v, -1, hi): NaN goes to -1"""
    return np.where(np.isnan(v), v.dtype.type(-1), np.minimum(np.maximum(v, v.dtype.type(-1)), v.dtype.type(hi)))


def positions(M, x, y, d, h, w, grid, dt):
    """Clamped sampling position (ix, iy) and Z of key pixels (x, y) at depths d (broadcastable arrays of dtype dt) under one
    composed transform M (3, 4) of dtype dt."""
    m = lambda i, j: dt(M[i, j])
    with np.errstate(all="ignore"):
        if grid == "exact":
            gx, gy, gz = x * d, y * d, dt(1.0) * d
            X = m(0, 0) * gx + m(0, 1) * gy + m(0, 2) * gz + m(0, 3)
            Y = m(1, 0) * gx + m(1, 1) * gy + m(1, 2) * gz + m(1, 3)
            Z = m(2, 0) * gx + m(2, 1) * gy + m(2, 2) * gz + m(2, 3)
            nx = (X / Z) / dt((w - 1) / 2) - dt(1.0)
            ny = (Y / Z) / dt((h - 1) / 2) - dt(1.0)
            ix = ((nx + dt(1.0)) * dt(w) - dt(1.0)) / dt(2.0)
            iy = ((ny + dt(1.0)) * dt(h) - dt(1.0)) / dt(2.0)
        else:
            assert grid == "folded", grid
            sx, sy = dt(w) / dt(w - 1), dt(h) / dt(h - 1)
            ax = _fma(m(0, 0), x, _fma(m(0, 1), y, m(0, 2), dt), dt)
            ay = _fma(m(1, 0), x, _fma(m(1, 1), y, m(1, 2), dt), dt)
            az = _fma(m(2, 0), x, _fma(m(2, 1), y, m(2, 2), dt), dt)
            X, Y, Z = _fma(ax, d, m(0, 3), dt), _fma(ay, d, m(1, 3), dt), _fma(az, d, m(2, 3), dt)
            rz = dt(1.0) / Z
            ix = _fma(X * rz, sx, dt(-0.5), dt)
            iy = _fma(Y * rz, sy, dt(-0.5), dt)
        ix, iy = np.asarray(ix, dt), np.asarray(iy, dt)
        return _clamp(ix, w), _clamp(iy, h), np.asarray(Z, dt)


def cells(M, depth_b, h, w, grid, dt):
    """per (plane, y, x): first-tap cell in the zero-bordered map and the four weights (nw, ne, sw, se), dtype dt"""
    x = np.arange(w, dtype=dt)[None, None, :]
    y = np.arange(h, dtype=dt)[None, :, None]
    d = depth_b.astype(dt)[:, None, None]
    ix, iy, _ = positions(M, x, y, d, h, w, grid, dt)
    ix, iy = np.broadcast_to(ix, (len(depth_b), h, w)), np.broadcast_to(iy, (len(depth_b), h, w))
    x0, y0 = np.floor(ix), np.floor(iy)
    if grid == "exact":  # grid_sampler's weights
        x1, y1 = x0 + dt(1.0), y0 + dt(1.0)
        wts = ((x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0))
    else:                # locate's
        wx, wy = ix - x0, iy - y0
        ux, uy = dt(1.0) - wx, dt(1.0) - wy
        wts = (ux * uy, wx * uy, ux * wy, wx * wy)
    return x0.astype(np.int64) + 1, y0.astype(np.int64) + 1, wts


def _sample(feat_b, cx, cy, wts, bt):
    """bilinear blend of one (C, h, w) map at the cells: taps nw, ne, sw, se added in that order, dtype bt"""
    C, h, w = feat_b.shape
    pad = np.zeros((C, h + 3, w + 3), bt)
    pad[:, 1:h + 1, 1:w + 1] = feat_b
    out = np.zeros((C,) + cx.shape, bt)
    for (dy, dx), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), wts):
        out += pad[:, cy + dy, cx + dx] * wt.astype(bt)[None]
    return out


def homo_warp_restated(feat, proj, key_inv, depth, grid="exact", pos_dtype=F32, blend_dtype=F32, compose="matmul"):
    """feat (B,C,h,w) warped to the key view at depth (B,D): (B,C,D,h,w) of blend_dtype"""
    B, C, h, w = feat.shape
    M = composed_transforms([proj], key_inv, pos_dtype, compose)[0]
    return np.stack([_sample(feat[b], *cells(M[b], depth[b], h, w, grid, pos_dtype), blend_dtype) for b in range(B)])


def warp_variance_restated(feats, projs, key_inv, depth, grid="exact", pos_dtype=F32, blend_dtype=F32, compose="matmul"):
    """feats[0] the key map, feats[1:] the V source maps, each (B,C,h,w): the variance volume (B,C,D,h,w) of blend_dtype"""
    bt = blend_dtype
    key = feats[0]
    D = depth.shape[1]
    nv = bt(len(feats))
    vsum = np.repeat(key[:, :, None], D, 2).astype(bt)
    vsq = vsum ** 2
    for f, P in zip(feats[1:], projs):
        wv = homo_warp_restated(f, P, key_inv, depth, grid, pos_dtype, bt, compose)
        vsum = vsum + wv
        vsq = vsq + wv ** 2
    return vsq / nv - (vsum / nv) ** 2


def key_only_variance(key, D, V, dt=F64):
    """the volume when every source map is zero"""
    k = np.repeat(key[:, :, None], D, 2).astype(dt)
    return k ** 2 / dt(V + 1) - (k / dt(V + 1)) ** 2


# ------------------------------------------------------------------------------------------------ probe
def classify(projs, key_inv, depth, h, w, win):
    """The tile kernel's PROBE in float64 (folded grid).  Per (batch element, tile, chunk, view): `npix`, the pixels of the unit's
    box (the whole zero-bordered map, as in the kernel, when a corner has Z <= 0 or NaN), `box` = (xmin, xmax, ymin, ymax), the
    range of first-tap cells the box admits, `behind`, whether a corner has Z <= 0, and `zrel`, the smallest Z / |depth| over the 8
    corners.  `window` (batch element, tile, chunk): the chunk runs in PASS 0."""
    B, D = depth.shape
    V = len(projs)
    M = composed_transforms(projs, key_inv, F64)
    tx, ty = (w + TILE_W - 1) // TILE_W, (h + TILE_H - 1) // TILE_H
    nchunk = (D + PLANES - 1) // PLANES
    npix = np.zeros((B, tx * ty, nchunk, V), np.int64)
    behind = np.zeros((B, tx * ty, nchunk, V), bool)
    zrel = np.zeros((B, tx * ty, nchunk, V))
    box = np.zeros((B, tx * ty, nchunk, V, 4), np.int64)
    for b in range(B):
        for t in range(tx * ty):
            x0, y0 = (t % tx) * TILE_W, (t // tx) * TILE_H
            cx = np.array([x0, min(x0 + TILE_W - 1, w - 1)], F64)[None, None, :]
            cy = np.array([y0, min(y0 + TILE_H - 1, h - 1)], F64)[None, :, None]
            for c in range(nchunk):
                planes = [min(c * PLANES, D - 1), min(c * PLANES + PLANES - 1, D - 1)]  # missing planes repeat plane D-1
                d = depth[b, planes].astype(F64)[:, None, None]
                for v in range(V):
                    ix, iy, Z = positions(M[v, b], cx, cy, d, h, w, "folded", F64)
                    Z = np.broadcast_to(Z, (2, 2, 2))
                    ok = Z > 0  # False for NaN
                    behind[b, t, c, v] = not ok.all()
                    with np.errstate(all="ignore"):
                        zrel[b, t, c, v] = np.nanmin(np.where(np.isnan(Z), -np.inf, Z / np.abs(d)))
                    cellx = np.broadcast_to(np.floor(ix) + 1, (2, 2, 2)).astype(np.int64)
                    celly = np.broadcast_to(np.floor(iy) + 1, (2, 2, 2)).astype(np.int64)
                    # a corner that is not ok takes part with cell 0 in the minimum and 65535 in the maximum
                    mnx, mny = np.where(ok, cellx, 0).min(), np.where(ok, celly, 0).min()
                    mxx, mxy = np.where(ok, cellx, 65535).max(), np.where(ok, celly, 65535).max()
                    xmin, ymin = max(mnx - 1, 0), max(mny - 1, 0)
                    xmax, ymax = min(mxx + 1, w + 1), min(mxy + 1, h + 1)
                    npix[b, t, c, v] = (xmax - xmin + 2) * (ymax - ymin + 2)
                    box[b, t, c, v] = (xmin, xmax, ymin, ymax)
    return dict(npix=npix, box=box, behind=behind, zrel=zrel, window=(npix <= win).all(-1))


def chunk_classes(cl, win):
    """Counts of the chunks (batch element, tile, chunk) a label may name: "window", every view's box at most win - 16 px and no
    corner with Z <= 0; "gather", no corner with Z <= 0 and some box at least win + 16 px; "behind", a corner with
    Z <= -1e-3 |depth|; "marginal", the others (a float32 probe on the device may decide them either way)."""
    any_behind = cl["behind"].any(-1)
    window = ~any_behind & (cl["npix"] <= win - LABEL_MARGIN_PX).all(-1)
    gather = ~any_behind & (cl["npix"] >= win + LABEL_MARGIN_PX).any(-1)
    behind = (cl["zrel"] <= -LABEL_MARGIN_Z).any(-1)
    n = window.size
    return dict(window=int(window.sum()), gather=int(gather.sum()), behind=int(behind.sum()),
                marginal=int(n - (window | gather | behind).sum()), chunks=int(n))


SIZEOF_VIEWREC = 12 * 4 + 2 * 4 + 2 * 4  # float M[12]; unsigned base_lo, base_hi; unsigned pad[2]
SIZEOF_UNITREC = 8 * 4                   # boxmin, extent, pitch, npix, base, skip, inv_nc, pad


def tile_lds_bytes(win, f16, V, nch):
    return (2 * win * (64 if f16 else 128) + 2 * 4096 + 2 * 1024 + 512 + 128 + V * SIZEOF_VIEWREC + nch * 32 +
            nch * V * SIZEOF_UNITREC)


def nch_of(V, win, f16):
    """chunks per march of the product's tile variants (one tap set: four workgroups per CU share 160 KiB of LDS)"""
    nch, budget = 8, 160 * 1024 // 4
    while nch > 1 and tile_lds_bytes(win, f16, V, nch) > budget:
        nch -= 1
    return nch


def march_groups(D, V, win, f16):
    """chunks of each chunk group of a tile: group g marches through chunks g, g + groups, ..."""
    dchunks = (D + PLANES - 1) // PLANES
    nch = nch_of(V, win, f16)
    groups = (dchunks + nch - 1) // nch
    return [len(range(g, dchunks, groups)) for g in range(groups)]


# ------------------------------------------------------------------------------------------------ cases
def _inv_depth(B, D, near=0.5, far=10.0):
    return np.stack([(1.0 / np.linspace(1.0 / near, 1.0 / far, D)).astype(F32)] * B)


WIDE = dict(rot=0.7, trans=0.8, dmin=0.2, dmax=3.0)  # test_warp_variance_wide_baseline_vs_oracle
FAR = dict(dmin=6.0, dmax=9.0)
# name -> (B, h, w, D, V), seed, mvs_inputs keywords, depth override, classes the label names per window size {104, 128}.
# A class a label does not name must have no chunk (marginal chunks aside).
# "behind" is the wide-baseline geometry of test_hip_shapes.py (seed 77); its third view never lands in the map at any depth of
# the range, and at D = 40 a float32 evaluation of its float64 reference sits at 0.85 of the hard band.  "all_three" therefore takes
# seed 88, the first after 77 at which all three classes have chunks at both window sizes, every view alone moves the volume
# (test_one_hot_views_move_the_reference) and the float32 evaluation stays within half the band
# (test_float32_restatement_sits_inside_the_hard_band).
CASES = {
    "window_ragged":   ((2, 5, 9, 17, 2), 11, FAR, None, {104: ("window",), 128: ("window",)}),
    "window_smallest": ((1, 2, 2, 1, 1), 11, FAR, None, {104: ("window",), 128: ("window",)}),
    "gather_only":     ((1, 9, 70, 3, 6), 1009, {}, None, {104: ("gather",), 128: ("gather",)}),
    "mixed":           ((1, 13, 22, 40, 4), 1013, {}, _inv_depth, {104: ("window", "gather"), 128: ("window",)}),
    "behind":          ((1, 24, 40, 8, 3), 77, WIDE, None, {104: ("behind",), 128: ("behind",)}),
    "all_three":       ((1, 24, 40, 40, 3), 88, WIDE, None, {104: ("window", "gather", "behind"), 128: ("window", "gather", "behind")}),
    "short_march":     ((1, 13, 22, 72, 11), 1013, FAR, None, {104: ("window",), 128: ("window",)}),
    "v32":             ((1, 8, 12, 20, 32), 1008, {}, None, {104: ("window", "gather"), 128: ("window", "gather")}),
    "xcd_8_tiles":     ((1, 4, 64, 9, 2), 1004, {}, None, {104: ("window", "gather"), 128: ("window", "gather")}),
    "xcd_9_tiles":     ((1, 4, 66, 9, 2), 1004, {}, None, {104: ("window",), 128: ("window",)}),
    # every factor of the block index above one at once: 2 batch elements x 2 tiles per XCD slot (12 tiles) x 2 chunk groups
    "batch_march":     ((2, 9, 30, 65, 11), 2009, {}, None, {104: ("window", "gather"), 128: ("window", "gather")}),
}
OTHER_CHANNELS = (4, 8, 16, 64)                              # warp_variance_kernel<1, 2, 4, 16>
OTHER_CHANNEL_GEOMETRIES = ("window_ragged", "mixed", "behind")
HOMO_WARP_CHANNELS = (4, 8, 16, 32, 64)
HOMO_WARP_GEOMETRIES = ("window_ragged", "behind")


@functools.lru_cache(maxsize=None)
def case_inputs(name, C=32):
    """(feats, projs, key_inv, depth) of a case.  The geometry is that of mvs_inputs at C = 32 whatever C is (mvs_inputs draws the
    features first, so its poses depend on C); at another C the features come from a generator of their own."""
    (B, h, w, D, V), seed, kw, depth_fn, _ = CASES[name]
    feats, projs, key_inv, depth = mvs_inputs(B, 32, h, w, D, V, seed=seed, **kw)
    if depth_fn is not None:
        depth = depth_fn(B, D)
    if C != 32:
        rng = np.random.default_rng(seed * 100 + C)
        feats = [rng.standard_normal((B, C, h, w)).astype(F32) for _ in range(V + 1)]
    return feats, projs, key_inv, depth  # shared by every test of a session: not to be written to


@functools.lru_cache(maxsize=None)
def case_classes(name, win):
    (B, h, w, D, V), *_ = CASES[name]
    _, projs, key_inv, depth = case_inputs(name)
    return chunk_classes(classify(projs, key_inv, depth, h, w, win), win)


def references(name, C=32, exact=False, half=False, hot=None):
    """(want64, sharp, e) of a case.  want64: the restatement in float64 on the grid the kernel is asked for.  With exact=True also
    `sharp`, the restatement with the kernel's float32 positions (exact chain, transforms composed by the kernel's fmaf chain) and a
    float64 blend, and e, the largest deviation of the all-float32 restatement from it: blend and summation rounding only.
    half: the features rounded to fp16 first.  hot: every source map but this one zeroed.  (Each is used by one test: not kept.)"""
    _, projs, key_inv, depth = case_inputs(name, C)
    feats = case_features(name, C, half, hot)
    grid = "exact" if exact else "folded"
    want64 = warp_variance_restated(feats, projs, key_inv, depth, grid, F64, F64)
    if not exact:
        return want64, None, None
    sharp = warp_variance_restated(feats, projs, key_inv, depth, "exact", F32, F64, compose="fma")
    all32 = warp_variance_restated(feats, projs, key_inv, depth, "exact", F32, F32, compose="fma")
    return want64, sharp, float(np.abs(all32.astype(F64) - sharp).max())


def case_features(name, C=32, half=False, hot=None):
    """the case's feature maps, rounded to fp16-representable values (half) or with every source map but `hot` zeroed"""
    feats = list(case_inputs(name, C)[0])
    if half:
        feats = [f.astype(np.float16).astype(F32) for f in feats]
    if hot is not None:
        feats = [feats[0]] + [f if i == hot else np.zeros_like(f) for i, f in enumerate(feats[1:])]
    return feats
