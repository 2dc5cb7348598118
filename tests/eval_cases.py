"""Inputs of the depth-evaluation fixtures (tests/golden/g18_eval*.npz), shared by tests/golden/make_golden_eval.py and the tests:
seeded, so the fixtures store only what the reference computed from them."""
import numpy as np

GT_SHAPE = (37, 53)
PRED_SHAPES = {"enlarged": (12, 16), "reduced": (40, 56), "same": (37, 53)}
LARGE_GT, LARGE_PRED = (197, 293), (64, 96)  # 57,721 pixels: 29 workgroups of 2048, the last one with 377
RESIZE_PAIRS = ((12, 37), (16, 53), (40, 37), (56, 53), (37, 37), (96, 768), (5, 64), (7, 3), (100, 33), (64, 197), (96, 293))


def nearest_index(n_in, n_out):
    o = np.arange(n_out, dtype=np.float64)
    return np.clip(np.floor((o + 0.5) * (np.float64(n_in) / np.float64(n_out))), 0, n_in - 1).astype(np.int64)


def surface(shape, rng_phase=0.0):
    """A smooth positive depth surface sampled at the pixel centres of a `shape` grid over the unit square."""
    y = (np.arange(shape[0]) + 0.5) / shape[0]
    x = (np.arange(shape[1]) + 0.5) / shape[1]
    return (2.0 + 1.5 * np.sin(3.0 * x[None] + rng_phase) * np.cos(2.0 * y[:, None]) + 2.0 * y[:, None]).astype(np.float32)


def exact_uncertainty(rng, shape):
    """A permutation of k / 1024: distinct values whose (u - min + 1) float32 holds exactly."""
    n = shape[0] * shape[1]
    return (rng.permutation(n).astype(np.float32) / np.float32(1024.0)).reshape(shape)


def one_valid_per_source(rng, gt, pred_shape, keep=0.8):
    """Invalidates gt (0 or a negative value) everywhere except at most one pixel per source pixel of an enlarged prediction, so that
    the resized uncertainty has no two valid pixels with the same value."""
    H, W = gt.shape
    row, col = nearest_index(pred_shape[0], H), nearest_index(pred_shape[1], W)
    src = row[:, None] * pred_shape[1] + col[None]
    src = src.ravel()
    order = np.lexsort((rng.random(src.size), src))  # a random pixel of every source pixel's block comes first
    first = np.ones(src.size, bool)
    first[1:] = src[order][1:] != src[order][:-1]
    chosen = order[first]
    valid = np.zeros(gt.size, bool)
    valid[chosen[rng.random(chosen.size) < keep]] = True
    valid = valid.reshape(gt.shape)
    out = gt.copy()
    bad = rng.random(gt.shape) < 0.5
    out[~valid & bad] = 0.0
    out[~valid & ~bad] = -1.5
    return out


def score_case(name):
    """-> dict(gt, pred, unc, alignment, sparse_pred, clip) of one per-function case."""
    spec = SCORE_CASES[name]
    rng = np.random.default_rng(18000 + sorted(SCORE_CASES).index(name))
    pshape = PRED_SHAPES[spec["size"]]
    gt = surface(GT_SHAPE) * (1 + 0.05 * rng.standard_normal(GT_SHAPE)).astype(np.float32)
    pred = surface(pshape, 0.2) * (1 + 0.08 * rng.standard_normal(pshape)).astype(np.float32) * np.float32(spec.get("gain", 1.0))
    # special prediction pixels: 0, inf, NaN, a negative and a tiny one
    flat = pred.reshape(-1)
    picks = rng.choice(flat.size, 12, replace=False)
    flat[picks[:4]] = 0.0
    flat[picks[4:6]] = np.inf
    flat[picks[6:8]] = np.nan
    flat[picks[8]] = -2.0
    flat[picks[9]] = 1e-3
    flat[picks[10]] = 500.0
    if spec["size"] == "enlarged":
        gt = one_valid_per_source(rng, gt, pshape)
    else:
        bad = rng.random(GT_SHAPE)
        gt[bad < 0.15] = 0.0
        gt[(bad >= 0.15) & (bad < 0.25)] = -3.0
    if spec.get("empty"):
        gt = -np.abs(gt)
        gt[::3] = 0.0
    if "valid" in spec:  # exactly this many valid pixels
        resized = pred[nearest_index(pshape[0], GT_SHAPE[0])][:, nearest_index(pshape[1], GT_SHAPE[1])]
        usable = (gt > 0) & np.isfinite(resized) & (resized != 0)
        keep = rng.permutation(np.flatnonzero(usable.reshape(-1)))[:spec["valid"]]
        g = np.where(gt > 0, -gt, gt).reshape(-1)
        g[keep] = np.abs(g[keep])
        gt = g.reshape(GT_SHAPE)
        assert (gt > 0).sum() == spec["valid"]
    unc = exact_uncertainty(rng, pshape)
    return dict(gt=gt.astype(np.float32), pred=pred.astype(np.float32), unc=unc, alignment=spec["alignment"],
                sparse_pred=spec["sparse"], clip=spec["clip"])


MED, LSQ = "median", "least_squares_scale_shift"
SCORE_CASES = {
    "a_none_enl": dict(size="enlarged", alignment=None, sparse=False, clip=True),
    "b_none_red_sparse": dict(size="reduced", alignment=None, sparse=True, clip=True),
    "c_none_same_noclip": dict(size="same", alignment=None, sparse=True, clip=False),
    "d_med_enl_sparse": dict(size="enlarged", alignment=MED, sparse=True, clip=True, gain=1.7),
    "e_med_red": dict(size="reduced", alignment=MED, sparse=False, clip=(0.5, 20.0), gain=0.4),
    "f_med_same_noclip": dict(size="same", alignment=MED, sparse=True, clip=False, gain=3.0),
    "g_lsq_enl": dict(size="enlarged", alignment=LSQ, sparse=True, clip=True, gain=2.0),
    "h_lsq_red_sparse": dict(size="reduced", alignment=LSQ, sparse=True, clip=(0.5, 20.0), gain=0.6),
    "i_lsq_same_noclip": dict(size="same", alignment=LSQ, sparse=False, clip=False),
    "j_empty_med": dict(size="same", alignment=MED, sparse=True, clip=True, empty=True),
    "k_empty_lsq": dict(size="reduced", alignment=LSQ, sparse=False, clip=True, empty=True),
    "l_empty_none": dict(size="same", alignment=None, sparse=False, clip=True, empty=True),
    "v1": dict(size="same", alignment=None, sparse=True, clip=True, valid=1),
    "v2": dict(size="same", alignment=MED, sparse=True, clip=True, valid=2),
    "v50": dict(size="same", alignment=None, sparse=True, clip=True, valid=50),
    "v100": dict(size="same", alignment=LSQ, sparse=True, clip=True, valid=100),
    "v101": dict(size="same", alignment=MED, sparse=True, clip=True, valid=101),
}


def median_case(kind, count):
    """gt and pred (37,53) for the median select: `count` valid pixels (gt > 0), values of the given kind in both maps."""
    rng = np.random.default_rng(18100 + 7 * ["quantised", "top24", "mixed"].index(kind) + count % 2)
    n = GT_SHAPE[0] * GT_SHAPE[1]
    if kind == "quantised":  # a handful of distinct values: the median falls among ties
        g = rng.integers(1, 6, n).astype(np.float32) * np.float32(0.5)
        p = rng.integers(1, 4, n).astype(np.float32)
    elif kind == "top24":  # the keys differ only in their last 8 bits: the last digit pass decides
        g = (np.uint32(0x40490F00) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
        p = (np.uint32(0x3FC00000) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    else:  # mixed signs and exponents in the prediction, exponents in gt
        g = np.exp2(rng.uniform(-20, 20, n)).astype(np.float32)
        p = (np.exp2(rng.uniform(-30, 30, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    valid = np.zeros(n, bool)
    valid[rng.permutation(n)[:count]] = True
    g = np.where(valid, g, np.where(rng.random(n) < 0.5, 0.0, -g)).astype(np.float32)
    return g.reshape(GT_SHAPE), p.reshape(GT_SHAPE)


MEDIAN_CASES = [(k, c) for k in ("quantised", "top24", "mixed") for c in (1200, 1201)]


def large_case():
    rng = np.random.default_rng(18200)
    gt = surface(LARGE_GT) * (1 + 0.05 * rng.standard_normal(LARGE_GT)).astype(np.float32)
    gt = one_valid_per_source(rng, gt, LARGE_PRED, keep=0.9)
    pred = surface(LARGE_PRED, 0.2) * (1 + 0.08 * rng.standard_normal(LARGE_PRED)).astype(np.float32) * np.float32(1.3)
    flat = pred.reshape(-1)
    picks = rng.choice(flat.size, 40, replace=False)
    flat[picks[:20]] = 0.0
    flat[picks[20:30]] = np.inf
    flat[picks[30:]] = np.nan
    return dict(gt=gt.astype(np.float32), pred=pred.astype(np.float32), unc=exact_uncertainty(rng, LARGE_PRED))


# ---- the whole-class case: a tiny in-memory dataset and a lookup-table model ----

N_VIEWS = 4
LOOKUP_PRED = (12, 16)
SUBSET_ERR = {  # relative noise of the prediction a subset of source-view SLOTS (0..2, in view order without the key) gives
    (): 0.20, (0,): 0.05, (1,): 0.08, (2,): 0.02, (0, 1): 0.06, (0, 2): 0.01, (1, 2): 0.04, (0, 1, 2): 0.03,
}  # single views rank 2, 0, 1 (not the nearest order 0, 1, 2); the prefixes (2,), (0,2), (0,1,2) give 0.02, 0.01, 0.03: best has 2


def lookup_dataset():
    """-> (samples, table): 2 unbatched sample dicts (key view 0 and key view 1; every image filled with 10 * sample + view) and
    table[(sample, subset of source VIEW indices)] = (pred, unc) of shape (12,16)."""
    samples, table = [], {}
    for s, key in enumerate((0, 1)):
        rng = np.random.default_rng(18300 + s)
        gt = surface(GT_SHAPE, 0.3 * s) * (1 + 0.03 * rng.standard_normal(GT_SHAPE)).astype(np.float32)
        gt = one_valid_per_source(rng, gt, LOOKUP_PRED, keep=0.85).astype(np.float32)
        sources = [v for v in range(N_VIEWS) if v != key]
        noise = rng.standard_normal(LOOKUP_PRED).astype(np.float32)  # one pattern per sample: absrel follows SUBSET_ERR
        for slots, err in SUBSET_ERR.items():
            pred = (surface(LOOKUP_PRED, 0.3 * s) * (1 + np.float32(err) * noise)).astype(np.float32)
            pred.reshape(-1)[rng.choice(pred.size, 3, replace=False)] = 0.0
            table[(s, tuple(sources[i] for i in slots))] = (pred, exact_uncertainty(rng, LOOKUP_PRED))
        pose = np.eye(4, dtype=np.float32)
        K = np.array([[50, 0, 8], [0, 50, 6], [0, 0, 1]], np.float32)
        with np.errstate(divide="ignore"):
            inv = np.where(gt > 0, 1 / gt, 0).astype(np.float32)
        samples.append(dict(images=[np.full((3, 24, 32), 10 * s + v, np.float32) for v in range(N_VIEWS)],
                            poses=[pose.copy() for _ in range(N_VIEWS)], intrinsics=[K.copy() for _ in range(N_VIEWS)],
                            keyview_idx=key, depth=gt[None], invdepth=inv[None], depth_range=(np.float32(1.0), np.float32(8.0))))
    return samples, table


class LookupModel:
    """model(images, keyview_idx, ...) -> {"depth", "depth_uncertainty"} (1,1,12,16) from the table; `to` converts the arrays
    (identity = numpy, or a function that uploads them)."""
    name = "lookup"

    def __init__(self, table, to=lambda a: a):
        self.table, self.to, self.calls = table, to, 0

    def __call__(self, images, keyview_idx, **_):
        self.calls += 1
        ids = [int(round(float(np.asarray(im).reshape(-1)[0]))) for im in images]
        key = int(np.asarray(keyview_idx).reshape(-1)[0])
        s = ids[key] // 10
        subset = tuple(sorted(i % 10 for k, i in enumerate(ids) if k != key))
        pred, unc = self.table[(s, subset)]
        return {"depth": self.to(pred[None, None].copy()), "depth_uncertainty": self.to(unc[None, None].copy())}


EVAL_CONFIGS = {
    "quasi_none": dict(inputs=["poses", "intrinsics"], alignment=None, view_ordering="quasi-optimal", sparse_pred=True),
    "quasi_median": dict(inputs=["poses", "intrinsics"], alignment=MED, view_ordering="quasi-optimal", sparse_pred=True),
    "nearest_lsq": dict(inputs=["poses", "intrinsics"], alignment=LSQ, view_ordering="nearest", sparse_pred=True,
                        clip_pred_depth=(0.5, 20.0)),
    "single_view": dict(inputs=None, alignment=MED, max_source_views=0, sparse_pred=False),
}
TIMING_COLUMNS = ("runtime_model_in_sec", "runtime_model_in_msec", "runtime_model_and_io_in_sec", "runtime_model_and_io_in_msec",
                  "gpu_mem_alloc_in_mib", "gpu_mem_reserved_in_mib")
