"""Scoring of one predicted depth map against a ground truth: what the multi-view depth evaluation (eval.py) does after every
model run.  Two implementations of the same arithmetic:

  DeviceScorer     the HIP kernels of csrc/depth_eval.hip on the prediction where the model left it (a GPU tensor)
  score_numpy      numpy on the host, for predictions that are on the CPU

Both restate rmvd/eval/multi_view_depth_evaluation.py:469-547,583-610 and rmvd/eval/metrics.py:32-220 and return a Score, from
which metrics() and sparsification_curve() form the reference's numbers.  Per-pixel maps, counts and medians are the reference's
bit for bit; quantities that come from sums (absrel, the curves, the least-squares parameters) are formed from float64 sums where
the reference adds float32 pairwise.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

ALIGNMENTS = (None, "median", "least_squares_scale_shift")
INLIER_THRESH = 1.03
NUM_STEPS = 100


def resize_index(n_in, n_out):
    """Input index that output index o reads in skimage.transform.resize(order=0, anti_aliasing=False), i.e. in
    scipy.ndimage.zoom(order=0, mode="mirror", grid_mode=True): floor((o + 0.5) * (n_in / n_out)) in float64, clamped.  The quotient
    is formed first, as scipy does; multiplying by n_in before dividing gives another index for some sizes (64 -> 197 at o = 98)."""
    o = np.arange(n_out, dtype=np.float64)
    return np.clip(np.floor((o + 0.5) * (np.float64(n_in) / np.float64(n_out))), 0, n_in - 1).astype(np.int32)


@functools.lru_cache(maxsize=64)
def resize_tables(h, w, H, W):
    """(row[H], col[W]) int32: the nearest resize (h,w) -> (H,W) as a gather, resized = pred[row][:, col]."""
    row, col = resize_index(h, H), resize_index(w, W)
    row.setflags(write=False)
    col.setflags(write=False)
    return row, col


def normalize_clip(clip_pred_depth):
    """clip_pred_depth of the evaluation -> (lo, hi) or None (multi_view_depth_evaluation.py:531-534)."""
    if isinstance(clip_pred_depth, tuple):
        return float(clip_pred_depth[0]), float(clip_pred_depth[1])
    return (0.1, 100.0) if clip_pred_depth else None


@dataclass
class Score:
    """One run's result.  The maps are None unless they were asked for; on the device path they are GPU tensors."""
    sum_rel_ae: float
    n_mask: int
    n_inliers: int
    n_eval: int
    n_pixels: int
    min_rel_ae: float
    alignment: str = None
    ratio: float = float("nan")      # median: the scaling factor, NaN when the prediction was left unscaled
    scale: float = float("nan")      # least squares
    shift: float = float("nan")
    median_gt: float = float("nan")
    median_pred: float = float("nan")
    uncertainty_min: float = float("nan")
    pred_depth: object = None
    pred_invdepth: object = None
    rel_ae: object = None
    uncertainty: object = None
    extra: dict = field(default_factory=dict)


def metrics(score):
    """The metrics dict of _compute_metrics (:583-610) from a Score."""
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.float64(score.sum_rel_ae) / np.float64(score.n_mask)
        absrel = float(mean * 100.0) if np.isfinite(mean) else np.nan
        # inliers are counted exactly, so this is the reference's float32 quotient and product
        ratio = np.float32(score.n_inliers) / np.float32(score.n_mask)
        inliers = float(ratio * np.float32(100.0)) if np.isfinite(ratio) else np.nan
    out = {"absrel": absrel, "inliers103": inliers}
    if score.alignment == "median":
        out["scaling_factor"] = score.ratio
    if score.alignment == "least_squares_scale_shift":
        out["least_squares_scale"] = score.scale
        out["least_squares_shift"] = score.shift
    out["pred_depth_density"] = score.n_eval / score.n_pixels * 100
    return out


def sparsification_steps(num_valid):
    return [int((num_valid / 100) * i) for i in range(NUM_STEPS)]  # metrics.py:176, float64 like np.int64 / 100


def sparsification_curve(num_valid, step_sums):
    """The curve of metrics.py:138-220 in closed form.  step_sums[i] = sum of the errors that remain once the
    sparsification_steps(num_valid)[i] highest-ranked valid pixels are removed.  The reference evaluates the mean error at each
    DISTINCT step (its loop meets every count once), divides by the error at step 0 and interpolates onto 0, 0.01 .. 0.99."""
    x = np.linspace(0, 0.99, NUM_STEPS)
    steps = sparsification_steps(num_valid)
    xs, ys = [], []
    if num_valid > 0:
        with np.errstate(divide="ignore", invalid="ignore"):
            base = np.float64(step_sums[0]) / num_valid
            for i, s in enumerate(steps):
                if i > 0 and s == steps[i - 1]:
                    continue
                cur = np.float64(step_sums[i]) / (num_valid - s)
                if np.isfinite(cur):
                    xs.append(s / num_valid)
                    ys.append(cur / base)
    if len(xs) > 1:
        return np.interp(x, xs, ys)
    return np.full(NUM_STEPS, np.nan)


def ause(curve_oracle, curve_pred):
    """-> (error curve, AUSE) as _compute_uncertainty_metrics (:644-646)."""
    err = curve_pred - curve_oracle
    a = err.sum() / 100
    return err, (a if np.isfinite(a) else np.nan)


# ---- host path ---------------------------------------------------------------------------------------------------------------------

def _nan_to_num(x, fill=0.0):
    return np.nan_to_num(x, nan=fill, posinf=fill, neginf=fill)


def align_numpy(gt, pred, alignment, sparse_pred):
    """gt, pred (H,W) float32, pred already resized -> dict(ratio | scale, shift, median_gt, median_pred, sums)."""
    mask = (gt > 0) & ((pred != 0) if sparse_pred else True)
    out = {}
    with np.errstate(all="ignore"):
        if alignment == "median":
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)  # np.median of an empty selection
                mg, mp = np.median(gt[mask]), np.median(pred[mask])
            ratio = mg / mp
            out.update(median_gt=float(mg), median_pred=float(mp),
                       ratio=np.float32(ratio) if mask.any() and np.isfinite(ratio) else np.nan)
        elif alignment == "least_squares_scale_shift":
            p = _nan_to_num(1 / pred)[mask].astype(np.float64)
            g = _nan_to_num(1 / gt)[mask].astype(np.float64)
            a00, a01, a11, b0, b1 = np.sum(p * p), np.sum(p), np.float64(mask.sum()), np.sum(g * p), np.sum(g)
            det = a00 * a11 - a01 * a01
            scale = shift = np.nan
            if mask.any() and det > 0:
                scale = np.float32((a11 * b0 - a01 * b1) / det)
                shift = np.float32((-a01 * b0 + a00 * b1) / det)
            out.update(scale=scale, shift=shift, sums=np.array([a00, a01, a11, b0, b1]))
    return out


def score_numpy(gt, pred, uncertainty=None, alignment=None, sparse_pred=False, clip=(0.1, 100.0), maps=False, params=None):
    """gt (H,W), pred and uncertainty (h,w) numpy float32 -> Score.  `params`: explicit alignment parameters (ratio,) or
    (scale, shift) instead of the ones computed from the maps."""
    assert alignment in ALIGNMENTS, alignment
    gt = np.ascontiguousarray(gt, dtype=np.float32)
    pred = np.ascontiguousarray(pred, dtype=np.float32)
    row, col = resize_tables(pred.shape[0], pred.shape[1], gt.shape[0], gt.shape[1])
    pred = pred[row][:, col]
    s = Score(0.0, 0, 0, 0, gt.size, np.nan, alignment=alignment)
    pred_mask = (pred != 0) if sparse_pred else np.ones_like(pred, dtype=bool)
    with np.errstate(all="ignore"):
        if alignment is not None:
            a = align_numpy(gt, pred, alignment, sparse_pred)
            s.extra.update(a)
        if alignment == "median":
            s.ratio = a["ratio"] if params is None else np.float32(params[0])
            s.median_gt, s.median_pred = a["median_gt"], a["median_pred"]
            if np.isfinite(s.ratio):
                pred = pred * np.float32(s.ratio)
        elif alignment == "least_squares_scale_shift":
            s.scale, s.shift = (a["scale"], a["shift"]) if params is None else (np.float32(params[0]), np.float32(params[1]))
            inv = np.float32(s.scale) * _nan_to_num(1 / pred) + np.float32(s.shift)
            pred = _nan_to_num(1 / inv)
        if clip is not None:
            pred = np.clip(pred, np.float32(clip[0]), np.float32(clip[1])) * pred_mask
        pred = pred.astype(np.float32, copy=False)
        invdepth = _nan_to_num(1 / pred)
        eval_mask = (pred != 0) if sparse_pred else np.ones_like(pred, dtype=bool)
        mask = (gt > 0).astype(np.float32) * eval_mask
        rel_ae = _nan_to_num(np.abs(pred - gt) / gt) * mask
        rel_1 = _nan_to_num(gt / pred, np.float32(INLIER_THRESH + 1))
        rel_2 = _nan_to_num(pred / gt)
        max_rel = np.maximum(rel_1, rel_2)
        inliers = (0 < max_rel) & (max_rel < np.float32(INLIER_THRESH)) & (mask != 0)
    s.sum_rel_ae = float(np.sum(rel_ae, dtype=np.float64))
    s.n_mask, s.n_inliers, s.n_eval = int((mask != 0).sum()), int(inliers.sum()), int(eval_mask.sum())
    s.min_rel_ae = float(rel_ae.min())
    if uncertainty is not None:
        unc = np.ascontiguousarray(uncertainty, dtype=np.float32)[row][:, col]
        s.uncertainty_min = float(unc.min())
        if maps:
            s.uncertainty = unc
    if maps:
        s.pred_depth, s.pred_invdepth, s.rel_ae = pred, invdepth, rel_ae
    return s


def rank_keys_numpy(u, gt, pred_depth, sparse_pred):
    mask = (gt > 0).astype(np.float32) * ((pred_depth != 0) if sparse_pred else np.ones_like(pred_depth, dtype=bool))
    with np.errstate(all="ignore"):
        return ((u - u.min() + 1) * mask).astype(np.float32)  # metrics.py:169


def ranked_step_sums_numpy(rel_ae, keys, num_valid):
    """Errors ranked by descending key (ties in index order, as a stable sort leaves them) -> the 100 float64 suffix sums."""
    order = np.argsort(-keys.ravel(), kind="stable")
    ranked = rel_ae.ravel()[order][:num_valid].astype(np.float64)
    from_end = np.concatenate([[0.0], np.cumsum(ranked[::-1])])  # from_end[k] = sum of the last k
    return np.array([from_end[num_valid - s] for s in sparsification_steps(num_valid)]) if num_valid > 0 else np.zeros(NUM_STEPS)


def uncertainty_curves_numpy(gt, score, sparse_pred):
    """-> (oracle curve, prediction curve) of a Score with maps."""
    out = []
    for u in (score.rel_ae, score.uncertainty):
        keys = rank_keys_numpy(u, gt, score.pred_depth, sparse_pred)
        out.append(sparsification_curve(score.n_mask, ranked_step_sums_numpy(score.rel_ae, keys, score.n_mask)))
    return out


# ---- device path -------------------------------------------------------------------------------------------------------------------

_MODE = {None: 0, "median": 1, "least_squares_scale_shift": 2}


class DeviceScorer:
    """Scores predictions against ONE ground truth on the GPU.  The ground truth is uploaded here, once; every score() runs the
    kernels on the current stream and reads back 72 bytes."""

    def __init__(self, gt, device, alignment=None, sparse_pred=False, clip=(0.1, 100.0)):
        import torch
        from . import ops  # here, not at the top: the numpy half of this module works without the library
        assert alignment in ALIGNMENTS, alignment
        self.ops, self.torch = ops, torch
        self.device = torch.device(device)
        if not isinstance(gt, torch.Tensor):
            gt = torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float32))
        if gt.ndim != 2:
            raise ValueError(f"gt: expected (H,W), got {tuple(gt.shape)}")
        self.gt = ops.L.as_f32(gt.to(self.device), "gt")
        self.H, self.W = self.gt.shape
        self.alignment, self.sparse_pred, self.clip = alignment, bool(sparse_pred), clip
        self.ws_bytes = ops.L.load().mvd_depth_eval_workspace_bytes(self.H, self.W)
        self.ws = ops.workspace(self.ws_bytes, self.device)
        self._tables = {}

    def tables(self, h, w):
        if (h, w) not in self._tables:
            row, col = resize_tables(h, w, self.H, self.W)
            self._tables[(h, w)] = tuple(self.torch.from_numpy(np.array(t)).to(self.device) for t in (row, col))
        return self._tables[(h, w)]

    def _map2d(self, t, name, shape=None):
        if t.ndim > 2:
            if t.numel() != t.shape[-2] * t.shape[-1]:
                raise ValueError(f"{name}: expected one (h,w) map, got {tuple(t.shape)}")
            t = t.reshape(t.shape[-2], t.shape[-1])
        return self.ops.L.as_f32(t, name, shape, self.device)

    def align_stats(self, pred, uncertainty=None, alignment="same"):
        """-> (params, sums): 8 floats and 5 doubles on the device (include/mvd.h: mvd_depth_align_stats_f32)."""
        torch = self.torch
        alignment = self.alignment if alignment == "same" else alignment
        pred = self._map2d(pred, "pred")
        unc = self._map2d(uncertainty, "uncertainty", pred.shape) if uncertainty is not None else None
        row, col = self.tables(*pred.shape)
        params = torch.empty(8, dtype=torch.float32, device=self.device)
        sums = torch.zeros(5, dtype=torch.float64, device=self.device)
        self.ops.call("mvd_depth_align_stats_f32", self.device, self.gt, pred, unc, row, col, self.H, self.W, pred.shape[0],
                      pred.shape[1], _MODE[alignment], int(self.sparse_pred), params, sums, self.ws, self.ws_bytes)
        return params, sums

    def score(self, pred, uncertainty=None, maps=False, params=None):
        """pred, uncertainty: GPU tensors with one (h,w) map -> Score (its maps stay on the device).  `params`: explicit alignment
        parameters, a sequence (ratio,) / (scale, shift) or a device tensor of at least 2 floats, instead of the computed ones."""
        call, torch = self.ops.call, self.torch
        pred = self._map2d(pred, "pred")
        unc = self._map2d(uncertainty, "uncertainty", pred.shape) if uncertainty is not None else None
        row, col = self.tables(*pred.shape)
        h, w = pred.shape
        out = torch.empty(9, dtype=torch.int64, device=self.device)  # 40 bytes of result, then the 8 floats of the parameters
        stats = out[5:].view(torch.float32)
        need_stats = unc is not None or (self.alignment is not None and params is None)
        if need_stats:
            call("mvd_depth_align_stats_f32", self.device, self.gt, pred, unc, row, col, self.H, self.W, h, w,
                 _MODE[self.alignment] if params is None else 0, int(self.sparse_pred), stats, None, self.ws, self.ws_bytes)
        else:
            stats.fill_(float("nan"))
        if params is not None and self.alignment is not None:
            if isinstance(params, torch.Tensor):
                stats[:2].copy_(params[:2])
            else:
                p = list(params) + [0.0]
                stats[:2].copy_(torch.tensor(p[:2], dtype=torch.float32), non_blocking=False)
        new = lambda: torch.empty((self.H, self.W), dtype=torch.float32, device=self.device)
        m_pred, m_inv, m_rel = (new(), new(), new()) if maps else (None, None, None)
        m_unc = new() if maps and unc is not None else None
        clip = self.clip
        call("mvd_depth_score_f32", self.device, self.gt, pred, unc, row, col, self.H, self.W, h, w, _MODE[self.alignment],
             int(self.sparse_pred), int(clip is not None), float(clip[0]) if clip else 0.0, float(clip[1]) if clip else 0.0, INLIER_THRESH,
             INLIER_THRESH + 1, stats, out, m_pred, m_inv, m_rel, m_unc, self.ws, self.ws_bytes)
        host = out.cpu().numpy()  # the run's one device-to-host read
        f = host[5:].view(np.float32)
        s = Score(float(host[:1].view(np.float64)[0]), int(host[1]), int(host[2]), int(host[3]), self.H * self.W,
                  float(host[4:5].view(np.float32)[0]), alignment=self.alignment)
        if self.alignment == "median":
            s.ratio, s.median_gt, s.median_pred = (np.float32(f[0]) if np.isfinite(f[0]) else np.nan), float(f[2]), float(f[3])
        elif self.alignment == "least_squares_scale_shift":
            s.scale, s.shift = (np.float32(f[0]) if np.isfinite(f[0]) else np.nan), (np.float32(f[1]) if np.isfinite(f[0]) else np.nan)
        s.uncertainty_min = float(f[5])
        s.pred_depth, s.pred_invdepth, s.rel_ae, s.uncertainty = m_pred, m_inv, m_rel, m_unc
        s.extra["device_out"] = out
        return s

    def rank_keys(self, u, u_min, pred_depth):
        """((u - u_min) + 1) * mask; u_min: a device tensor whose first float is the minimum."""
        keys = self.torch.empty(self.H * self.W, dtype=self.torch.float32, device=self.device)
        self.ops.call("mvd_rank_keys_f32", self.device, u, u_min, self.gt, pred_depth, int(self.sparse_pred), self.H * self.W, keys)
        return keys

    def ranked_step_sums(self, ranked, count, out=None):
        """ranked: the errors in ranked order; count: device int64 tensor -> 100 float64 sums on the device."""
        out = self.torch.empty(NUM_STEPS, dtype=self.torch.float64, device=self.device) if out is None else out
        self.ops.call("mvd_ranked_step_sums_f64", self.device, ranked, ranked.numel(), count, out, self.ws, self.ws_bytes)
        return out

    def uncertainty_curves(self, score):
        """-> (oracle curve, prediction curve) of a Score from score(..., maps=True) with an uncertainty: two rankings
        (mvd_rank_keys_f32, a stable descending torch.sort, a gather), their step sums, and one read of the 200 sums."""
        torch = self.torch
        dev_out = score.extra["device_out"]
        as_f32 = dev_out.view(torch.float32)
        sums = torch.empty((2, NUM_STEPS), dtype=torch.float64, device=self.device)
        rel = score.rel_ae.reshape(-1)
        for i, (u, u_min) in enumerate(((score.rel_ae, as_f32[8:9]), (score.uncertainty, as_f32[15:16]))):
            keys = self.rank_keys(u, u_min, score.pred_depth)
            order = torch.sort(keys, descending=True, stable=True).indices
            self.ranked_step_sums(rel[order], dev_out[1:2], out=sums[i])
        sums = sums.cpu().numpy()
        return [sparsification_curve(score.n_mask, sums[i]) for i in range(2)]
