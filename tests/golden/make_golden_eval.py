#!/usr/bin/env python3
"""Generate tests/golden/g18_eval.npz (per-function cases), g18_eval_large.npz (the multi-workgroup case) and g18_eval_class.npz (the
whole evaluation on a lookup model): results of the REFERENCE's own rmvd/eval/metrics.py and multi_view_depth_evaluation.py.

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_eval.py

The two files are loaded with importlib under their dotted names, with stand-ins for what they import and this image lacks:
skimage.transform.resize(order=0, anti_aliasing=False) -> scipy.ndimage.zoom(order=0, mode="mirror", grid_mode=True), which is what
skimage delegates to; thin rmvd.utils (this package's numpy_collate / select_by_index, a silent logging and writer), rmvd.data.layout
and rmvd.data.updates; in metrics.py an np whose nan_to_num ignores copy= (NumPy 2 refuses copy=False on a scalar); the torch.cuda
memory calls are stubbed.  Everything stored is computed by the reference's own functions and methods (_postprocess_sample_and_output,
_compute_metrics, _compute_uncertainty_metrics, sparsification, and the whole class with out_dir=None), except the ranking keys,
which metrics.py:169 forms inline: they are restated here with the same expression.

Inputs come from tests/eval_cases.py (seeded).  Conditions asserted: the predicted-uncertainty ranking keys of the valid pixels are
distinct in every case (the reference's argsort is unstable: tied keys would make its own answer arbitrary); tied oracle keys belong
to errors within one key ulp of each other; the lookup model's quasi-optimal order differs from the nearest order and its best run is
not the one with most views.

Tolerances.  absrel, the curves, the AUSE and the least-squares parameters come from sums that the reference forms in float32
(pairwise) and the package in float64.  For each of them the reference's formula is evaluated once more with float64 sums
(sparsification() itself with a float64 error function, on maps flipped in both axes so that ranking ties break in another order)
and tol_* = 2 x the largest relative gap to the reference's float32 value over all cases, at least 4 float32 ulps.  The values are
printed and stored.
"""
import importlib.util
import math
import os
import sys
import types
import warnings

import numpy as np
import scipy.ndimage
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import eval_cases as EC  # noqa: E402
from _ref_loader import REF_ROOT  # noqa: E402
from robustmvd_amd import utils as U  # noqa: E402

ULP4 = 4 * float(np.finfo(np.float32).eps)


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _load(name, relpath):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, relpath))
    m = importlib.util.module_from_spec(spec)
    m.__package__ = name.rpartition(".")[0]
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


class _NumpyIgnoringCopy:
    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def nan_to_num(x, copy=True, **kw):
        return np.nan_to_num(x, **kw)


def load_reference_eval():
    def resize(image, output_shape, order=0, anti_aliasing=False):
        assert order == 0 and not anti_aliasing
        zoom = [o / i for o, i in zip(output_shape, image.shape)]
        return scipy.ndimage.zoom(image, zoom, order=0, mode="mirror", grid_mode=True)

    sk = _mod("skimage")
    sk.__path__ = []
    sk.transform = _mod("skimage.transform", resize=resize)
    quiet = types.SimpleNamespace(info=lambda *a, **k: None, add_log_file=lambda *a, **k: None, remove_log_file=lambda *a, **k: None)
    writer = types.SimpleNamespace(put_scalar_dict=lambda **k: None, write_out_storage=lambda: None)
    for pkg in ("rmvd", "rmvd.data", "rmvd.eval"):
        _mod(pkg).__path__ = []
    _mod("rmvd.utils", numpy_collate=U.numpy_collate, select_by_index=U.select_by_index, vis=None,
         get_full_class_name=lambda o: type(o).__name__, writer=writer, logging=quiet)
    _mod("rmvd.data.layout", Layout=object, Visualization=object)
    _mod("rmvd.data.updates", Update=object)
    for f in ("empty_cache", "reset_peak_memory_stats", "reset_accumulated_memory_stats"):
        setattr(torch.cuda, f, lambda *a, **k: None)
    torch.cuda.max_memory_allocated = torch.cuda.max_memory_reserved = lambda *a, **k: 0
    metrics = _load("rmvd.eval.metrics", "rmvd/eval/metrics.py")
    metrics.np = _NumpyIgnoringCopy()
    mvde = _load("rmvd.eval.multi_view_depth_evaluation", "rmvd/eval/multi_view_depth_evaluation.py")
    return metrics, mvde


def rel_gap(a, b):
    """largest |a - b| / |b| over the entries where both are finite and b != 0"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    ok = np.isfinite(a) & np.isfinite(b) & (b != 0)
    assert np.array_equal(np.isfinite(a), np.isfinite(b)), "float32 and float64 evaluations disagree on what is finite"
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0


def reference_case(metrics, mvde, gt, pred, unc, alignment, sparse_pred, clip, gaps, want_maps=True):
    ev = mvde.MultiViewDepthEvaluation(out_dir=None, alignment=alignment, clip_pred_depth=clip, sparse_pred=sparse_pred, verbose=False)
    ev._init_results()
    g = {"depth": gt[None, None]}
    p = {"depth": pred[None, None].copy(), "depth_uncertainty": unc[None, None].copy()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        resized_raw = sys.modules["skimage.transform"].resize(pred, gt.shape, order=0, anti_aliasing=False)
        ev._postprocess_sample_and_output({}, g, p)
        m = ev._compute_metrics({}, g, p)
        ev._compute_uncertainty_metrics({}, g, p)
        ause = (ev.sparsification_curves.loc[(0, "error")].astype(np.float64).sum(skipna=False)) / 100
    ause = ause if np.isfinite(ause) else np.nan
    depth, invdepth, uncr = p["depth"][0, 0], p["invdepth"][0, 0], p["depth_uncertainty"][0, 0]
    pmask = depth != 0 if sparse_pred else np.ones_like(depth, dtype=bool)
    rel = metrics.pointwise_rel_ae(gt=gt, pred=depth, mask=pmask)
    mask = (gt > 0).astype(np.float32) * pmask
    with np.errstate(all="ignore"):
        keys_oracle = (rel - rel.min() + 1) * mask  # metrics.py:169
        keys_pred = (uncr - uncr.min() + 1) * mask
    valid = mask != 0
    assert len(np.unique(keys_pred[valid])) == valid.sum(), "tied predicted-uncertainty keys"
    ko, order = keys_oracle[valid], np.argsort(keys_oracle[valid], kind="stable")
    tied = np.flatnonzero(np.diff(ko[order]) == 0)
    if tied.size:  # tied oracle keys: the errors are within one ulp of the key
        r = rel[valid][order]
        assert np.all(np.abs(r[tied + 1] - r[tied]) <= np.spacing(ko[order][tied])), "tied oracle keys with different errors"
    curves = np.stack([ev.sparsification_curves.loc[(0, c)].to_numpy(np.float64) for c in ("oracle", "pred", "error")])
    out = dict(resized_index_check=resized_raw, pred_depth=depth, invdepth=invdepth, rel_ae=rel, unc_resized=uncr, keys_oracle=keys_oracle,
               keys_pred=keys_pred, absrel=np.float64(m["absrel"]), inliers103=np.float64(m["inliers103"]),
               density=np.float64(m["pred_depth_density"]), n_mask=np.int64(valid.sum()), curves=curves, ause=np.float64(ause))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sel = (gt > 0) & ((resized_raw != 0) if sparse_pred else True)
        out["median_gt"], out["median_pred"] = np.float32(np.median(gt[sel])), np.float32(np.median(resized_raw[sel]))
    if alignment == "median":
        out["scaling_factor"] = np.float32(m["scaling_factor"])
    if alignment == "least_squares_scale_shift":
        out["lsq"] = np.array([m["least_squares_scale"], m["least_squares_shift"]], np.float32)
        with np.errstate(all="ignore"):
            pi = np.nan_to_num(1 / resized_raw, nan=0, posinf=0, neginf=0)[sel].astype(np.float64)
            gi = np.nan_to_num(1 / gt, nan=0, posinf=0, neginf=0)[sel].astype(np.float64)
        a00, a01, a11, b0, b1 = math.fsum(pi * pi), math.fsum(pi), float(sel.sum()), math.fsum(gi * pi), math.fsum(gi)
        det = a00 * a11 - a01 * a01
        if sel.any() and det > 0:
            gaps["lsq"].append(rel_gap(out["lsq"], [(a11 * b0 - a01 * b1) / det, (-a01 * b0 + a00 * b1) / det]))

    # the same formulas with float64 sums, ranking ties broken in another order
    def err64(gt, pred, mask):
        r = metrics.pointwise_rel_ae(gt=gt, pred=pred, mask=None).astype(np.float64)
        return np.sum(r * mask) / np.sum(mask) if np.sum(mask) > 0 else np.nan

    f = lambda a: np.ascontiguousarray(a[::-1, ::-1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a64 = err64(gt, depth, mask) * 100.0
        c64 = [metrics.sparsification(gt=f(gt), pred=f(depth), uncertainty=f(u), mask=f(pmask), error_fct=err64).to_numpy(np.float64)
               for u in (rel, uncr)]
    gaps["absrel"].append(rel_gap(out["absrel"], a64))
    gaps["curve"].append(max(rel_gap(curves[0], c64[0]), rel_gap(curves[1], c64[1])))
    ause64 = (c64[1] - c64[0]).sum() / 100
    gaps["ause"].append(rel_gap(out["ause"], ause64 if np.isfinite(ause64) else np.nan))
    if not want_maps:
        for k in ("resized_index_check", "pred_depth", "invdepth", "rel_ae", "unc_resized", "keys_oracle", "keys_pred"):
            del out[k]
    return out


class _Dataset:
    name = "lookup"

    def __init__(self, samples):
        self.samples = samples

    def __len__(self):
        return len(self.samples)

    def get_loader(self, batch_size, indices, num_workers, collate_fn):
        return (collate_fn([self.samples[i]]) for i in indices)


def main():
    metrics, mvde = load_reference_eval()
    gaps = {"absrel": [], "curve": [], "ause": [], "lsq": []}
    small = {}
    for name in EC.SCORE_CASES:
        c = EC.score_case(name)
        ref = reference_case(metrics, mvde, c["gt"], c["pred"], c["unc"], c["alignment"], c["sparse_pred"], c["clip"], gaps)
        if "valid" in EC.SCORE_CASES[name]:
            assert ref["n_mask"] == EC.SCORE_CASES[name]["valid"], (name, ref["n_mask"])
        if EC.SCORE_CASES[name].get("empty"):
            assert ref["n_mask"] == 0 and np.isnan(ref["absrel"]) and np.isnan(ref["inliers103"]) and np.isnan(ref["ause"])
        del ref["resized_index_check"]
        for k, v in ref.items():
            small[f"{name}/{k}"] = v
    for kind, count in EC.MEDIAN_CASES:
        g, p = EC.median_case(kind, count)
        sel = g > 0
        assert sel.sum() == count
        small[f"median_{kind}_{count}/gt"], small[f"median_{kind}_{count}/pred"] = np.float32(np.median(g[sel])), np.float32(np.median(p[sel]))
        ev = mvde.MultiViewDepthEvaluation(out_dir=None, alignment="median", clip_pred_depth=False, sparse_pred=False, verbose=False)
        pd_ = {"depth": p[None, None].copy()}
        ev._postprocess_sample_and_output({}, {"depth": g[None, None]}, pd_)
        small[f"median_{kind}_{count}/scaling_factor"] = np.float32(pd_["scaling_factor"])

    lc = EC.large_case()
    large = {}
    for tag, (alignment, sparse, clip) in {"median": ("median", True, True), "lsq": ("least_squares_scale_shift", True, (0.5, 20.0)),
                                            "none": (None, False, False)}.items():
        ref = reference_case(metrics, mvde, lc["gt"], lc["pred"], lc["unc"], alignment, sparse, clip, gaps, want_maps=False)
        for k, v in ref.items():
            large[f"{tag}/{k}"] = v

    tol = {k: max(2 * max(v), ULP4) for k, v in gaps.items()}
    for k, v in tol.items():
        print(f"tol_{k} = {v:.3e}   (largest gap {max(gaps[k]):.3e} over {len(gaps[k])} cases)")
        small[f"tol_{k}"] = large[f"tol_{k}"] = np.float64(v)

    # the whole class on the lookup model
    samples, table = EC.lookup_dataset()
    cls = {f"tol_{k}": np.float64(v) for k, v in tol.items()}
    for cfg_name, cfg in EC.EVAL_CONFIGS.items():
        ev = mvde.MultiViewDepthEvaluation(out_dir=None, verbose=False, eval_uncertainty=True, **cfg)
        model = EC.LookupModel(table)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = ev(dataset=_Dataset(samples), model=model, burn_in_samples=0)
            curves = None
            # the curves frame is reset after the call: run _evaluate once more on a fresh instance to read it
            ev2 = mvde.MultiViewDepthEvaluation(out_dir=None, verbose=False, eval_uncertainty=True, **cfg)
            ev2._init_evaluation(dataset=_Dataset(samples), model=EC.LookupModel(table), burn_in_samples=0)
            ev2._evaluate()
            curves = ev2.sparsification_curves
            orders = []
            for smp in samples:
                inp, gtd = ev2._inputs_and_gt_from_sample(U.numpy_collate([smp]))
                orders.append(ev2._get_source_view_ordering(sample_inputs=inp, sample_gt=gtd))
                nearest = ev2._get_nearest_source_view_ordering(sample_inputs=inp, sample_gt=gtd)
                assert (orders[-1] != nearest) == (cfg.get("view_ordering") == "quasi-optimal" and cfg.get("max_source_views") != 0)
        cls[f"{cfg_name}/order"] = np.array(orders, np.int64)
        cols = [c for c in res.columns if c[1] not in EC.TIMING_COLUMNS]
        cls[f"{cfg_name}/columns"] = np.array([f"{c[0]}|{c[1]}" for c in cols])
        cls[f"{cfg_name}/values"] = np.array([[float(res.loc[i, c]) for c in cols] for i in res.index], np.float64)
        cls[f"{cfg_name}/index"] = np.array(list(res.index), np.int64)
        cls[f"{cfg_name}/curve_index"] = np.array([f"{i}|{c}" for i, c in curves.index])
        cls[f"{cfg_name}/curves"] = curves.to_numpy(np.float64)
        cls[f"{cfg_name}/model_calls"] = np.int64(model.calls)
        if cfg_name == "quasi_none":
            best = res[("best", "num_views")].to_numpy()
            assert np.all(best == 2), best  # not the run with most views
            one = [res.loc[0, (1, "absrel")], res.loc[1, (1, "absrel")]]
            print("quasi_none: best num_views", best, "absrel with 1 view", one)
    near = cls["nearest_lsq/values"][:, list(cls["nearest_lsq/columns"]).index("1|absrel")]
    quasi = cls["quasi_median/values"][:, list(cls["quasi_median/columns"]).index("1|absrel")]
    print("1-view absrel: nearest order", near, "quasi-optimal order", quasi)

    for fname, data in (("g18_eval.npz", small), ("g18_eval_large.npz", large), ("g18_eval_class.npz", cls)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **data)
        print(fname, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
