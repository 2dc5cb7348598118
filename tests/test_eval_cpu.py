"""CPU checks of the multi-view depth evaluation: the index tables, the numpy scoring path against the reference's results
(tests/golden/g18_eval*.npz, written by tests/golden/make_golden_eval.py), the whole evaluation on the lookup model, its output
files, and the argument checks of the new entries.  Per-pixel maps, keys, counts and medians must equal the reference's bit for
bit; absrel, curves, AUSE and the least-squares parameters within the fixture's tol_* (make_golden_eval.py says where they come
from)."""
import ctypes
import os

import numpy as np
import pytest

import eval_cases as EC
from robustmvd_amd import depth_score as DS


def assert_same_bits(a, b, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, what
    assert np.array_equal(a, b, equal_nan=True), f"{what}: {np.sum(~((a == b) | (np.isnan(a) & np.isnan(b))))} entries differ"


def assert_close(a, b, tol, what):
    """relative tolerance where the reference is finite and non-zero; NaN must meet NaN"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(b)
    assert np.all(np.abs(a[ok] - b[ok]) <= tol * np.abs(b[ok])), f"{what}: {np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300))} > {tol}"


def check_curves(oracle, pred, ref_curves, g, what):
    error, ause = DS.ause(oracle, pred)
    assert_close(oracle, ref_curves[0], g["tol_curve"], what + " oracle curve")
    assert_close(pred, ref_curves[1], g["tol_curve"], what + " pred curve")
    # the error curve is a difference of the two: each may be off by tol_curve of itself
    assert np.array_equal(np.isnan(error), np.isnan(ref_curves[2])), what
    if not np.isnan(error).any():
        assert np.all(np.abs(error - ref_curves[2]) <= g["tol_curve"] * (np.abs(ref_curves[0]) + np.abs(ref_curves[1]))), what
    return ause


def check_score(score, curves, g, prefix, maps=True):
    """A Score with host maps and its two curves against the fixture's entries prefix/*."""
    ref = lambda k: g[f"{prefix}/{k}"]
    m = DS.metrics(score)
    if maps:
        assert_same_bits(score.pred_depth, ref("pred_depth"), prefix + " pred_depth")
        assert_same_bits(score.pred_invdepth, ref("invdepth"), prefix + " invdepth")
        assert_same_bits(score.rel_ae, ref("rel_ae"), prefix + " rel_ae")
        assert_same_bits(score.uncertainty, ref("unc_resized"), prefix + " uncertainty")
    assert score.n_mask == int(ref("n_mask"))
    assert_same_bits(m["inliers103"], ref("inliers103"), prefix + " inliers103")
    assert m["pred_depth_density"] == float(ref("density"))
    assert_close(m["absrel"], ref("absrel"), g["tol_absrel"], prefix + " absrel")
    if score.alignment == "median":
        assert_same_bits(score.median_gt, ref("median_gt"), prefix + " median gt")
        assert_same_bits(score.median_pred, ref("median_pred"), prefix + " median pred")
        assert_same_bits(m["scaling_factor"], ref("scaling_factor"), prefix + " scaling_factor")
    if score.alignment == "least_squares_scale_shift":
        assert_close([m["least_squares_scale"], m["least_squares_shift"]], ref("lsq"), g["tol_lsq"], prefix + " scale, shift")
    ause = check_curves(curves[0], curves[1], ref("curves"), g, prefix)
    assert_close(ause, ref("ause"), g["tol_ause"], prefix + " ause")


@pytest.mark.parametrize("n_in,n_out", EC.RESIZE_PAIRS)
def test_index_table_is_scipy_order0_zoom(n_in, n_out):
    import scipy.ndimage as scipy_ndimage
    src = np.arange(n_in, dtype=np.float32)
    ref = scipy_ndimage.zoom(src, n_out / n_in, order=0, mode="mirror", grid_mode=True)
    idx = DS.resize_index(n_in, n_out)
    assert idx.dtype == np.int32 and idx.shape == (n_out,)
    assert np.array_equal(src[idx], ref)


@pytest.mark.parametrize("name", sorted(EC.SCORE_CASES))
def test_numpy_path_matches_reference(golden, name):
    g = golden("g18_eval")
    c = EC.score_case(name)
    clip = DS.normalize_clip(c["clip"])
    s = DS.score_numpy(c["gt"], c["pred"], c["unc"], c["alignment"], c["sparse_pred"], clip, maps=True)
    assert_same_bits(DS.rank_keys_numpy(s.rel_ae, c["gt"], s.pred_depth, c["sparse_pred"]), g[f"{name}/keys_oracle"], "oracle keys")
    assert_same_bits(DS.rank_keys_numpy(s.uncertainty, c["gt"], s.pred_depth, c["sparse_pred"]), g[f"{name}/keys_pred"], "pred keys")
    check_score(s, DS.uncertainty_curves_numpy(c["gt"], s, c["sparse_pred"]), g, name)
    if EC.SCORE_CASES[name].get("empty"):
        m = DS.metrics(s)
        assert all(np.isnan(m[k]) for k in ("absrel", "inliers103")) and s.n_mask == 0
    # explicit alignment parameters give what the computed ones give
    if c["alignment"] is not None:
        p = (s.ratio,) if c["alignment"] == "median" else (s.scale, s.shift)
        s2 = DS.score_numpy(c["gt"], c["pred"], c["unc"], c["alignment"], c["sparse_pred"], clip, maps=True, params=p)
        assert_same_bits(s2.pred_depth, s.pred_depth, "explicit parameters")


@pytest.mark.parametrize("kind,count", EC.MEDIAN_CASES)
def test_numpy_medians(golden, kind, count):
    g = golden("g18_eval")
    gt, pred = EC.median_case(kind, count)
    s = DS.score_numpy(gt, pred, None, "median", False, None)
    assert_same_bits(s.median_gt, g[f"median_{kind}_{count}/gt"], "median gt")
    assert_same_bits(s.median_pred, g[f"median_{kind}_{count}/pred"], "median pred")
    assert_same_bits(s.ratio, g[f"median_{kind}_{count}/scaling_factor"], "scaling factor")


LARGE = {"median": ("median", True, True), "lsq": ("least_squares_scale_shift", True, (0.5, 20.0)), "none": (None, False, False)}


@pytest.mark.parametrize("tag", sorted(LARGE))
def test_numpy_path_large_case(golden, tag):
    g = golden("g18_eval_large")
    c = EC.large_case()
    alignment, sparse, clip = LARGE[tag]
    s = DS.score_numpy(c["gt"], c["pred"], c["unc"], alignment, sparse, DS.normalize_clip(clip), maps=True)
    check_score(s, DS.uncertainty_curves_numpy(c["gt"], s, sparse), g, tag, maps=False)


# ---- the whole evaluation ----

def frame_matches(results, curves, g, cfg):
    cols = [tuple(c.split("|")) for c in g[f"{cfg}/columns"]]
    cols = [(c[0] if c[0] == "best" else int(c[0]), c[1]) for c in cols]
    have = [c for c in results.columns if c[1] not in EC.TIMING_COLUMNS]
    assert sorted(map(str, have)) == sorted(map(str, cols))
    assert list(results.index) == list(g[f"{cfg}/index"])
    exact = ("inliers103", "pred_depth_density", "scaling_factor", "num_views")
    tol = {"absrel": "tol_absrel", "ause": "tol_ause", "least_squares_scale": "tol_lsq", "least_squares_shift": "tol_lsq"}
    for j, c in enumerate(cols):
        ours = results[c].to_numpy(np.float64)
        ref = g[f"{cfg}/values"][:, j]
        if c[1] in exact:
            assert np.array_equal(ours, ref, equal_nan=True), c
        else:
            assert_close(ours, ref, g[tol[c[1]]], str(c))
    if curves is not None:
        assert [f"{i}|{c}" for i, c in curves.index] == list(g[f"{cfg}/curve_index"])
        ours = curves.to_numpy(np.float64)
        ref = g[f"{cfg}/curves"]
        for r in range(0, len(ref), 3):
            check_curves(ours[r], ours[r + 1], ref[r:r + 3], g, f"{cfg} curves {r}")
            assert np.allclose(ours[r + 2], ours[r + 1] - ours[r], equal_nan=True)


class KeepCurves:
    """the evaluation clears its curves frame when it returns: keep it"""

    def __init__(self, ev):
        self.ev, self.curves = ev, None
        inner = ev._output_results

        def wrapped():
            self.curves = ev.sparsification_curves
            inner()
        ev._output_results = wrapped


@pytest.mark.parametrize("cfg", sorted(EC.EVAL_CONFIGS))
def test_whole_evaluation_on_the_numpy_path(golden, cfg):
    import robustmvd_amd as R
    g = golden("g18_eval_class")
    samples, table = EC.lookup_dataset()
    ev = R.create_evaluation("mvd", out_dir=None, verbose=False, **EC.EVAL_CONFIGS[cfg])
    assert isinstance(ev, R.MultiViewDepthEvaluation)
    keep = KeepCurves(ev)
    model = EC.LookupModel(table)
    results = ev(dataset=samples, model=model, burn_in_samples=0)
    assert model.calls == int(g[f"{cfg}/model_calls"])
    assert results.columns.names == ["num_views", "metric"] and results.index.name == "sample_idx"
    frame_matches(results, keep.curves, g, cfg)
    if cfg == "single_view":  # max_source_views=0: one run without source views, no ordering runs
        assert model.calls == len(samples) and set(results.columns.get_level_values(0)) == {0, "best"}
    if cfg == "quasi_none":
        assert list(results[("best", "num_views")]) == [2, 2]  # not the run with most views
    for k in ("gpu_mem_alloc_in_mib", "gpu_mem_reserved_in_mib", "runtime_model_in_msec"):
        assert ("best", k) in results.columns


def test_view_ordering(golden):
    import robustmvd_amd as R
    from robustmvd_amd.utils import numpy_collate
    g = golden("g18_eval_class")
    samples, table = EC.lookup_dataset()
    for cfg in ("quasi_none", "nearest_lsq"):
        ev = R.create_evaluation("mvd", verbose=False, **EC.EVAL_CONFIGS[cfg])
        ev.model, ev.burn_in_samples = EC.LookupModel(table), 0
        for s, sample in enumerate(samples):
            batched = numpy_collate([sample])
            inputs = {k: v for k, v in batched.items() if k in ev.inputs or k == "keyview_idx"}
            order = ev._source_view_ordering(inputs, np.ascontiguousarray(batched["depth"][0, 0]))
            assert order == list(g[f"{cfg}/order"][s]), (cfg, s)
    assert list(g["quasi_none/order"][0]) != list(g["nearest_lsq/order"][0])


def test_result_files_and_skip_if_present(tmp_path):
    import pandas as pd
    import robustmvd_amd as R
    samples, table = EC.lookup_dataset()
    out = str(tmp_path / "eval")
    cfg = EC.EVAL_CONFIGS["quasi_median"]
    model = EC.LookupModel(table)
    results = R.create_evaluation("mvd", out_dir=out, verbose=False, **cfg)(dataset=samples, model=model, qualitatives=-1,
                                                                            burn_in_samples=0)
    for stem in ("results", "num_source_view_results", "sparsification_curves"):
        for ext in (".csv", ".pickle"):
            assert os.path.exists(os.path.join(out, stem + ext)), stem + ext
            assert os.path.exists(os.path.join(out, "per_sample", stem + ext)), "per_sample/" + stem + ext
    assert os.path.exists(os.path.join(out, ".results_df.pickle"))
    mean_curves = pd.read_pickle(os.path.join(out, "sparsification_curves.pickle"))
    assert list(mean_curves.index) == ["error", "oracle", "pred"] and mean_curves.shape == (3, 100)
    per_sample = pd.read_pickle(os.path.join(out, "per_sample", "sparsification_curves.pickle"))
    assert np.allclose(mean_curves.loc["pred"].to_numpy(float),
                       per_sample.xs("pred", level=1).astype(float).mean().to_numpy(float))
    assert pd.read_pickle(os.path.join(out, "results.pickle")).equals(results["best"].mean())
    for name in ("pointwise_absrel", "pred_depth", "pred_invdepth", "pred_depth_uncertainty"):
        m = np.load(os.path.join(out, "qualitative", f"{1:07d}-{name}.npy"))
        assert m.shape == (1,) + EC.GT_SHAPE and m.dtype == np.float32
    calls = model.calls
    again = R.create_evaluation("mvd", out_dir=out, verbose=False, **cfg)(dataset=samples, model=model)
    assert model.calls == calls, "the second call ran the model"
    assert again.equals(results)


def test_create_and_list_evaluations():
    import robustmvd_amd as R
    assert "mvd" in R.list_evaluations()
    ev = R.create_evaluation("mvd", verbose=False, max_source_views=0, min_source_views=1)
    assert ev.min_source_views == 0 and ev.view_ordering is None and ev.inputs == ["images"]
    with pytest.raises(ValueError):
        R.create_evaluation("nope")
    with pytest.raises(ValueError):
        R.create_evaluation("mvd", alignment="translation", verbose=False)
    for difference in ("Dataset", "Where scoring runs", "Host path", "Memory columns", "Output files", "groupby(level=1)",
                       "gpu_mem_reserved_in_mib", "output_adapter", "synchronised"):
        assert difference in R.eval.__doc__, difference


def test_new_entries_reject_bad_arguments_without_gpu():
    from robustmvd_amd import _lib
    lib = _lib.load()
    assert lib.mvd_depth_eval_workspace_bytes(0, 5) == 0
    assert lib.mvd_depth_eval_workspace_bytes(768, 1152) >= 432 * 8
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)  # never dereferenced: every call below is refused first
    bad = _lib.load().mvd_depth_align_stats_f32
    assert bad(null, one, null, one, one, 4, 4, 4, 4, 1, 0, one, null, one, 1 << 20, null) != 0
    assert b"NULL" in lib.mvd_last_error()
    assert bad(one, one, null, one, one, 0, 4, 4, 4, 1, 0, one, null, one, 1 << 20, null) != 0
    assert b"dimension" in lib.mvd_last_error()
    assert bad(one, one, null, one, one, 4, 4, 4, 4, 7, 0, one, null, one, 1 << 20, null) != 0
    assert bad(one, one, null, one, one, 64, 64, 4, 4, 1, 0, one, null, one, 16, null) != 0
    assert b"workspace" in lib.mvd_last_error()
    score = lib.mvd_depth_score_f32
    args = lambda gt, H, mode, params, result: (gt, one, null, one, one, H, 4, 4, 4, mode, 0, 1, 0.1, 100.0, 1.03, 2.03, params, result,
                                                null, null, null, null, one, 1 << 20, null)
    assert score(*args(null, 4, 0, null, one)) != 0
    assert score(*args(one, -1, 0, null, one)) != 0
    assert score(*args(one, 4, 1, null, one)) != 0  # an alignment without parameters
    assert score(*args(one, 4, 0, null, null)) != 0
    assert lib.mvd_rank_keys_f32(one, one, one, one, 0, 0, one, null) != 0
    assert lib.mvd_rank_keys_f32(one, null, one, one, 0, 16, one, null) != 0
    assert lib.mvd_ranked_step_sums_f64(one, 16, null, one, one, 1 << 20, null) != 0
    assert lib.mvd_ranked_step_sums_f64(one, 0, one, one, one, 1 << 20, null) != 0
    assert lib.mvd_ranked_step_sums_f64(one, 16, one, one, one, 8, null) != 0
