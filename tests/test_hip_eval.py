"""GPU checks of the depth-evaluation kernels (csrc/depth_eval.hip) and of the evaluation that runs on them, against the reference's
results in tests/golden/g18_eval*.npz (tests/golden/make_golden_eval.py).

Match levels: index tables, per-pixel maps, ranking keys, counts (hence inliers103 and pred_depth_density), both medians (hence
scaling_factor), the view ordering and num_views equal the reference's bit for bit.  absrel, the curves, the AUSE and the
least-squares scale and shift come from sums, float64 on the device and float32 pairwise in the reference; their relative tolerances
are the fixture's tol_*: twice the largest gap between the reference's float32 value and the same formula with float64 sums (ranking
ties broken in another order) over all cases, at least 4 float32 ulps.  As generated:
    tol_absrel 4.768e-07 (largest gap 9.664e-08)     tol_curve 5.126e-07 (largest gap 2.563e-07)
    tol_ause   4.768e-07 (largest gap 1.517e-07)     tol_lsq   4.768e-07 (largest gap 4.915e-08)
"""
import numpy as np
import pytest
import torch

import eval_cases as EC
import gen_common as gc
from robustmvd_amd import depth_score as DS
from test_eval_cpu import LARGE, KeepCurves, assert_close, assert_same_bits, check_score, frame_matches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host_maps(s):
    for k in ("pred_depth", "pred_invdepth", "rel_ae", "uncertainty"):
        v = getattr(s, k)
        setattr(s, k, v.cpu().numpy() if v is not None else None)
    return s


def device_score(c, alignment, sparse, clip, params=None):
    scorer = DS.DeviceScorer(c["gt"], DEV, alignment, sparse, DS.normalize_clip(clip))
    s = scorer.score(up(c["pred"]), up(c["unc"]), maps=True, params=params)
    keys = [scorer.rank_keys(u, m, s.pred_depth).cpu().numpy().reshape(c["gt"].shape)
            for u, m in ((s.rel_ae, s.extra["device_out"].view(torch.float32)[8:9]),
                         (s.uncertainty, s.extra["device_out"].view(torch.float32)[15:16]))]
    curves = scorer.uncertainty_curves(s)
    return scorer, host_maps(s), keys, curves


@pytest.mark.parametrize("name", sorted(EC.SCORE_CASES))
def test_kernels_match_reference(golden, name):
    g = golden("g18_eval")
    c = EC.score_case(name)
    scorer, s, keys, curves = device_score(c, c["alignment"], c["sparse_pred"], c["clip"])
    row, col = scorer.tables(*c["pred"].shape)
    assert np.array_equal(row.cpu().numpy(), DS.resize_index(c["pred"].shape[0], EC.GT_SHAPE[0]))
    assert np.array_equal(col.cpu().numpy(), DS.resize_index(c["pred"].shape[1], EC.GT_SHAPE[1]))
    assert_same_bits(keys[0], g[f"{name}/keys_oracle"], "oracle keys")
    assert_same_bits(keys[1], g[f"{name}/keys_pred"], "pred keys")
    check_score(s, curves, g, name)
    ref = DS.score_numpy(c["gt"], c["pred"], c["unc"], c["alignment"], c["sparse_pred"], DS.normalize_clip(c["clip"]))
    assert (s.n_mask, s.n_inliers, s.n_eval) == (ref.n_mask, ref.n_inliers, ref.n_eval)
    assert_same_bits(s.min_rel_ae, ref.min_rel_ae, "min rel_ae")
    assert_same_bits(s.uncertainty_min, ref.uncertainty_min, "min uncertainty")


@pytest.mark.parametrize("kind,count", EC.MEDIAN_CASES)
def test_radix_select_medians(golden, kind, count):
    g = golden("g18_eval")
    gt, pred = EC.median_case(kind, count)
    s = DS.DeviceScorer(gt, DEV, "median", False, None).score(up(pred))
    assert s.n_mask == count
    assert_same_bits(s.median_gt, g[f"median_{kind}_{count}/gt"], "median gt")
    assert_same_bits(s.median_pred, g[f"median_{kind}_{count}/pred"], "median pred")
    assert_same_bits(s.ratio, g[f"median_{kind}_{count}/scaling_factor"], "scaling factor")


@pytest.mark.parametrize("tag", sorted(LARGE))
def test_large_case_several_workgroups(golden, tag):
    g = golden("g18_eval_large")
    c = EC.large_case()
    assert -(-c["gt"].size // 2048) > 1 and c["gt"].size % 2048 != 0  # several workgroups, a partial last one
    alignment, sparse, clip = LARGE[tag]
    _, s, keys, curves = device_score(c, alignment, sparse, clip)
    check_score(s, curves, g, tag, maps=False)
    ref = DS.score_numpy(c["gt"], c["pred"], c["unc"], alignment, sparse, DS.normalize_clip(clip), maps=True)
    for k in ("pred_depth", "pred_invdepth", "rel_ae", "uncertainty"):  # the numpy path's maps, which the small cases pin
        assert_same_bits(getattr(s, k), getattr(ref, k), f"{tag} {k}")
    assert_same_bits(keys[0], DS.rank_keys_numpy(ref.rel_ae, c["gt"], ref.pred_depth, sparse), "oracle keys")
    assert_same_bits(keys[1], DS.rank_keys_numpy(ref.uncertainty, c["gt"], ref.pred_depth, sparse), "pred keys")
    assert (s.n_mask, s.n_inliers, s.n_eval) == (ref.n_mask, ref.n_inliers, ref.n_eval)
    if alignment == "least_squares_scale_shift":
        scorer = DS.DeviceScorer(c["gt"], DEV, alignment, sparse, None)
        _, sums = scorer.align_stats(up(c["pred"]))
        # two summation orders of n positive float64 terms differ by at most 2 n 2^-53 relative
        assert_close(sums.cpu().numpy(), ref.extra["sums"], 2 * c["gt"].size * 2.0 ** -53, "the five float64 sums")


@pytest.mark.parametrize("tag", sorted(LARGE))
def test_two_calls_give_the_same_bits(tag):
    c = EC.large_case()
    alignment, sparse, clip = LARGE[tag]
    scorer = DS.DeviceScorer(c["gt"], DEV, alignment, sparse, DS.normalize_clip(clip))
    pred, unc = up(c["pred"]), up(c["unc"])
    outs = []
    for _ in range(2):
        params, sums = scorer.align_stats(pred, unc)
        s = scorer.score(pred, unc, maps=True)
        raw = s.extra["device_out"].cpu().numpy().copy()
        keys = scorer.rank_keys(s.uncertainty, params[5:6], s.pred_depth)
        ranked = s.rel_ae.reshape(-1)[torch.sort(keys, descending=True, stable=True).indices]
        steps = scorer.ranked_step_sums(ranked, s.extra["device_out"][1:2])
        outs.append([params.cpu().numpy().view(np.uint32), sums.cpu().numpy().view(np.uint64), raw, keys.cpu().numpy().view(np.uint32),
                     steps.cpu().numpy().view(np.uint64), s.rel_ae.cpu().numpy().view(np.uint32)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["d_med_enl_sparse", "h_lsq_red_sparse"])
def test_parameters_from_the_device_buffer_or_explicit(name):
    c = EC.score_case(name)
    scorer = DS.DeviceScorer(c["gt"], DEV, c["alignment"], c["sparse_pred"], DS.normalize_clip(c["clip"]))
    pred = up(c["pred"])
    a = scorer.score(pred, maps=True)
    params, _ = scorer.align_stats(pred)
    host = params.cpu().numpy()
    b = scorer.score(pred, maps=True, params=params)                    # the device buffer handed over
    e = scorer.score(pred, maps=True, params=(host[0], host[1]))        # the same numbers from the host
    for other in (b, e):
        assert np.array_equal(a.extra["device_out"][:4].cpu().numpy(), other.extra["device_out"][:4].cpu().numpy())
        assert torch.equal(a.pred_depth.view(torch.int32), other.pred_depth.view(torch.int32))
        assert torch.equal(a.rel_ae.view(torch.int32), other.rel_ae.view(torch.int32))


@pytest.mark.parametrize("cfg", sorted(EC.EVAL_CONFIGS))
def test_whole_evaluation_on_the_device(golden, cfg):
    import robustmvd_amd as R
    g = golden("g18_eval_class")
    samples, table = EC.lookup_dataset()
    ev = R.create_evaluation("mvd", out_dir=None, verbose=False, **EC.EVAL_CONFIGS[cfg])
    keep = KeepCurves(ev)
    scorers = []
    make = DS.DeviceScorer

    class Counting(make):
        def __init__(self, *a, **k):
            scorers.append(self)
            super().__init__(*a, **k)
    DS.DeviceScorer = Counting
    try:
        model = EC.LookupModel(table, to=up)
        results = ev(dataset=samples, model=model, burn_in_samples=0)
    finally:
        DS.DeviceScorer = make
    assert len(scorers) == len(samples), "the ground truth is uploaded once per sample"
    assert model.calls == int(g[f"{cfg}/model_calls"])
    frame_matches(results, keep.curves, g, cfg)
    assert np.isfinite(results[("best", "gpu_mem_alloc_in_mib")]).all() and np.isfinite(results[("best", "gpu_mem_reserved_in_mib")]).all()


def test_robust_mvd_device_scoring_equals_host_scoring(golden):
    import robustmvd_amd as R
    tol = golden("g18_eval")
    model = R.RobustMVD().eval()
    weights = gc.robustmvd_weights({k: tuple(v.shape) for k, v in model.state_dict().items()}, 2)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    model = model.to(DEV)
    s = gc.synthetic_sample(1, 64, 128, 2)
    rng = np.random.default_rng(5)
    gt = (EC.surface((45, 101)) * (1 + 0.05 * rng.standard_normal((45, 101)))).astype(np.float32)
    gt[rng.random(gt.shape) < 0.2] = 0.0
    sample = dict(images=s["images"], poses=s["poses"], intrinsics=s["intrinsics"], keyview_idx=0, depth=gt[None],
                  invdepth=np.where(gt > 0, 1 / np.where(gt > 0, gt, 1), 0).astype(np.float32)[None])
    frames, curves = [], []
    for device_scoring in (True, False):
        ev = R.create_evaluation("mvd", verbose=False, inputs=["poses", "intrinsics"], alignment="median",
                                 device_scoring=device_scoring)
        keep = KeepCurves(ev)
        frames.append(ev(dataset=[sample], model=model, burn_in_samples=0))
        curves.append(keep.curves.to_numpy(np.float64))
    dev, host = frames
    assert list(dev.columns) == list(host.columns)
    assert np.isfinite(dev[("best", "absrel")]).all()
    sums = {"absrel": "tol_absrel", "ause": "tol_ause"}
    for c in dev.columns:
        if c[1] in EC.TIMING_COLUMNS:
            continue
        a, b = dev[c].to_numpy(np.float64), host[c].to_numpy(np.float64)
        if c[1] in sums:
            assert_close(a, b, tol[sums[c[1]]], str(c))
        else:
            assert np.array_equal(a, b, equal_nan=True), c
    assert_close(curves[0][:2], curves[1][:2], tol["tol_curve"], "curves")
