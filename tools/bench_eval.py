#!/usr/bin/env python3
"""Times the scoring of the multi-view depth evaluation and writes profiles/depth_eval.txt (commit and device name in the header).

At a 768 x 1152 ground truth, with the prediction and uncertainty that robust_mvd itself gives for a 768 x 1152 frame with 4 source
views (random weights; its frame time is measured in the same process and printed next to the rest):
  (a) one run's scoring on the device (DeviceScorer.score: alignment statistics, the scoring pass, the 72-byte read), for each
      alignment, as host wall time per call with the read included (the call ends synchronised);
  (b) one sample's AUSE on the device (the scoring pass with its four maps, two rankings: keys, torch.sort, gather, step sums, and
      the read of the 200 sums);
  (c) the numpy path of (a) and (b) on the same box, from numpy arrays already on the host.
A figure is the median over --repeats calls after --warmup calls."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_common as gc  # noqa: E402
import robustmvd_amd as R  # noqa: E402
from robustmvd_amd import depth_score as DS  # noqa: E402
from bench_vis_mvsnet import event_ms, tree_label  # noqa: E402


def wall_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1000 * (time.perf_counter() - t0))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--numpy-repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_eval.txt"))
    ap.add_argument("--commit", default=None, help="commit to name in the header (default: the checkout's)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W, V = 768, 1152, 4
    out = [f"depth evaluation scoring on {torch.cuda.get_device_name(0)}; commit {args.commit or tree_label()}; tools/bench_eval.py "
           f"--warmup {args.warmup} --repeats {args.repeats} --numpy-repeats {args.numpy_repeats}", ""]

    torch.manual_seed(0)
    model = R.RobustMVD().eval().to(dev)
    s = gc.synthetic_sample(1, H, W, V)
    sample = model.input_adapter(images=[im[None] for im in s["images"]], keyview_idx=np.array([0]), poses=[p[None] for p in s["poses"]],
                                 intrinsics=[k[None] for k in s["intrinsics"]])
    with torch.no_grad():
        frame = event_ms(lambda: model(**sample), args.warmup, args.repeats)
        pred, _ = model(**sample)
    depth, unc = pred["depth"][0, 0].clone(), pred["depth_uncertainty"][0, 0].clone()
    # a prediction worth scoring: random weights give a flat map, so the model's output only sets the size
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    gt = (2.0 + np.sin(xx / 90.0) * np.cos(yy / 70.0) + yy / 400.0).astype(np.float32)
    gt[rng.random(gt.shape) < 0.2] = 0.0
    h, w = depth.shape
    row, col = DS.resize_tables(H, W, h, w)
    small = gt[row][:, col]
    depth_np = (np.where(small > 0, small, 3.0) * (1 + 0.05 * rng.standard_normal((h, w)))).astype(np.float32)
    unc_np = np.abs(rng.standard_normal((h, w))).astype(np.float32)
    depth.copy_(torch.from_numpy(depth_np))
    unc.copy_(torch.from_numpy(unc_np))
    out.append(f"robust_mvd, {H} x {W}, {V} source views: {frame[0]:.3f} ms per frame (median of {args.repeats}; min {frame[1]:.3f}, "
               f"max {frame[2]:.3f}); its prediction is {h} x {w}, the ground truth {H} x {W}")
    out.append("")

    for alignment in DS.ALIGNMENTS:
        scorer = DS.DeviceScorer(gt, dev, alignment, False, (0.1, 100.0))
        a = scorer.score(depth, unc)
        b = DS.score_numpy(gt, depth_np, unc_np, alignment, False, (0.1, 100.0))
        assert (a.n_mask, a.n_inliers, a.n_eval) == (b.n_mask, b.n_inliers, b.n_eval), "device and numpy paths disagree"
        d = wall_ms(lambda: scorer.score(depth, unc), args.warmup, args.repeats)
        n = wall_ms(lambda: DS.score_numpy(gt, depth_np, unc_np, alignment, False, (0.1, 100.0)), 1, args.numpy_repeats)
        out.append(f"(a) one run's scoring, alignment {str(alignment):<26s}: device {d[0]:7.3f} ms (min {d[1]:.3f}, max {d[2]:.3f})   "
                   f"(c) numpy {n[0]:8.2f} ms   ({n[0] / d[0]:.0f}x; device = {d[0] / frame[0]:.2f} model frames)")

    scorer = DS.DeviceScorer(gt, dev, None, False, (0.1, 100.0))

    def device_ause():
        return scorer.uncertainty_curves(scorer.score(depth, unc, maps=True))

    def numpy_ause():
        return DS.uncertainty_curves_numpy(gt, DS.score_numpy(gt, depth_np, unc_np, None, False, (0.1, 100.0), maps=True), False)

    ca, cb = device_ause(), numpy_ause()
    assert np.allclose(ca[1], cb[1], rtol=1e-9, equal_nan=True), "device and numpy curves disagree"
    d = wall_ms(device_ause, args.warmup, args.repeats)
    n = wall_ms(numpy_ause, 1, args.numpy_repeats)
    out.append(f"(b) one sample's AUSE (maps, two rankings, curves)        : device {d[0]:7.3f} ms (min {d[1]:.3f}, max {d[2]:.3f})   "
               f"(c) numpy {n[0]:8.2f} ms   ({n[0] / d[0]:.0f}x; device = {d[0] / frame[0]:.2f} model frames)")
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
