#!/usr/bin/env python3
"""Times the point-cloud evaluation and writes profiles/cloud_eval.txt (commit and device name in the header).

Two workloads, in one process on one GPU:
  fused      the fused cloud of one 768 x 1152 key view with 4 sources (tools/bench_depth_fusion.py's scene, fused by the kernels)
             as the prediction, against a voxel-thinned copy of itself (voxel 0.006) with N(0, 0.003) noise as the ground truth;
             thresholds (0.005, 0.01), max_dist 0.04: some fifty points per cell
  clustered  200,000 + 200,000 points from one Gaussian blob of sigma = max_dist = 0.04: up to ten thousand points per cell, the
             case in which the grid prunes little and the scan itself is timed
For each:
  (a) the sort (mvd_cloud_cell_keys_f32, torch.sort, mvd_cloud_grid_build_f32) of each cloud, the nearest kernel per direction, the
      scores kernel of one direction, mvd_voxel_reduce_f32 on the prediction's sorted voxel keys and the whole PointCloudEvaluation
      call (with its host reads), each as the median over --repeats HIP-event brackets of --inner calls after --warmup brackets;
  (b) the same definition as chunked torch.cdist(compute_mode="donot_use_mm_for_euclid_dist").min(dim=1) on the same GPU, chunks of
      2^28 distances, one timed pass per direction after one warm-up chunk; the largest difference between its distances and the
      kernel's is printed;
  (c) scipy.spatial.cKDTree (build + query with distance_upper_bound) on the same machine's CPU, in a child process that imports no
      GPU library, while this process leaves the GPU idle; with 1 worker and with 16.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DIST, THRESHOLDS = 0.04, (0.005, 0.01)


def kdtree_child(path):
    """The CPU comparison: both directions of one workload, no GPU library imported."""
    from scipy.spatial import cKDTree
    data = np.load(path)
    pred, gt = data["pred"].astype(np.float64), data["gt"].astype(np.float64)
    out = {}
    for workers in (1, 16):
        t0 = time.perf_counter()
        for q, p in ((pred, gt), (gt, pred)):
            d, _ = cKDTree(p).query(q, distance_upper_bound=MAX_DIST, workers=workers)
        out[f"workers{workers}_ms"] = 1000 * (time.perf_counter() - t0)
    out["mean_gt_to_pred"] = float(np.minimum(d, np.float64(np.float32(MAX_DIST))).mean())
    print(json.dumps(out))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--kdtree-child":
        return kdtree_child(sys.argv[2])
    import torch
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from robustmvd_amd import cloud_eval as CE
    from robustmvd_amd import depth_fusion as DF
    from robustmvd_amd import _lib as L
    from robustmvd_amd import ops
    from bench_depth_fusion import bench_scene
    from bench_vis_mvsnet import event_ms, tree_label

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3, help="calls per HIP-event bracket")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_eval.txt"))
    ap.add_argument("--commit", default=None, help="commit to name in the header (default: the checkout's)")
    ap.add_argument("--small", action="store_true", help="a rehearsal at a toy size: no figure of it means anything")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(0)

    H, W, V = (96, 144, 4) if args.small else (768, 1152, 4)
    K, Ts, depths, image = bench_scene(H, W, V)
    mats = up(DF.compose_matrices(K, Ts[0], [K] * V, Ts[1:]).astype(np.float32))
    bp = up(DF.compose_backprojection(K, Ts[0]).astype(np.float32))
    maps = [up(d) for d in depths]
    _, fused, mask, _ = ops.geo_consistency(maps[0], maps[1:], mats)
    xyz, _, count = ops.compact_points(mask, fused, bp)
    pred = xyz[:int(count.item())].clone()
    thin, _, _ = ops.voxel_downsample(pred, 0.006 * 768 / H)
    gt = (thin + up(rng.normal(0, 0.003, tuple(thin.shape)).astype(np.float32))).contiguous()
    n_blob = 2000 if args.small else 200000
    blob = lambda: up(rng.normal(0, MAX_DIST, (n_blob, 3)).astype(np.float32))
    workloads = [("fused", pred, gt), ("clustered", blob(), blob())]

    out = [f"point-cloud evaluation on {torch.cuda.get_device_name(0)}; commit {args.commit or tree_label()}; tools/bench_cloud_eval.py "
           f"--warmup {args.warmup} --repeats {args.repeats} --inner {args.inner}" + (" --small (REHEARSAL: not a measurement)" if args.small else ""),
           f"max_dist {MAX_DIST}, thresholds {THRESHOLDS}; ms = median (min, max) per call over HIP-event brackets", ""]
    md = float(np.float32(MAX_DIST))
    cell = md * ops.CLOUD_CELL_MARGIN
    for name, a, b in workloads:
        n, m = len(a), len(b)
        origin = torch.minimum(a.amin(0), b.amin(0)).double().cpu().tolist()
        ga, gb = ops.cloud_grid(a, origin, cell), ops.cloud_grid(b, origin, cell)
        th = up(np.float32(THRESHOLDS))
        res = {}

        def nearest(q, t, key):
            res[key] = ops.cloud_nearest(q, t, md)

        nearest(ga, gb, "ab")
        nearest(gb, ga, "ba")
        sort_a = event_ms(lambda: ops.cloud_grid(a, origin, cell, check=False), args.warmup, args.repeats, args.inner)
        sort_b = event_ms(lambda: ops.cloud_grid(b, origin, cell, check=False), args.warmup, args.repeats, args.inner)
        k_ab = event_ms(lambda: nearest(ga, gb, "ab"), args.warmup, args.repeats, args.inner)
        k_ba = event_ms(lambda: nearest(gb, ga, "ba"), args.warmup, args.repeats, args.inner)
        sc = event_ms(lambda: ops.cloud_scores(res["ab"][0], res["ab"][1], th, a), args.warmup, args.repeats, args.inner)
        # the voxel thinning's own entry on keys sorted beforehand (ops.voxel_downsample's launches without its sort and its read)
        voxel = float(np.float32(0.006 * 768 / H))
        vkeys, vperm = ops.cloud_sorted(a, origin, 1.0 / voxel)
        vout = (torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty(1, dtype=torch.int64, device=dev))
        vbytes = int(L.load().mvd_voxel_reduce_workspace_bytes(n))
        vws = ops.workspace(vbytes, dev)
        vx = event_ms(lambda: ops.call("mvd_voxel_reduce_f32", dev, vkeys, vperm, a, None, n, vout[0], None, vout[1], vout[2], vws, vbytes),
                      args.warmup, args.repeats, args.inner)
        ev = CE.PointCloudEvaluation(THRESHOLDS, MAX_DIST)
        whole = event_ms(lambda: ev(a, b), args.warmup, args.repeats, 1)
        score = ev(a, b)

        # (b) the same definition from torch.cdist on differences, chunked
        def cdist_direction(q, t):
            step = max(1, (1 << 28) // max(len(t), 1))
            parts = [torch.cdist(q[i:i + step], t, compute_mode="donot_use_mm_for_euclid_dist").min(dim=1).values.clamp(max=md)
                     for i in range(0, len(q), step)]
            return torch.cat(parts)

        cdist_direction(a[:1024], b)
        torch.cuda.synchronize()
        c_ms, c_out = [], []
        for q, t in ((a, b), (b, a)):
            t0 = time.perf_counter()
            c_out.append(cdist_direction(q, t))
            torch.cuda.synchronize()
            c_ms.append(1000 * (time.perf_counter() - t0))
        worst = max(float((got - want).abs().max()) for got, want in ((res["ab"][0], c_out[0]), (res["ba"][0], c_out[1])))

        # (c) the k-d tree on the CPU, in a child that imports no GPU library; this process waits with the GPU idle
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "clouds.npz")
            np.savez(path, pred=a.cpu().numpy(), gt=b.cpu().numpy())
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--kdtree-child", path], capture_output=True, text=True,
                                   check=True)
        kd = json.loads(child.stdout.strip().splitlines()[-1])
        kd_gap = abs(kd["mean_gt_to_pred"] - float(res["ba"][0].double().mean()))

        per_cell = np.unique(gb.keys.cpu().numpy(), return_counts=True)[1]
        gpu_ms = k_ab[0] + k_ba[0] + sort_a[0] + sort_b[0]
        out += [f"{name}: {n} predicted and {m} ground-truth points; ground-truth cells hold median {int(np.median(per_cell))}, max "
                f"{int(per_cell.max())} points; accuracy {score.accuracy:.5f}, completeness {score.completeness:.5f}, F {np.round(score.fscore, 4).tolist()}",
                f"  sort (keys, torch.sort, records)   pred {sort_a[0]:8.3f} ms ({sort_a[1]:.3f}, {sort_a[2]:.3f})   gt {sort_b[0]:8.3f} ms ({sort_b[1]:.3f}, {sort_b[2]:.3f})",
                f"  nearest kernel   pred -> gt {k_ab[0]:9.3f} ms ({k_ab[1]:.3f}, {k_ab[2]:.3f})   gt -> pred {k_ba[0]:9.3f} ms ({k_ba[1]:.3f}, {k_ba[2]:.3f})",
                f"  scores kernels (one direction, {n} distances) {sc[0]:8.4f} ms ({sc[1]:.4f}, {sc[2]:.4f})",
                f"  voxel reduce kernels (the predicted cloud at voxel {voxel:.4g}, {int(vout[2].item())} voxels) {vx[0]:8.4f} ms ({vx[1]:.4f}, {vx[2]:.4f})",
                f"  whole PointCloudEvaluation call (extent reads, two sorts, two searches, two scores, one read) {whole[0]:9.3f} ms ({whole[1]:.3f}, {whole[2]:.3f})",
                f"  chunked torch.cdist(...).min on the same GPU   pred -> gt {c_ms[0]:10.1f} ms   gt -> pred {c_ms[1]:10.1f} ms   "
                f"= {c_ms[0] / k_ab[0]:.1f}x and {c_ms[1] / k_ba[0]:.1f}x the nearest kernel (one pass each; {n * m / 1e9:.1f} G distances per direction)",
                f"  scipy cKDTree on the CPU, both directions, build + query: {kd['workers1_ms']:.0f} ms with 1 worker, {kd['workers16_ms']:.0f} ms with 16   "
                f"= {kd['workers16_ms'] / gpu_ms:.0f}x the two sorts and two searches",
                f"  agreement: max |kernel - cdist| {worst:.2e} over both directions; |mean(gt -> pred) kernel - k-d tree| {kd_gap:.2e}", ""]
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
