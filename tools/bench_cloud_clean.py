#!/usr/bin/env python3
"""Times the point-cloud clean-up and writes profiles/cloud_clean.txt (commit and device name in the header).

Two clouds, each against itself, in one process on one GPU:
  fused      the fused cloud of one 768 x 1152 key view with 4 sources (tools/bench_cloud_eval.py's prediction); the radius is 3 x its
             cloud_spacing, some thirty neighbours per point
  clustered  200,000 points from one Gaussian blob of sigma = radius = 0.04: up to ten thousand points per cell, the case in which
             the grid prunes little and the scan itself is timed
For each:
  (a) mvd_cloud_nearest_f32 on the same grid (the yardstick: the new kernels stage the same records), the radius-moments kernel, the
      k-NN kernel at k = 8 and 16, the list moments, the normals kernel, the verdict + selection + gather of the density rule, and the
      whole estimate_normals / remove_outliers calls (with their sorts and host reads), each as the median over --repeats HIP-event
      brackets of --inner calls after --warmup brackets;
  (b) the density filter composed from torch on the same GPU: chunked torch.cdist(compute_mode="donot_use_mm_for_euclid_dist") < r,
      a row sum and boolean indexing, chunks of 2^23 distances (cdist launches a workgroup of 256 threads per distance, and a HIP
      launch holds fewer than 2^32 threads), one timed pass after one warm-up chunk; this pass is nearly all of the tool's five minutes;
  (c) scipy.spatial.cKDTree on the same machine's CPU with 16 workers (build, query_ball_point(return_length=True), query(k + 1)),
      where scipy is importable, in a child process that imports no GPU library, while this process leaves the GPU idle.
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
BLOB_RADIUS = 0.04


def kdtree_child(path):
    """The CPU comparison of one cloud, no GPU library imported."""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        print(json.dumps({}))
        return
    data = np.load(path)
    p, r = data["points"].astype(np.float64), float(data["radius"])
    out = {}
    t0 = time.perf_counter()
    tree = cKDTree(p)
    out["build_ms"] = 1000 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    counts = tree.query_ball_point(p, r, workers=16, return_length=True)
    out["ball_ms"] = 1000 * (time.perf_counter() - t0)
    out["mean_count"] = float(np.mean(counts) - 1)  # the point itself is in its ball
    for k in (8, 16):
        t0 = time.perf_counter()
        tree.query(p, k=k + 1, distance_upper_bound=r, workers=16)
        out[f"knn{k}_ms"] = 1000 * (time.perf_counter() - t0)
    print(json.dumps(out))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--kdtree-child":
        return kdtree_child(sys.argv[2])
    import torch
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from robustmvd_amd import cloud_clean as CL
    from robustmvd_amd import depth_fusion as DF
    from robustmvd_amd import ops
    from bench_depth_fusion import bench_scene
    from bench_vis_mvsnet import event_ms, tree_label

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=2, help="calls per HIP-event bracket")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_clean.txt"))
    ap.add_argument("--commit", default=None, help="commit to name in the header (default: the checkout's)")
    ap.add_argument("--small", action="store_true", help="a rehearsal at a toy size: no figure of it means anything")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(0)
    ms = lambda fn, inner=args.inner: event_ms(fn, args.warmup, args.repeats, inner)
    fmt = lambda t: f"{t[0]:9.3f} ms ({t[1]:.3f}, {t[2]:.3f})"

    H, W, V = (96, 144, 4) if args.small else (768, 1152, 4)
    K, Ts, depths, _ = bench_scene(H, W, V)
    mats = up(DF.compose_matrices(K, Ts[0], [K] * V, Ts[1:]).astype(np.float32))
    bp = up(DF.compose_backprojection(K, Ts[0]).astype(np.float32))
    maps = [up(d) for d in depths]
    _, fused, mask, _ = ops.geo_consistency(maps[0], maps[1:], mats)
    xyz, _, count = ops.compact_points(mask, fused, bp)
    pred = xyz[:int(count.item())].clone()
    spacing = CL.cloud_spacing(pred, BLOB_RADIUS)
    n_blob = 2000 if args.small else 200000
    workloads = [("fused", pred, float(np.float32(3.0 * spacing))),
                 ("clustered", up(rng.normal(0, BLOB_RADIUS, (n_blob, 3)).astype(np.float32)), float(np.float32(BLOB_RADIUS)))]

    out = [f"point-cloud clean-up on {torch.cuda.get_device_name(0)}; commit {args.commit or tree_label()}; tools/bench_cloud_clean.py "
           f"--warmup {args.warmup} --repeats {args.repeats} --inner {args.inner}" + (" --small (REHEARSAL: not a measurement)" if args.small else ""),
           "every cloud against itself; ms = median (min, max) per call over HIP-event brackets; x = multiples of the nearest kernel on the "
           "same grid", ""]
    for name, a, r in workloads:
        n = len(a)
        grid = CL._device_grid(a, r, "points")
        res = {}
        nearest = ms(lambda: ops.cloud_nearest(grid, grid, r))
        sort = ms(lambda: ops.cloud_grid(a, grid.origin, grid.cell, check=False))
        radius = ms(lambda: res.__setitem__("nb", ops.cloud_radius_moments(None, grid, r)))
        knn = {k: ms(lambda k=k: res.__setitem__(k, ops.cloud_knn(None, grid, k, r))) for k in (8, 16)}
        lists = ms(lambda: ops.cloud_list_moments(a, a, res[16][0], res[16][1]))
        cnt, _, mom = res["nb"]
        normals = ms(lambda: ops.cloud_normals(a, cnt, mom, 5))
        min_nb = max(2, int(cnt.float().median().item()) // 2)

        def select():
            kept, remap, kk = ops.cloud_select(ops.cloud_keep_density(a, cnt, min_nb))
            return ops.mesh_gather_rows(a, remap, kk)

        selection = ms(select, 1)
        whole_normals = ms(lambda: CL.estimate_normals(a, radius=r), 1)
        whole_normals_k = ms(lambda: CL.estimate_normals(a, k=16, max_dist=r), 1)
        whole_density = ms(lambda: CL.remove_outliers(a, radius=r, min_neighbours=min_nb), 1)
        whole_stat = ms(lambda: CL.remove_outliers(a, k=8, std_ratio=2.0, max_dist=r), 1)
        kept_density = CL.remove_outliers(a, radius=r, min_neighbours=min_nb)
        kept_stat = CL.remove_outliers(a, k=8, std_ratio=2.0, max_dist=r)

        # (b) the density filter composed from torch, chunked
        def torch_filter():
            step = max(1, (1 << 23) // n)
            counts = torch.cat([(torch.cdist(a[i:i + step], a, compute_mode="donot_use_mm_for_euclid_dist") < r).sum(dim=1)
                                for i in range(0, n, step)]) - 1  # the point itself
            return counts, a[counts >= min_nb]

        (torch.cdist(a[:8], a, compute_mode="donot_use_mm_for_euclid_dist") < r).sum(dim=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t_counts, t_kept = torch_filter()
        torch.cuda.synchronize()
        torch_ms = 1000 * (time.perf_counter() - t0)
        differ = int((t_counts != cnt).sum().item())

        # (c) the k-d tree on the CPU, in a child that imports no GPU library; this process waits with the GPU idle
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "cloud.npz")
            np.savez(path, points=a.cpu().numpy(), radius=np.float64(r))
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--kdtree-child", path], capture_output=True, text=True,
                                   check=True)
        kd = json.loads(child.stdout.strip().splitlines()[-1])

        per_cell = np.unique(grid.keys.cpu().numpy(), return_counts=True)[1]
        c = cnt.cpu().numpy()
        x = lambda t: f"{t[0] / nearest[0]:6.1f}x"
        out += [f"{name}: {n} points, radius {r:.5f}" + (f" = 3 x the spacing {spacing:.5f}" if name == "fused" else "") +
                f"; cells hold median {int(np.median(per_cell))}, max {int(per_cell.max())} points; neighbours within the radius: median "
                f"{int(np.median(c))}, max {int(c.max())}; full lists at k = 8: {int((res[8][2] == 8).sum())}, at k = 16: {int((res[16][2] == 16).sum())}",
                f"  sort (keys, torch.sort, records)              {fmt(sort)}",
                f"  nearest kernel (the yardstick)                {fmt(nearest)}",
                f"  radius moments kernel                         {fmt(radius)}  {x(radius)}",
                f"  k-NN kernel, k = 8                            {fmt(knn[8])}  {x(knn[8])}",
                f"  k-NN kernel, k = 16                           {fmt(knn[16])}  {x(knn[16])}",
                f"  list moments kernel (k = 16)                  {fmt(lists)}",
                f"  normals kernel (Jacobi, a lane per point)     {fmt(normals)}",
                f"  density verdict + selection + gather, a read  {fmt(selection)}",
                f"  whole estimate_normals(radius)                {fmt(whole_normals)}",
                f"  whole estimate_normals(k = 16)                {fmt(whole_normals_k)}",
                f"  whole remove_outliers(radius, min_neighbours = {min_nb}) {fmt(whole_density)}   keeps {len(kept_density.kept)}",
                f"  whole remove_outliers(k = 8, std_ratio = 2)   {fmt(whole_stat)}   keeps {len(kept_stat.kept)}, threshold {kept_stat.threshold:.5f}",
                f"  the density filter from torch.cdist on the same GPU {torch_ms:10.1f} ms = {torch_ms / whole_density[0]:.0f}x the whole call (one pass; "
                f"{n * n / 1e9:.1f} G distances); keeps {len(t_kept)}; counts that differ from the kernel's: {differ}"]
        if kd:
            out += [f"  scipy cKDTree on the CPU, 16 workers: build {kd['build_ms']:.0f} ms, query_ball_point {kd['ball_ms']:.0f} ms = "
                    f"{(kd['build_ms'] + kd['ball_ms']) / (sort[0] + radius[0]):.0f}x sort + radius kernel; query k = 8 {kd['knn8_ms']:.0f} ms = "
                    f"{(kd['build_ms'] + kd['knn8_ms']) / (sort[0] + knn[8][0]):.0f}x, k = 16 {kd['knn16_ms']:.0f} ms = "
                    f"{(kd['build_ms'] + kd['knn16_ms']) / (sort[0] + knn[16][0]):.0f}x sort + k-NN kernel; mean count {kd['mean_count']:.2f} against "
                    f"the kernel's {float(c.mean()):.2f}"]
        else:
            out += ["  scipy is not importable here: no k-d tree comparison"]
        out += [""]
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
