#!/usr/bin/env python3
"""Times the point-cloud registration and writes profiles/cloud_register.txt (commit and device name in the header).

The workload is profiles/cloud_eval.txt's "fused" pair: the fused cloud of one 768 x 1152 key view with 4 sources as the source, a
voxel-thinned, noisy copy of it as the target.  The target has no normals of its own: the plane-mode sums are timed with random
unit normals, which cost the kernel the same loads and arithmetic.  The source is displaced by the inverse of a known T* (1 degree
about (0.3, -0.5, 0.8) through the cloud's centre, 0.01 of translation) and registered at the radii (4, 2, 1) x 0.04.
  (a) per iteration, at the first and at the last radius: move + records (mvd_cloud_transform_records_f32), the nearest kernel and
      the pair sums in point and in plane mode, and the three calls back to back, each as the median over --repeats HIP-event
      brackets of --inner calls; the host's time to enqueue the three calls, and the wall clock of an iteration with its read and
      its solve;
  (b) a whole register_clouds call in rigid mode (wall clock, with its host reads and solves), its iterations and how far every
      source point lands from where T* puts it; the same call with the source sorted once per stage instead of before every
      iteration;
  (c) the same ICP (the same sums, solver and stop rule, pairs from scipy.spatial.cKDTree with 16 workers) on the same machine's
      CPU, in a child process that imports no GPU library, while this process leaves the GPU idle.
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
MAX_DIST = 0.04
RADII = (4 * MAX_DIST, 2 * MAX_DIST, MAX_DIST)
ITERATIONS = 50


def rotation(axis, degrees):
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def kdtree_child(path):
    """The CPU comparison: rigid ICP with the package's stop rule, pairs from a k-d tree; no GPU library imported."""
    from scipy.spatial import cKDTree
    data = np.load(path)
    s, p = data["source"].astype(np.float64), data["target"].astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(p)
    lo, hi = s.min(0), s.max(0)
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    M, t = np.eye(3), np.zeros(3)
    tol = max(1e-3 * RADII[-1], 2.0 ** -21 * np.abs(p).max())
    total = 0
    for radius in RADII:
        for _ in range(ITERATIONS):
            q = (s @ M.T + t).astype(np.float32).astype(np.float64)
            d, j = tree.query(q, distance_upper_bound=radius, workers=16)
            ok = j < len(p)
            a, b = q[ok], p[j[ok]]
            ma, mb = a.mean(0), b.mean(0)
            U, D, Vt = np.linalg.svd((b - mb).T @ (a - ma) / len(a))
            S = np.array([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
            dM = (U * S) @ Vt
            dt = mb - dM @ ma
            at = corners @ M.T + t
            step = np.linalg.norm(at @ dM.T + dt - at, axis=1).max()
            M, t = dM @ M, dM @ t + dt
            total += 1
            if step <= tol:
                break
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = M, t
    print(json.dumps({"ms": 1000 * (time.perf_counter() - t0), "iterations": total, "transform": T.tolist()}))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--kdtree-child":
        return kdtree_child(sys.argv[2])
    import torch
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from robustmvd_amd import cloud_register as CR
    from robustmvd_amd import depth_fusion as DF
    from robustmvd_amd import ops
    from bench_depth_fusion import bench_scene
    from bench_vis_mvsnet import event_ms, tree_label

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3, help="calls per HIP-event bracket")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_register.txt"))
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
    target = (thin + up(rng.normal(0, 0.003, tuple(thin.shape)).astype(np.float32))).contiguous()
    normals = rng.normal(size=tuple(target.shape))
    normals = up((normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32))
    centre = pred.double().mean(0).cpu().numpy()
    star = np.eye(4)
    star[:3, :3] = rotation((0.3, -0.5, 0.8), 1.0)
    star[:3, 3] = centre - star[:3, :3] @ centre + np.array([0.006, -0.005, 0.006])
    source = ops.cloud_transform(pred, np.linalg.inv(star))
    n, m = len(source), len(target)

    out = [f"point-cloud registration on {torch.cuda.get_device_name(0)}; commit {args.commit or tree_label()}; tools/bench_register.py "
           f"--warmup {args.warmup} --repeats {args.repeats} --inner {args.inner}" + (" --small (REHEARSAL: not a measurement)" if args.small else ""),
           f"{n} source points onto {m} target points, radii {RADII}; ms = median (min, max) per call over HIP-event brackets", ""]

    box = ops.cloud_extent(target)
    pivot = 0.5 * (box[0] + box[1])
    grid = ops.cloud_grid(target, box[0].tolist(), float(np.float32(RADII[0])) * ops.CLOUD_CELL_MARGIN)
    for label, T in (("first iteration (identity, radius %g)" % RADII[0], np.eye(4)), ("last radius (T*, radius %g)" % RADII[-1], star)):
        radius = RADII[0] if T is not star else RADII[-1]
        moved = ops.cloud_transform(source, T)
        perm = ops.cloud_sorted(moved, grid.origin, grid.inv)[1]
        records = ops.cloud_transform_records(source, perm, T)
        index = ops.cloud_nearest_records(records, grid, radius)[1]
        sort = event_ms(lambda: ops.cloud_sorted(ops.cloud_transform(source, T), grid.origin, grid.inv), args.warmup, args.repeats, args.inner)
        move = event_ms(lambda: ops.cloud_transform_records(source, perm, T), args.warmup, args.repeats, args.inner)
        near = event_ms(lambda: ops.cloud_nearest_records(records, grid, radius), args.warmup, args.repeats, args.inner)
        s_pt = event_ms(lambda: ops.cloud_pair_sums(source, T, index, target, pivot), args.warmup, args.repeats, args.inner)
        s_pl = event_ms(lambda: ops.cloud_pair_sums(source, T, index, target, pivot, normals), args.warmup, args.repeats, args.inner)
        pairs = ops.cloud_pair_sums_read(ops.cloud_pair_sums(source, T, index, target, pivot), False)[0]

        def enqueue():
            rec = ops.cloud_transform_records(source, perm, T)
            return ops.cloud_pair_sums(source, T, ops.cloud_nearest_records(rec, grid, radius)[1], target, pivot)

        def iteration():
            N, sums = ops.cloud_pair_sums_read(enqueue(), False)
            return CR.solve_point(N, sums, pivot)

        three = event_ms(enqueue, args.warmup, args.repeats, args.inner)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            iteration()
        wall = 1000 * (time.perf_counter() - t0) / 20
        t0 = time.perf_counter()
        for _ in range(20):
            enqueue()
        host = 1000 * (time.perf_counter() - t0) / 20
        torch.cuda.synchronize()
        gather = (n * 16 + pairs * 12) / 1e6  # index + source (16 B a point) and one target row a pair, in MB
        out += [f"{label}: {pairs} pairs",
                f"  once per stage: move, keys, torch.sort                {sort[0]:8.4f} ms ({sort[1]:.4f}, {sort[2]:.4f})",
                f"  move + records (mvd_cloud_transform_records_f32)      {move[0]:8.4f} ms ({move[1]:.4f}, {move[2]:.4f})",
                f"  nearest kernel                                       {near[0]:8.4f} ms ({near[1]:.4f}, {near[2]:.4f})",
                f"  pair sums, point mode (both kernels)                 {s_pt[0]:8.4f} ms ({s_pt[1]:.4f}, {s_pt[2]:.4f})   "
                f"= {gather / s_pt[0]:.1f} GB/s of index, source and gathered target rows",
                f"  pair sums, plane mode (both kernels)                 {s_pl[0]:8.4f} ms ({s_pl[1]:.4f}, {s_pl[2]:.4f})",
                f"  the three calls of an iteration, back to back        {three[0]:8.4f} ms ({three[1]:.4f}, {three[2]:.4f})   "
                f"their enqueue alone takes the host {host:.4f} ms",
                f"  one iteration with its 256-byte read and solve_point, wall clock, mean of 20: {wall:.4f} ms", ""]

    def whole(resort=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if resort is None:
            reg = CR.register_clouds(source, target, RADII, mode="rigid", iterations=ITERATIONS)
        else:
            reg = CR._register_device(source, target, RADII, "rigid", None, None, ITERATIONS, None, resort=resort)
        torch.cuda.synchronize()
        return reg, 1000 * (time.perf_counter() - t0)

    whole()
    runs = [whole() for _ in range(5)]
    reg = runs[0][0]
    ms = sorted(r[1] for r in runs)
    landing = lambda T: float(np.linalg.norm(source.double().cpu().numpy() @ (np.asarray(T)[:3, :3] - star[:3, :3]).T
                                             + (np.asarray(T)[:3, 3] - star[:3, 3]), axis=1).max())
    policies = []
    for name, resort in (("sorted once per stage", False),):
        whole(resort)
        other = [whole(resort) for _ in range(3)]
        same = np.array_equal(other[0][0].transform, reg.transform)
        policies.append(f"  the same call with the source {name}: {sorted(r[1] for r in other)[1]:.2f} ms (median of 3); the same transform, bit for bit: {same}")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "clouds.npz")
        np.savez(path, source=source.cpu().numpy(), target=target.cpu().numpy())
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--kdtree-child", path], capture_output=True, text=True, check=True)
    kd = json.loads(child.stdout.strip().splitlines()[-1])
    out += [f"whole register_clouds(mode='rigid') call, wall clock with its reads and solves: {ms[2]:.2f} ms (min {ms[0]:.2f}, max {ms[-1]:.2f} of 5); "
            f"{reg.iterations} iterations = {ms[2] / max(reg.iterations, 1):.3f} ms each; converged {reg.converged}, {reg.pairs} pairs, rmse {reg.rmse:.5f}; "
            f"every source point within {landing(reg.transform):.2e} of T* (the target is noisy: sigma 0.003)",
            *policies,
            f"the same ICP with scipy cKDTree pairs (16 workers) on the CPU, build + {kd['iterations']} iterations: {kd['ms']:.0f} ms "
            f"= {kd['ms'] / ms[2]:.0f}x; within {landing(kd['transform']):.2e} of T*", ""]
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
