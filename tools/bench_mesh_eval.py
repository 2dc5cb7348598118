#!/usr/bin/env python3
"""Times the mesh-evaluation kernels at a size a user would run and writes profiles/mesh_eval.txt (commit and device name in the header).

One mesh, in one process on one GPU: the mesh tools/bench_tsdf.py extracts from its 512^3 volume after 32 views (about 2.6 M vertices
and 4.8 M triangles), against a ground-truth cloud of --gt points (the order of profiles/cloud_eval.txt's): samples of the same
surface with N(0, 0.004) noise on every coordinate.  max_dist 0.04, thresholds (0.005, 0.01).
  (a) the grid: cell counts, the prefix sum and its one read, pair emission, torch.sort, records, each as the median over --repeats
      HIP-event brackets after --warmup; the pair count P / T;
  (b) mesh_nearest of the ground truth against the grid, with the number of (lane, record) evaluations the waves make (recomputed
      on the host from the sorted keys by the kernel's own grouping), so that the rate can be set against the VALU and LDS peaks;
  (c) sampling at the smallest threshold: counts, emission;
  (d) a whole MeshEvaluation call under a host clock that ends in a synchronise, its host reads included;
  (e) yardsticks in the same process: cloud_nearest of the same queries against the mesh's VERTICES (the cheaper, wrong answer: what the
      triangle arithmetic costs over the point kernel); the definition as chunked torch on the same GPU on --subset queries, scaled;
      scipy's cKDTree on the samples on the CPU with 16 workers."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from robustmvd_amd import mesh_eval as ME  # noqa: E402
from robustmvd_amd import ops  # noqa: E402
from bench_mesh_clean import host_ms, tsdf_mesh  # noqa: E402
from bench_vis_mvsnet import event_ms, tree_label  # noqa: E402

MAX_DIST, THRESHOLDS = 0.04, (0.005, 0.01)
VALU_LANE_OPS = 256 * 4 * 16 * 2.4e9  # 256 CUs x 4 SIMDs x 16 lanes per clock at 2.4 GHz
LDS_BYTES = 256 * 256 * 2.4e9         # 256 B/clk/CU for ds_read_b128 (a broadcast read still takes its 4 LDS cycles per wave)
# vector instructions per (lane, record), counted in the compiled scan loop (246 for the two records of an iteration); four of them are
# v_rcp_f32, which issue at a quarter of the rate and so take the slots of 16
VALU_PER_EVAL, VALU_SLOTS_PER_EVAL = 123, 123 + 4 * 3


def torch_d2(q, A, B, C):
    """mesh_eval.triangle_d2_numpy in float32 torch: q (n,1,3) against A, B, C (1,m,3) -> (n,m)"""
    dot = lambda u, v: (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]

    def seg(p, E):
        ee = dot(E, E)
        t = torch.where(ee == 0, torch.zeros_like(ee), (-dot(p, E) / torch.where(ee == 0, torch.ones_like(ee), ee)).clamp(0, 1))
        r = p + t[..., None] * E
        return dot(r, r)

    a, b, c = A - q, B - q, C - q
    E0, E1, E2 = B - A, C - B, A - C
    d2 = torch.minimum(seg(a, E0), torch.minimum(seg(b, E1), seg(c, E2)))
    n = torch.linalg.cross(E0, E1)
    nn = dot(n, n)
    inside = (nn > 0) & (dot(n, torch.linalg.cross(a, E0.expand_as(a))) >= 0) & (dot(n, torch.linalg.cross(b, E1.expand_as(b))) >= 0) \
        & (dot(n, torch.linalg.cross(c, E2.expand_as(c))) >= 0)
    na = dot(n, a)
    return torch.where(inside, torch.minimum(d2, na * na / torch.where(nn > 0, nn, torch.ones_like(nn))), d2)


def torch_distance(q, v, t, md, chunk=1 << 18):
    best = torch.full((q.shape[0],), float("inf"), device=q.device)
    for b in range(0, t.shape[0], chunk):
        tri = t[b:b + chunk].long()
        best = torch.minimum(best, torch_d2(q[:, None, :], v[tri[:, 0]][None], v[tri[:, 1]][None], v[tri[:, 2]][None]).amin(dim=1))
    return best.sqrt().clamp(max=md)


def scanned_records(query_grid, keys, origin, inv):
    """The (lane, record) evaluations of mesh_nearest_kernel, from its own grouping: per wave of 64 sorted queries, per group (the
    leader's column, z within 3 above), the records of the nine runs; every one of the 64 lanes scans each of them."""
    rec = query_grid.records[:, :3].double().cpu().numpy()
    cells = np.floor((rec - np.asarray(origin)) * inv).astype(np.int64)
    keys = keys.cpu().numpy()
    total = 0
    for b in range(0, len(cells), 64):
        c = cells[b:b + 64]
        todo = np.ones(len(c), dtype=bool)
        while todo.any():
            g = c[np.argmax(todo)]
            todo &= ~((c[:, 0] == g[0]) & (c[:, 1] == g[1]) & (c[:, 2] - g[2] >= 0) & (c[:, 2] - g[2] < 4))
            x, y = np.meshgrid(g[0] + np.arange(-1, 2), g[1] + np.arange(-1, 2), indexing="ij")
            ok = (x >= 0) & (y >= 0)
            lo = (x[ok] << 42) | (y[ok] << 21) | max(g[2] - 1, 0)
            hi = (x[ok] << 42) | (y[ok] << 21) | (g[2] + 4)
            total += int((np.searchsorted(keys, hi, side="right") - np.searchsorted(keys, lo, side="left")).sum())
    return 64 * total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--n", type=int, default=512, help="the TSDF volume is n^3")
    ap.add_argument("--gt", type=int, default=400000, help="ground-truth points")
    ap.add_argument("--subset", type=int, default=64, help="queries of the chunked torch definition")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_eval.txt"))
    ap.add_argument("--commit", default=None, help="commit to name in the header (default: the checkout's)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ms = lambda t: f"{t[0]:9.4f} ms ({t[1]:.4f}, {t[2]:.4f})"
    timed = lambda fn: event_ms(fn, args.warmup, args.repeats)
    out = [f"Mesh evaluation on {torch.cuda.get_device_name(0)}; commit {args.commit or tree_label()}; tools/bench_mesh_eval.py --warmup "
           f"{args.warmup} --repeats {args.repeats} --n {args.n} --gt {args.gt} --subset {args.subset}",
           f"max_dist {MAX_DIST}, thresholds {THRESHOLDS}; ms = median (min, max) over {args.repeats} HIP-event brackets of one call each, after "
           f"{args.warmup} warm-up calls; whole calls under a host clock that ends in a synchronise", ""]

    def flush():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(out) + "\n")

    v, t = tsdf_mesh(args.n, dev)
    M, T = int(v.shape[0]), int(t.shape[0])
    spacing = THRESHOLDS[0]
    samples = ops.mesh_sample(v, t, spacing)[0]
    S = int(samples.shape[0])
    g = torch.Generator(device="cpu").manual_seed(1)
    pick = torch.randperm(S, generator=g)[:args.gt].to(dev)
    gt = samples[pick] + 0.004 * torch.randn((len(pick), 3), generator=g).to(dev)
    out.append(f"TSDF mesh of the {args.n}^3 volume after 32 views: M = {M} vertices, T = {T} triangles; ground truth {len(gt)} points; "
               f"{S} samples at a spacing of {spacing}")

    # (a) the grid
    cell = float(np.float32(MAX_DIST)) * ops.CLOUD_CELL_MARGIN
    origin = ME._device_origin(ops, [v, gt])
    inv = 1.0 / cell
    counts = torch.empty(T, dtype=torch.int64, device=dev)
    t_counts = timed(lambda: ops.call("mvd_mesh_cell_counts_f32", dev, v, M, t, T, origin[0], origin[1], origin[2], inv, counts))
    t_ends = host_ms(lambda: ops._mesh_ends(counts), args.warmup, args.repeats)
    ends, P, largest = ops._mesh_ends(counts)
    keys = torch.empty(P, dtype=torch.int64, device=dev)
    ptri = torch.empty(P, dtype=torch.int32, device=dev)
    t_pairs = timed(lambda: ops.call("mvd_mesh_pairs_f32", dev, v, M, t, T, ends, P, origin[0], origin[1], origin[2], inv, keys, ptri))
    t_sort = timed(lambda: torch.sort(keys, stable=True))
    skeys, perm = torch.sort(keys, stable=True)
    records = torch.empty((P, 12), dtype=torch.float32, device=dev)
    t_rec = timed(lambda: ops.call("mvd_mesh_records_f32", dev, v, M, t, T, ptri, perm, P, records))
    t_grid = host_ms(lambda: ops.mesh_grid(v, t, origin, cell), args.warmup, args.repeats)
    out += [f"  grid at a cell of {cell:.5f}: P = {P} pairs, P / T = {P / T:.3f}, the largest box {largest} cells",
            f"    cell counts (one lane per triangle)        {ms(t_counts)}",
            f"    torch.cumsum + the one read (host clock)   {ms(t_ends)}",
            f"    pair emission (one lane per pair)          {ms(t_pairs)}",
            f"    torch.sort of the P keys, stable           {ms(t_sort)}",
            f"    records (48 bytes per pair)                {ms(t_rec)}",
            f"    whole ops.mesh_grid, extent check included (host clock) {ms(t_grid)}"]
    flush()

    # (b) the nearest kernel
    grid = ops.mesh_grid(v, t, origin, cell)
    qgrid = ops.cloud_grid(gt, origin, cell, check=False)
    t_near = timed(lambda: ops.mesh_nearest(qgrid, grid, MAX_DIST))
    dist, index = ops.mesh_nearest(qgrid, grid, MAX_DIST)
    evals = scanned_records(qgrid, grid.keys, origin, inv)
    rate = evals / (t_near[0] * 1e-3)
    out += [f"  mesh_nearest, {len(gt)} sorted queries           {ms(t_near)}   found {100 * float((index >= 0).float().mean()):.1f} %, mean distance "
            f"{float(dist.double().mean()):.5f}",
            f"    {evals / 1e9:.3f} G (lane, record) evaluations ({evals / 64 / max(len(gt), 1):.0f} records per query's wave and lane) = {rate / 1e12:.3f} T per second.  "
            f"At {VALU_PER_EVAL} vector instructions each (four of them quarter-rate reciprocals: {VALU_SLOTS_PER_EVAL} issue slots) that is "
            f"{100 * rate * VALU_SLOTS_PER_EVAL / VALU_LANE_OPS:.0f} % of the {VALU_LANE_OPS / 1e12:.1f} T lane-operations per second of the VALUs at 2.4 GHz; the three broadcast ds_read_b128 per (wave, record) are {100 * rate / 64 * 3 * 1024 / LDS_BYTES:.1f} % of the LDS read rate (1024 bytes, 4 LDS cycles, per wave-instruction); the staging "
            f"loads are 48 bytes per (wave, record), {rate / 64 * 48 / 1e12:.3f} TB/s, mostly from L2"]
    flush()

    # (c) sampling
    inv_s2 = 1.0 / (float(np.float32(spacing)) ** 2)
    t_sc = timed(lambda: ops.call("mvd_mesh_sample_counts_f32", dev, v, M, t, T, inv_s2, counts))
    sends = torch.cumsum(counts, 0)
    pts, stri = torch.empty((S, 3), dtype=torch.float32, device=dev), torch.empty(S, dtype=torch.int32, device=dev)
    t_se = timed(lambda: ops.call("mvd_mesh_sample_f32", dev, v, M, t, T, None, 0, sends, S, inv_s2, pts, stri, None))
    t_sw = host_ms(lambda: ops.mesh_sample(v, t, spacing), args.warmup, args.repeats)
    out += [f"  sampling at {spacing}: S = {S} samples, S / T = {S / T:.2f}",
            f"    sample counts (one lane per triangle)      {ms(t_sc)}",
            f"    sample emission (one lane per sample)      {ms(t_se)}   {16 * S / 1e6:.0f} MB written, {16 * S / (t_se[0] * 1e-3) / 1e12:.2f} TB/s",
            f"    whole ops.mesh_sample (host clock)         {ms(t_sw)}"]
    flush()

    # (d) the whole evaluation
    ev = ME.MeshEvaluation(THRESHOLDS, MAX_DIST)
    t_ev = host_ms(lambda: ev((v, t), gt), 1, max(3, args.repeats // 2))
    score = ev((v, t), gt)
    out += [f"  whole MeshEvaluation call, mesh against cloud (samples, three sorts, the grid, two searches, two scores, the reads) {ms(t_ev)}",
            f"    accuracy {score.accuracy:.5f}, completeness {score.completeness:.5f}, F {np.round(score.fscore, 4).tolist()}, n_pred {score.n_pred}, n_gt {score.n_gt}"]
    flush()

    # (e) yardsticks
    vgrid = ops.cloud_grid(v, origin, cell)
    t_cn = timed(lambda: ops.cloud_nearest(qgrid, vgrid, MAX_DIST))
    dv, iv = ops.cloud_nearest(qgrid, vgrid, MAX_DIST)
    # a vertex that no triangle names (the extraction keeps them) can be nearer than the surface; a referenced one never by more than rounding
    referenced = torch.zeros(M, dtype=torch.bool, device=dev)
    referenced[t.reshape(-1).long()] = True
    below = (dv < dist) & (iv >= 0)
    by_ref = below & referenced[iv.clamp(min=0).long()]
    out.append(f"  cloud_nearest of the same queries against the {M} VERTICES (the cheaper, wrong answer) {ms(t_cn)}: mesh_nearest is {t_near[0] / t_cn[0]:.1f}x; "
               f"the vertex distance is above the surface distance by {float((dv - dist).double().mean()):.5f} on average; it is below it for {int(below.sum())} queries, "
               f"of which {int((below & ~by_ref).sum())} have an unreferenced vertex nearest ({int((~referenced).sum())} of the mesh's vertices) and the other "
               f"{int(by_ref.sum())} differ by at most {float((dist - dv)[by_ref].max()) if bool(by_ref.any()) else 0.0:.1e}")
    sub = gt[:args.subset]
    t_td = host_ms(lambda: torch_distance(sub, v, t, MAX_DIST), 1, 3)
    td = torch_distance(sub, v, t, MAX_DIST)
    want = ops.mesh_nearest(sub, grid, MAX_DIST)[0]
    scaled = t_td[0] * len(gt) / max(len(sub), 1)
    out.append(f"  the definition as chunked torch on the same GPU, {len(sub)} queries x {T} triangles: {ms(t_td)}, scaled to {len(gt)} queries {scaled:.0f} ms = "
               f"{scaled / t_near[0]:.0f}x mesh_nearest ({scaled / (t_near[0] + t_grid[0]):.0f}x with the grid's build); max |torch - kernel| {float((td - want).abs().max()):.2e}")
    flush()
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        out.append("  scipy: not installed, not measured")
    else:
        sh, gh = samples.cpu().numpy().astype(np.float64), gt.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(sh)
        t1 = time.perf_counter()
        dk, _ = tree.query(gh, distance_upper_bound=MAX_DIST, workers=16)
        t2 = time.perf_counter()
        dk = np.minimum(dk, MAX_DIST)
        out.append(f"  scipy cKDTree on the {S} samples on the CPU: build {1e3 * (t1 - t0):.0f} ms, query of the ground truth with 16 workers {1e3 * (t2 - t1):.0f} ms = "
                   f"{1e3 * (t2 - t0) / (t_near[0] + t_grid[0] ):.0f}x the grid and mesh_nearest; the nearest sample is {float((dk - dist.cpu().numpy()).mean()):.5f} "
                   f"farther than the surface on average")
    out.append("")
    flush()
    print("\n".join(out))


if __name__ == "__main__":
    main()
