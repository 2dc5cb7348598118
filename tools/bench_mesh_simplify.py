#!/usr/bin/env python3
"""Times the mesh simplification at a size a user would run and writes profiles/mesh_simplify.txt (commit and device name in the header).

One mesh, in one process on one GPU: the mesh tools/bench_tsdf.py extracts from its 512^3 volume after 32 views (about 2.6 M vertices
and 4.8 M triangles), simplified at cells of 2, 4 and 8 voxels.  Per cell:
  (a) every step on its own as the median over --repeats HIP-event brackets after --warmup: the keys and their sort, the cluster
      ids, the means, the triples, the corner sort, the quadrics (with the float64 operations and the nominal bytes per corner
      against the device's rates), the placement, the two sorts and the mark of the duplicates, the filter's two calls, the gather;
  (b) the whole simplify_mesh call under a host clock that ends in a synchronise, its host reads included; the output sizes;
  (c) the pay-off: mesh_grid + mesh_nearest of a ground-truth cloud, and one rendered view, on the simplified mesh against the
      original;
  (d) the accuracy lost: MeshEvaluation of the simplified mesh against samples of the original surface;
  (e) yardsticks in the same process: the same definition from torch ops on the same GPU (index_add_ for the sums,
      torch.linalg.solve, torch.unique(dim=0)), compared with the kernels' result; simplify_numpy on a crop that finishes."""
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
import robustmvd_amd as R  # noqa: E402
from robustmvd_amd import mesh_eval as ME  # noqa: E402
from robustmvd_amd import mesh_simplify as MS  # noqa: E402
from robustmvd_amd import ops  # noqa: E402
from bench_mesh_clean import host_ms, tsdf_mesh  # noqa: E402
from bench_tsdf import ring_scene  # noqa: E402
from bench_vis_mvsnet import event_ms, tree_label  # noqa: E402

MAX_DIST, THRESHOLDS = 0.04, (0.005, 0.01)
F64_OPS_PER_CORNER = 53   # counted in cluster_quadrics_kernel: 6 edge differences, 9 for the cross product, 9 for the centre, 3 for q,
#                           6 for d, 10 products, 10 additions (the conversions left out)
BYTES_PER_CORNER = 68     # perm 8, key 4, three indices 12, nine coordinates 36, the cluster's key 8: every one a gather
F64_VECTOR_PEAK = 78.6e12  # the vendor's FP64 vector figure for the MI355X
STREAM_RATE = 5.0e12       # mixed read/write streams


def torch_simplify(v, t, cell, reg=1e-3):
    """The definition from torch ops (unordered float64 sums: index_add_) -> (vertices (K,3) float32, placed, triangles (T',3) int64
    of cluster indices, unique and rotated, in torch.unique's order)."""
    c = float(np.float32(cell))
    f = v.double()
    ok = torch.isfinite(v).all(dim=1)
    o = f[ok].amin(dim=0)
    idx = torch.floor((f - o) * (1.0 / c)).long()
    key = torch.where(ok, (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2], torch.full_like(idx[:, 0], MS.INVALID_KEY))
    ukey, vc = torch.unique(key, return_inverse=True)
    K = int((ukey != MS.INVALID_KEY).sum())
    vc = torch.where(ok, vc, torch.full_like(vc, -1))
    cnt = torch.zeros(K, dtype=torch.float64, device=v.device).index_add_(0, vc[ok], torch.ones(int(ok.sum()), dtype=torch.float64, device=v.device))
    mean = torch.zeros((K, 3), dtype=torch.float64, device=v.device).index_add_(0, vc[ok], f[ok]) / cnt[:, None]
    uk = ukey[:K]
    ctr = (torch.stack([uk >> 42, (uk >> 21) & MS._MASK, uk & MS._MASK], dim=1).double() + 0.5) * c + o
    tl = t.long()
    tc = vc[tl]
    valid = (tc >= 0).all(dim=1)
    tl, tc = tl[valid], tc[valid]
    p0 = f[tl[:, 0]]
    n = torch.linalg.cross(f[tl[:, 1]] - p0, f[tl[:, 2]] - p0)
    Q = torch.zeros((K, 10), dtype=torch.float64, device=v.device)
    for j in range(3):
        q = p0 - ctr[tc[:, j]]
        d = -(n * q).sum(dim=1)
        terms = torch.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2], n[:, 2] * n[:, 2],
                             n[:, 0] * d, n[:, 1] * d, n[:, 2] * d, d * d], dim=1)
        Q.index_add_(0, tc[:, j], terms)
    lam = reg * (Q[:, 0] + Q[:, 3] + Q[:, 5])
    A = torch.stack([Q[:, 0] + lam, Q[:, 1], Q[:, 2], Q[:, 1], Q[:, 3] + lam, Q[:, 4], Q[:, 2], Q[:, 4], Q[:, 5] + lam], dim=1).reshape(K, 3, 3)
    r = -Q[:, 6:9] + lam[:, None] * (mean - ctr)
    solvable = lam > 0
    eye = torch.eye(3, dtype=torch.float64, device=v.device)
    x = torch.linalg.solve(torch.where(solvable[:, None, None], A, eye), r[:, :, None])[:, :, 0]
    good = solvable & torch.isfinite(x).all(dim=1) & (x.abs() <= 0.5 * c).all(dim=1) & (cnt > 1)
    pos = torch.where(good[:, None], ctr + x, mean).float()
    alive = (tc[:, 0] != tc[:, 1]) & (tc[:, 1] != tc[:, 2]) & (tc[:, 0] != tc[:, 2])
    tc = tc[alive]
    first = tc.argmin(dim=1)
    rot = torch.gather(tc, 1, (first[:, None] + torch.arange(3, device=v.device)) % 3)
    return pos, good, torch.unique(rot, dim=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--n", type=int, default=512, help="the TSDF volume is n^3")
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0, 8.0], help="cell edges in voxels")
    ap.add_argument("--gt", type=int, default=400000, help="ground-truth points of the mesh_nearest comparison")
    ap.add_argument("--crop", type=int, default=60000, help="vertices of simplify_numpy's crop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify.txt"))
    ap.add_argument("--commit", default=None, help="commit to name in the header (default: the checkout's)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ms = lambda t: f"{t[0]:9.4f} ms ({t[1]:.4f}, {t[2]:.4f})"
    timed = lambda fn: event_ms(fn, args.warmup, args.repeats)
    out = [f"Mesh simplification on {torch.cuda.get_device_name(0)}; commit {args.commit or tree_label()}; tools/bench_mesh_simplify.py --warmup "
           f"{args.warmup} --repeats {args.repeats} --n {args.n} --cells {' '.join(f'{c:g}' for c in args.cells)} --gt {args.gt} --crop {args.crop}",
           f"ms = median (min, max) over {args.repeats} HIP-event brackets of one call each, after {args.warmup} warm-up calls; whole calls under a "
           "host clock that ends in a synchronise", ""]

    def flush():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(out) + "\n")

    voxel = 3.072 / args.n
    v, t = tsdf_mesh(args.n, dev)
    M, T = int(v.shape[0]), int(t.shape[0])
    H, W = 768, 1152
    K_cam, Ts, _ = ring_scene(H, W, 32)
    samples = ops.mesh_sample(v, t, THRESHOLDS[0])[0]
    g = torch.Generator(device="cpu").manual_seed(1)
    pick = torch.randperm(int(samples.shape[0]), generator=g)[:args.gt].to(dev)
    gt = samples[pick] + 0.004 * torch.randn((len(pick), 3), generator=g).to(dev)
    near_cell = float(np.float32(MAX_DIST)) * ops.CLOUD_CELL_MARGIN
    origin = ME._device_origin(ops, [v, gt])
    qgrid = ops.cloud_grid(gt, origin, near_cell, check=False)
    ev = ME.MeshEvaluation(THRESHOLDS, MAX_DIST)

    def consumers(mv, mt):
        t_grid = host_ms(lambda: ops.mesh_grid(mv, mt, origin, near_cell), 1, 5)
        grid = ops.mesh_grid(mv, mt, origin, near_cell)
        t_near = timed(lambda: ops.mesh_nearest(qgrid, grid, MAX_DIST))
        t_render = host_ms(lambda: R.render_mesh((mv, mt), [K_cam], [Ts[0]], (H, W)), 1, 5)
        return t_grid, t_near, t_render

    base = consumers(v, t)
    out += [f"TSDF mesh of the {args.n}^3 volume (voxel {voxel:.4f}) after 32 views: M = {M} vertices, T = {T} triangles",
            f"  the consumers on the ORIGINAL mesh: mesh_grid (host clock) {ms(base[0])}; mesh_nearest of {len(gt)} points {ms(base[1])}; one "
            f"{H} x {W} view of render_mesh (host clock) {ms(base[2])}", ""]
    flush()

    for mult in args.cells:
        cell = float(np.float32(mult * voxel))
        inv = 1.0 / cell
        extent = ops.cloud_extent(v)
        o = extent[0].tolist()
        t_keys = timed(lambda: ops.cloud_sorted(v, o, inv))
        t_ids = host_ms(lambda: ops.mesh_cluster_ids(v, cell), args.warmup, args.repeats)
        cl = ops.mesh_cluster_ids(v, cell)
        K = cl.num_clusters
        t_means = timed(lambda: ops.mesh_cluster_means(v, cl))
        means = ops.mesh_cluster_means(v, cl)
        t_tri = timed(lambda: ops.mesh_cluster_triples(t, cl))
        triples, alive, corner = ops.mesh_cluster_triples(t, cl)
        t_csort = timed(lambda: torch.sort(corner.reshape(-1), stable=True))
        key, perm = torch.sort(corner.reshape(-1), stable=True)
        t_quad = timed(lambda: ops.mesh_cluster_quadrics(v, t, key, perm, cl))
        quadrics = ops.mesh_cluster_quadrics(v, t, key, perm, cl)
        corners = int((key < K).sum())
        seg = torch.bincount(key[key < K].long(), minlength=K)
        t_place = timed(lambda: ops.mesh_cluster_place(v, cl, means, quadrics, 1e-3))

        def dedup_sorts():
            p1 = torch.sort(triples[:, 2], stable=True)[1]
            pair = (triples[:, 0].to(torch.int64) << 32) | triples[:, 1].to(torch.int64)
            pair = torch.where(alive.bool(), pair, torch.full_like(pair, MS.INVALID_KEY))
            return p1[torch.sort(pair[p1], stable=True)[1]]

        t_dsort = timed(dedup_sorts)
        order = dedup_sorts()
        t_mark = timed(lambda: ops.mesh_cluster_mark_first(triples, alive, order))
        keep = ops.mesh_cluster_mark_first(triples, alive, order)
        own = torch.arange(T, dtype=torch.int32, device=dev)
        t_filter = host_ms(lambda: ops.mesh_filter(triples, K, own, keep, True), args.warmup, args.repeats)
        pos, placed = ops.mesh_cluster_place(v, cl, means, quadrics, 1e-3)
        _, _, remap, Mk = ops.mesh_filter(triples, K, own, keep, True)
        t_gather = timed(lambda: ops.mesh_gather_rows(pos, remap, Mk))
        t_whole = host_ms(lambda: R.simplify_mesh((v, t), cell), 1, max(3, args.repeats // 2))
        t_mean = host_ms(lambda: R.simplify_mesh((v, t), cell, placement="mean"), 1, max(3, args.repeats // 2))
        res = R.simplify_mesh((v, t), cell, details=True)
        sv, st = res.mesh.vertices, res.mesh.triangles
        Ms, Tsz = int(sv.shape[0]), int(st.shape[0])
        rate = corners / (t_quad[0] * 1e-3)
        out += [f"cell = {mult:g} voxels = {cell:.5f}: K = {K} clusters ({M / max(K, 1):.1f} vertices each), {corners} corners in segments of up to "
                f"{int(seg.max())} ({100 * float((seg > 64).float().mean()):.1f} % of the clusters above 64: the wave's path); alive triangles "
                f"{int(alive.sum())}, kept {int(keep.sum())}",
                f"  keys + torch.sort of the M keys, stable        {ms(t_keys)}",
                f"  whole mesh_cluster_ids: extent read, keys, sort, ids, the read of K (host clock) {ms(t_ids)}",
                f"  means of the positions (K,3)                   {ms(t_means)}",
                f"  triples, alive bytes and corner keys           {ms(t_tri)}",
                f"  torch.sort of the 3 T corner keys, stable      {ms(t_csort)}",
                f"  quadrics (segments + the walk)                 {ms(t_quad)}   {rate / 1e9:.2f} G corners per second = "
                f"{rate * F64_OPS_PER_CORNER / 1e12:.3f} T float64 operations per second ({100 * rate * F64_OPS_PER_CORNER / F64_VECTOR_PEAK:.2f} % of "
                f"{F64_VECTOR_PEAK / 1e12:.1f} T) and {rate * BYTES_PER_CORNER / 1e12:.3f} TB/s of gathered operands at {BYTES_PER_CORNER} B per corner "
                f"({100 * rate * BYTES_PER_CORNER / STREAM_RATE:.1f} % of {STREAM_RATE / 1e12:.0f} TB/s)",
                f"  placement (one lane per cluster)               {ms(t_place)}",
                f"  duplicates: two torch.sort of T keys + gathers {ms(t_dsort)}",
                f"  duplicates: mark the first of each run         {ms(t_mark)}",
                f"  mesh_filter, both calls and its read (host clock) {ms(t_filter)}",
                f"  mesh_gather_rows of the positions              {ms(t_gather)}",
                f"  whole simplify_mesh, quadric placement (host clock) {ms(t_whole)};  placement='mean' {ms(t_mean)}",
                f"  result: {Ms} vertices ({100 * Ms / M:.2f} %), {Tsz} triangles ({100 * Tsz / T:.2f} %); placed "
                f"{torch.bincount(res.placed.long(), minlength=3).tolist()} (mean, quadric, single)"]
        flush()
        c = consumers(sv, st)
        out.append(f"  the consumers on the simplified mesh: mesh_grid {ms(c[0])} ({base[0][0] / c[0][0]:.2f}x); mesh_nearest {ms(c[1])} "
                   f"({base[1][0] / c[1][0]:.2f}x); render_mesh {ms(c[2])} ({base[2][0] / c[2][0]:.2f}x)")
        for name, mesh in (("quadric", res.mesh), ("mean", R.simplify_mesh((v, t), cell, placement="mean"))):
            score = ev((mesh.vertices, mesh.triangles), samples)
            out.append(f"  accuracy lost, placement {name}: MeshEvaluation against the {int(samples.shape[0])} samples of the original: accuracy "
                       f"{score.accuracy:.6f}, completeness {score.completeness:.6f} ({score.accuracy / voxel:.4f} / {score.completeness / voxel:.4f} voxels), "
                       f"F {np.round(score.fscore, 4).tolist()} at {THRESHOLDS}")
        flush()
        t_torch = host_ms(lambda: torch_simplify(v, t, cell), 1, 3)
        tp, tgood, ttri = torch_simplify(v, t, cell)
        mine = R.simplify_mesh((v, t), cell, remove_unreferenced=False, details=True)
        same_t = int(ttri.shape[0]) == int(mine.mesh.triangles.shape[0]) and bool(
            torch.equal(ttri, torch.unique(mine.mesh.triangles.long(), dim=0)))
        gap = float((tp - mine.mesh.vertices).abs().max())
        out.append(f"  the definition from torch ops on the same GPU (index_add_, linalg.solve, unique(dim=0)) (host clock) {ms(t_torch)} = "
                   f"{t_torch[0] / t_whole[0]:.2f}x the whole call; same triangle set {same_t}, placed flags differ on "
                   f"{int((tgood != (mine.placed == 1)).sum())} clusters, max |vertex difference| {gap:.2e} ({gap / cell:.2e} cells)")
        flush()

    # simplify_numpy on a crop: the first vertices of the extraction (a slab of the volume) and the triangles among them
    Mc = min(args.crop, M)
    hv = v[:Mc].cpu().numpy()
    ht = t[(t < Mc).all(dim=1)].cpu().numpy()
    cell = float(np.float32(args.cells[0] * voxel))
    t0 = time.perf_counter()
    hres = MS.simplify_numpy(hv, ht, cell)
    t_np = (time.perf_counter() - t0) * 1e3
    dv, dt = torch.from_numpy(hv).to(dev), torch.from_numpy(ht).to(dev)
    t_crop = host_ms(lambda: R.simplify_mesh((dv, dt), cell), 1, 5)
    dres = R.simplify_mesh((dv, dt), cell)
    out += ["", f"simplify_numpy on a crop of {Mc} vertices and {len(ht)} triangles at {args.cells[0]:g} voxels: {t_np:.0f} ms on the CPU; the kernels on the "
            f"same crop {ms(t_crop)} (host clock): {t_np / t_crop[0]:.0f}x; triangles equal {bool(np.array_equal(dres.triangles.cpu().numpy(), hres.mesh.triangles))}, "
            f"vertices bit-equal on {100 * float((dres.vertices.cpu().numpy().view(np.uint32) == hres.mesh.vertices.view(np.uint32)).mean()):.3f} % of the coordinates", ""]
    flush()
    print("\n".join(out))


if __name__ == "__main__":
    main()
