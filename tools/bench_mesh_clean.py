#!/usr/bin/env python3
"""Times the mesh clean-up kernels at sizes a user would run and writes profiles/mesh_clean.txt (commit and device name in the header).

Two meshes, in one process on one GPU: the mesh tools/bench_tsdf.py extracts from its 512^3 volume after 32 views (about 2.6 M
vertices and 4.8 M triangles, with the floaters and border slivers of a fused volume), and a shuffled strip of 2^20 quads, the
long-diameter case.  Per mesh:
  (a) the labelling: the rounds, and per round the hook and the shortcut launch on their own (HIP events around each, the median
      over --repeats whole labellings after --warmup), with their algorithmic bytes against the 5 TB/s mixed-stream rate of DESIGN.md;
  (b) the ranking, the table, the two stable sorts (torch), the fixed-order sums, the filter's two calls and the vertex normals, each
      as the median over --repeats HIP-event brackets;
  (c) whole calls under a host clock that ends in a synchronise, their host reads included: mesh_components, clean_mesh(keep_largest=1),
      clean_mesh(min_triangles=...), vertex_normals;
  (d) yardsticks in the same process: scipy.sparse.csgraph.connected_components on the CPU, and a composition of torch ops on the
      same GPU (min-label rounds with scatter_reduce(amin) and pointer jumping, boolean-mask filtering), whose labels and kept
      triangles the tool compares with the kernels'."""
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
import mesh_cases as MC_  # noqa: E402
from robustmvd_amd import _lib as L  # noqa: E402
from robustmvd_amd import mesh_clean as MC  # noqa: E402
from robustmvd_amd import ops  # noqa: E402
from robustmvd_amd import tsdf as TS  # noqa: E402
from bench_tsdf import ring_scene  # noqa: E402
from bench_vis_mvsnet import event_ms, tree_label  # noqa: E402

STREAM_RATE = 5.0e12  # mixed read/write streams


def tsdf_mesh(n, dev):
    """bench_tsdf.py's volume after its 32 views -> (vertices, triangles) on the device"""
    H, W, V = 768, 1152, 32
    voxel, origin = 3.072 / n, (-1.5, -1.5, 2.4)
    K, Ts, depths = ring_scene(H, W, V)
    vol = TS.TSDFVolume(origin, voxel, (n, n, n), max_weight=64.0, device=dev)
    vol.integrate(depths, [K] * V, Ts)
    mesh = vol.extract_mesh()
    return mesh.vertices, mesh.triangles


def host_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def torch_labels(tri, M):
    """The same rounds from torch ops -> (label, rounds)"""
    label = torch.arange(M, dtype=torch.int64, device=tri.device)
    t = tri.long()
    flat = t.reshape(-1)
    for rounds in range(1, MC.max_rounds(M) + 1):
        m = label[label][t].amin(dim=1).repeat_interleave(3)
        hooked = label.scatter_reduce(0, label[flat], m, "amin").scatter_reduce(0, flat, m, "amin")
        new = hooked[hooked]
        same = bool(torch.equal(new, label))
        label = new
        if same:
            return label, rounds
    raise RuntimeError("torch composition: not converged")


def torch_keep_largest(vertices, tri, M):
    """clean(keep_largest=1) from torch ops -> (vertices, triangles)"""
    label, _ = torch_labels(tri, M)
    tl = label[tri[:, 0].long()]
    roots, counts = torch.unique(tl, return_counts=True)
    keep_t = tl == roots[torch.argmax(counts)]
    kept = tri[keep_t].long()
    used = torch.zeros(M, dtype=torch.bool, device=tri.device)
    used[kept.reshape(-1)] = True
    remap = torch.cumsum(used, 0) - 1
    return vertices[used], remap[kept].int()


def measure(name, vertices, tri, args, out):
    dev = vertices.device
    M, T = int(vertices.shape[0]), int(tri.shape[0])
    ms = lambda t: f"{t[0]:9.4f} ms ({t[1]:.4f}, {t[2]:.4f})"
    share = lambda nbytes, t: f"{nbytes / 1e6:8.1f} MB  {100 * nbytes / (t[0] * 1e-3) / STREAM_RATE:5.1f} % of the rate"
    timed = lambda fn: event_ms(fn, args.warmup, args.repeats)
    out.append(f"{name}: M = {M} vertices, T = {T} triangles")

    # (a) the rounds, launch by launch
    label = torch.empty(M, dtype=torch.int32, device=dev)
    referenced = torch.empty(M, dtype=torch.uint8, device=dev)
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    per_round = []
    for rep in range(args.warmup + args.repeats):
        times = []
        for r in range(MC.max_rounds(M)):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            ops.mesh_hook_round(tri, M, label, referenced, changed, first=r == 0, stages=L.MESH_ROUND_NO_SHORTCUT)
            ev[1].record()
            ops.mesh_hook_round(tri, M, label, referenced, changed, stages=L.MESH_ROUND_NO_HOOK)
            ev[2].record()
            done = int(changed.item()) == 0
            times.append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
            if done:
                break
        if rep >= args.warmup:
            per_round.append(times)
    rounds = len(per_round[0])
    assert all(len(t) == rounds for t in per_round), "the number of rounds changed between two labellings"
    med = np.median(np.asarray(per_round), axis=0)  # (rounds, 2)
    out.append(f"  labelling: {rounds} rounds, the unchanged last one included (cap {MC.max_rounds(M)}); per round the hook / the shortcut launch, ms:")
    out.append("    " + "  ".join(f"{h:.3f}/{s:.3f}" for h, s in med))
    hook_bytes, jump_bytes = 12 * T + 6 * 4 * T, 8 * M
    out.append(f"    sum {med[:, 0].sum():.3f} ms of hooks, {med[:, 1].sum():.3f} ms of shortcuts.  A hook launch moves at least {hook_bytes / 1e6:.1f} MB (the "
               f"triangles once and six 4-byte label gathers each; more where it lowers a label): {100 * hook_bytes / (np.median(med[:, 0]) * 1e-3) / STREAM_RATE:.1f} "
               f"% of the rate at the median round: bound by the random label gathers, not by the stream.  A shortcut moves {jump_bytes / 1e6:.1f} MB "
               f"(label[v] and the gather label[label[v]]): {100 * jump_bytes / (np.median(med[:, 1]) * 1e-3) / STREAM_RATE:.1f} %")
    t_lab = host_ms(lambda: MC._labels_device(tri, M), args.warmup, args.repeats)
    out.append(f"    the whole labelling as the product runs it (both launches per call, the changed word read after every round): {ms(t_lab)} host clock")

    # (b) the stages
    label, referenced, _ = MC._labels_device(tri, M)
    t_rank = timed(lambda: ops.mesh_component_rank(label, referenced))
    vcomp, num = ops.mesh_component_rank(label, referenced)
    C = int(num.item())
    t_table = timed(lambda: ops.mesh_component_table(vcomp, tri, C))
    tcomp, nv = ops.mesh_component_table(vcomp, tri, C)
    t_sort_t = timed(lambda: torch.sort(tcomp, stable=True))
    key, perm = torch.sort(tcomp, stable=True)
    t_sums = timed(lambda: ops.mesh_component_sums(vertices, tri, key, perm, C))
    nt, area = ops.mesh_component_sums(vertices, tri, key, perm, C)
    largest = int(torch.argmax(nt))
    keep = torch.zeros(C, dtype=torch.uint8, device=dev)
    keep[largest] = 1
    t_filter = timed(lambda: ops.mesh_filter(tri, M, tcomp, keep, True))
    new_tri, kept, remap, Mk = ops.mesh_filter(tri, M, tcomp, keep, True)
    t_rows = timed(lambda: ops.mesh_gather_rows(vertices, remap, Mk))
    t_sort_c = timed(lambda: torch.sort(tri.reshape(-1), stable=True))
    ckey, cperm = torch.sort(tri.reshape(-1), stable=True)
    t_norm = timed(lambda: ops.mesh_vertex_normals(vertices, tri, ckey, cperm))
    Tk = int(kept.shape[0])
    out += [f"  components: C = {C}; the largest has {int(nt[largest])} triangles ({100 * int(nt[largest]) / max(T, 1):.2f} %) and {int(nv[largest])} vertices; "
            f"keep_largest=1 keeps M' = {Mk}, T' = {Tk}",
            f"  ranking (count, two-level scan, walk, vertex ids) {ms(t_rank)}  {share(2 * 5 * M + 8 * M, t_rank)}",
            f"  table (triangle ids, vertex counts)               {ms(t_table)}  {share(12 * T + 4 * T + 4 * T + 4 * M, t_table)}  (a random gather per triangle)",
            f"  torch.sort of the T component keys, stable        {ms(t_sort_t)}",
            f"  fixed-order sums (areas, segments, sums)          {ms(t_sums)}  {share(12 * T + 12 * T + 36 * T + 8 * T + 8 * T, t_sums)}  (three random vertex gathers per triangle)",
            f"  filter, both calls with the 16-byte read          {ms(t_filter)}  {share(2 * (4 * T + 12 * T) + 2 * M + 4 * M + 16 * Tk + 12 * Tk, t_filter)}",
            f"  vertices through the remap (gather_rows, k = 3)   {ms(t_rows)}  {share(12 * M + 4 * M + 12 * Mk, t_rows)}",
            f"  torch.sort of the 3 T corner keys, stable         {ms(t_sort_c)}",
            f"  vertex normals (one lane per vertex)              {ms(t_norm)}  {share(12 * 3 * T + 36 * 3 * T + 12 * M, t_norm)}  (a triangle and three vertices gathered per corner)"]

    # (c) whole calls
    t_comp = host_ms(lambda: MC.mesh_components(vertices, tri), args.warmup, args.repeats)
    t_clean = host_ms(lambda: MC.clean_mesh((vertices, tri), keep_largest=1), args.warmup, args.repeats)
    t_clean2 = host_ms(lambda: MC.clean_mesh((vertices, tri), min_triangles=100), args.warmup, args.repeats)
    t_vn = host_ms(lambda: MC.vertex_normals(vertices, tri), args.warmup, args.repeats)
    out += [f"  whole calls, host clock to a synchronise, host reads and index check included:",
            f"    mesh_components            {ms(t_comp)}",
            f"    clean_mesh(keep_largest=1) {ms(t_clean)}",
            f"    clean_mesh(min_triangles=100) {ms(t_clean2)}",
            f"    vertex_normals             {ms(t_vn)}"]

    # (d) yardsticks
    tl, trounds = torch_labels(tri, M)
    assert torch.equal(tl.int(), label), "the torch composition's labels differ from the kernels'"
    tv, tt = torch_keep_largest(vertices, tri, M)
    assert torch.equal(tt, new_tri) and torch.equal(tv, ops.mesh_gather_rows(vertices, remap, Mk)), "the torch composition's mesh differs"
    t_tl = host_ms(lambda: torch_labels(tri, M), 1, max(3, args.repeats // 4))
    t_tk = host_ms(lambda: torch_keep_largest(vertices, tri, M), 1, max(3, args.repeats // 4))
    out += [f"  torch composition on the same GPU (equal labels and equal kept mesh): labelling {ms(t_tl)} in {trounds} rounds, "
            f"{t_tl[0] / t_lab[0]:.1f}x the kernels';  keep_largest=1 {ms(t_tk)}, {t_tk[0] / t_clean[0]:.1f}x clean_mesh"]
    try:
        from scipy import sparse
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        out.append("  scipy: not installed, not measured")
    else:
        th = tri.cpu().numpy().astype(np.int64)
        e = np.concatenate([th[:, [0, 1]], th[:, [1, 2]]])
        graph = sparse.coo_matrix((np.ones(len(e), dtype=np.int8), (e[:, 0], e[:, 1])), shape=(M, M)).tocsr()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            n, lab = connected_components(graph, directed=False)
            times.append((time.perf_counter() - t0) * 1e3)
        nref = int((referenced != 0).sum())
        assert n - (M - nref) == C, "scipy counts other components"
        out.append(f"  scipy.sparse.csgraph.connected_components on the CPU (serial, the CSR graph built before the clock starts): "
                   f"{np.median(times):9.1f} ms ({min(times):.1f}, {max(times):.1f}), {np.median(times) / t_lab[0]:.1f}x the kernels' labelling")
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--n", type=int, default=512, help="the TSDF volume is n^3")
    ap.add_argument("--quads", type=int, default=2 ** 20, help="the strip's quads")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean.txt"))
    ap.add_argument("--commit", default=None, help="commit to name in the header (default: the checkout's)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = [f"Mesh clean-up on {torch.cuda.get_device_name(0)}; commit {args.commit or tree_label()}; tools/bench_mesh_clean.py --warmup "
           f"{args.warmup} --repeats {args.repeats} --n {args.n} --quads {args.quads}",
           f"ms = median (min, max) over {args.repeats} HIP-event brackets of one call each, after {args.warmup}; MB = algorithmic bytes; the rate is "
           f"{STREAM_RATE / 1e12:.0f} TB/s (mixed read/write streams).  The changed word is read after every round.", ""]

    def flush():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(out) + "\n")

    v, t = tsdf_mesh(args.n, dev)
    measure(f"TSDF mesh of the {args.n}^3 volume after 32 views", v, t, args, out)
    flush()
    del v, t
    sv, st = MC_.strip_arrays(2 * args.quads, seed=1)
    measure(f"shuffled strip of {args.quads} quads", torch.from_numpy(sv).to(dev), torch.from_numpy(st).to(dev), args, out)
    flush()
    print("\n".join(out))


if __name__ == "__main__":
    main()
