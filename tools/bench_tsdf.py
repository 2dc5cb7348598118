#!/usr/bin/env python3
"""Times the TSDF kernels at sizes a user would run and writes profiles/tsdf.txt (commit and device name in the header).

A 512^3 volume (voxel 0.006 around the tests' analytic scene A: plane, occluding patch, depth noise), without and with colour, and
768 x 1152 depth maps from 32 cameras on a ring, in one process on one GPU:
  (a) mvd_tsdf_integrate_f32 with V = 1, 4, 8 and 32 views per launch, each as the median over --repeats HIP-event brackets after
      --warmup brackets; a bracket holds as many launches as fill --bracket-ms.  Per launch the algorithmic bytes (the state read
      once, written where the launch stores it, i.e. in the four-voxel groups that one of the V views updates, plus the V maps once)
      and the share of 5 TB/s, the mixed read/write stream rate of DESIGN.md section 8, they amount to;
  (b) the same V views as V launches of one view;
  (c) the same definition composed from torch ops (broadcast index arithmetic, torch.round, index gathers, torch.where) for one view,
      V = 1 against V = 1; the tool prints the agreement with the kernel and refuses weights that differ on more than 0.1 % of the
      voxels or a tsdf that differs by more than 1e-4 on more than 0.5 % of them;
  (d) the extraction of the volume after 32 views: the classification pass with its two scans (the count-only call), the emission pass
      (the call with classified = 1), with M and T, and their algorithmic bytes.
The volume keeps integrating across brackets (max_weight 64 bounds the weights); the work per launch does not depend on the values."""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import fusion_cases as FC  # noqa: E402
from robustmvd_amd import _lib as L  # noqa: E402
from robustmvd_amd import ops  # noqa: E402
from robustmvd_amd import tsdf as TS  # noqa: E402
from bench_vis_mvsnet import event_ms, tree_label  # noqa: E402

STREAM_RATE = 5.0e12  # mixed read/write streams


def ring_scene(H, W, V):
    rng = np.random.default_rng(V)
    K = FC.intrinsics(H, W)
    Ts, depths = [], []
    for i in range(V):
        a = 2 * np.pi * i / V
        r = 0.25 + 0.1 * rng.random()
        T = FC.pose(FC.rot_x(0.03 * np.sin(a + 1)) @ FC.rot_y(-0.03 * np.cos(a)), (r * np.cos(a), r * np.sin(a), 0.02 * np.sin(3 * a)))
        Ts.append(T)
        depths.append((FC.render(K, T, H, W, patch=True) * (1 + FC.NOISE_SIGMA * rng.standard_normal((H, W)))).astype(np.float32))
    return K, Ts, depths


def torch_integrate(F, Wt, C, d, img, m, idx, H, W, trunc, max_weight):
    """One view of the definition from torch ops, in place; m: 12 python floats; idx: the broadcastable index tensors i, j, k."""
    i, j, k = idx
    q = [m[4 * r] * i + m[4 * r + 1] * j + m[4 * r + 2] * k + m[4 * r + 3] for r in range(3)]
    px, py = torch.round(q[0] / q[2]), torch.round(q[1] / q[2])
    inb = (q[2] > 0) & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    pix = torch.where(inb, py * W + px, torch.zeros_like(px)).long()
    dm = d.view(-1)[pix]
    sdf = dm - q[2]
    upd = inb & torch.isfinite(dm) & (dm > 0) & (sdf >= -trunc)
    f = torch.clamp(sdf / trunc, max=1.0)
    Wn = Wt + 1.0
    F.copy_(torch.where(upd, (F * Wt + f) / Wn, F))
    if C is not None:
        for c in range(3):
            C[c].copy_(torch.where(upd, (C[c] * Wt + img[c].view(-1)[pix]) / Wn, C[c]))
    Wt.copy_(torch.where(upd, torch.clamp(Wn, max=max_weight), Wt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--bracket-ms", type=float, default=30.0, help="fill every HIP-event bracket with launches up to this time")
    ap.add_argument("--n", type=int, default=512, help="the volume is n^3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf.txt"))
    ap.add_argument("--commit", default=None, help="commit to name in the header (default: the checkout's)")
    args = ap.parse_args()
    assert args.repeats >= 20, "the figures are medians of at least 20 brackets"
    dev = torch.device("cuda:0")
    lib = L.load()
    n, H, W, VMAX = args.n, 768, 1152, 32
    N = n ** 3
    voxel, origin = 3.072 / n, (-1.5, -1.5, 2.4)
    trunc, max_weight = 3 * voxel, 64.0
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    K, Ts, depths = ring_scene(H, W, VMAX)
    maps = [up(d) for d in depths]
    rng = np.random.default_rng(1)
    images = [up(rng.random((3, H, W)).astype(np.float32) * 255) for _ in range(VMAX)]
    mats_host = np.stack([TS.compose_matrix(K, T, origin, voxel) for T in Ts]).astype(np.float32)
    mats = up(mats_host)
    ms = lambda t: f"{t[0]:9.4f} ms ({t[1]:.4f}, {t[2]:.4f})"

    def timed(fn):
        """event_ms with the bracket filled up to --bracket-ms"""
        one = event_ms(fn, 1, 3)[0]
        return event_ms(fn, args.warmup, args.repeats, max(1, math.ceil(args.bracket_ms / one)))

    out = [f"TSDF volume {n}^3 (voxel {voxel:.4f}, trunc {trunc:.4f}), {H} x {W} maps, on {torch.cuda.get_device_name(0)}; commit "
           f"{args.commit or tree_label()}; tools/bench_tsdf.py --warmup {args.warmup} --repeats {args.repeats} --bracket-ms {args.bracket_ms}",
           f"ms = median (min, max) per launch over HIP-event brackets of at least {args.bracket_ms:.0f} ms; share = algorithmic bytes / time "
           f"/ {STREAM_RATE / 1e12:.0f} TB/s (state read once and stored where a view updated its four-voxel group, + the maps)", ""]
    batched_cheaper = True
    for colour in (False, True):
        F, Wt = torch.zeros((n, n, n), device=dev), torch.zeros((n, n, n), device=dev)
        C = torch.zeros((3, n, n, n), device=dev) if colour else None
        per_voxel, per_pixel = (8 + (12 if colour else 0)) * 2, 4 + (12 if colour else 0)
        out.append(f"integration, {'with' if colour else 'without'} colour ({per_voxel // 2} B of state per voxel, {per_pixel} B per map pixel)")

        def launch(first, V):
            ops.call("mvd_tsdf_integrate_f32", dev, F, Wt, C, n, n, n, maps[first:first + V], None,
                     images[first:first + V] if colour else None, mats[first:first + V], V, H, W, trunc, max_weight)

        # the share of the four-voxel groups that the first V views update: what a launch stores
        stored = {}
        for V in (1, 4, 8, 32):
            Wt.zero_()
            launch(0, V)
            stored[V] = float((Wt.view(-1, 4) > 0).any(dim=1).float().mean())
        touched = float((Wt > 0).float().mean())
        single = timed(lambda: launch(0, 1))
        for V in (1, 4, 8, 32):
            t = single if V == 1 else timed(lambda: launch(0, V))

            def one_by_one():
                for v in range(V):
                    launch(v, 1)

            s = t if V == 1 else timed(one_by_one)
            nbytes = per_voxel // 2 * N * (1 + stored[V]) + per_pixel * H * W * V
            batched_cheaper &= V == 1 or t[0] < s[0]
            out.append(f"  V = {V:2d}  one launch {ms(t)}   {nbytes / 1e9:6.3f} GB ({100 * stored[V]:4.1f} % of the state stored)  "
                       f"{100 * nbytes / (t[0] * 1e-3) / STREAM_RATE:5.1f} % of the rate   {t[0] / V:8.4f} ms per view   {V} launches of one view "
                       f"{ms(s)}   {s[0] / t[0]:5.2f}x")
        out.append(f"  {100 * touched:.1f} % of the voxels are updated by one of the 32 views")

        # the torch composition of one view, on a fresh state next to the kernel's
        idx = (torch.arange(n, dtype=torch.float32, device=dev).view(1, 1, n), torch.arange(n, dtype=torch.float32, device=dev).view(1, n, 1),
               torch.arange(n, dtype=torch.float32, device=dev).view(n, 1, 1))
        tF, tW = torch.zeros_like(F), torch.zeros_like(Wt)
        tC = torch.zeros_like(C) if colour else None
        m0 = mats_host[0].tolist()
        torch_integrate(tF, tW, tC, maps[0], images[0], m0, idx, H, W, trunc, max_weight)
        kF, kW = torch.zeros_like(F), torch.zeros_like(Wt)
        kC = torch.zeros_like(C) if colour else None
        ops.tsdf_integrate(kF, kW, kC, maps[:1], mats[:1], trunc, max_weight, None, images[:1] if colour else None)
        agree = float((tW == kW).float().mean())
        # a voxel whose u or v is within a rounding of a half-integer takes the neighbouring pixel in one of the two: its F may differ by
        # up to 2 at a depth edge, so the share of such voxels is reported, not the largest difference
        differ = float(((tF - kF).abs() > 1e-4).float().mean())
        assert agree > 0.999, f"the torch composition disagrees with the kernel on {100 * (1 - agree):.3f} % of the weights"
        assert differ < 0.005, f"the torch composition's tsdf differs from the kernel's on {100 * differ:.3f} % of the voxels"
        del kF, kW, kC
        tt = timed(lambda: torch_integrate(tF, tW, tC, maps[0], images[0], m0, idx, H, W, trunc, max_weight))
        out += [f"  torch composition, one view {ms(tt)}   {tt[0] / single[0]:6.1f}x the kernel's V = 1 launch; its weights agree with the "
                f"kernel's on {100 * agree:.3f} % of the voxels, its tsdf within 1e-4 on {100 * (1 - differ):.3f} %", ""]
        del tF, tW, tC, idx

        if colour:
            nbytes_ws = lib.mvd_tsdf_extract_workspace_bytes(n, n, n)
            ws = ops.workspace(nbytes_ws, dev)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
            head = (F, Wt, C, n, n, n, *origin, voxel, 1.0)
            ops.call("mvd_tsdf_extract_f32", dev, *head, 0, None, None, None, 0, 0, counts, ws, int(nbytes_ws))
            M, T = counts.tolist()
            vertices, colors = torch.empty((M, 3), device=dev), torch.empty((M, 3), device=dev)
            triangles = torch.empty((T, 3), dtype=torch.int32, device=dev)
            t_c = timed(lambda: ops.call("mvd_tsdf_extract_f32", dev, *head, 0, None, None, None, 0, 0, counts, ws, int(nbytes_ws)))
            t_e = timed(lambda: ops.call("mvd_tsdf_extract_f32", dev, *head, 1, vertices, colors, triangles, M, T, counts, ws, int(nbytes_ws)))
            b_c, b_e = (8 + 2) * N, 2 * N + 24 * M + 12 * T
            out += [f"extraction of the volume above (min_weight 1): M = {M} vertices, T = {T} triangles, workspace {nbytes_ws / 1e6:.0f} MB",
                    f"  classification + scans {ms(t_c)}   {b_c / 1e9:6.3f} GB (tsdf and weight once, two bytes per voxel)  "
                    f"{100 * b_c / (t_c[0] * 1e-3) / STREAM_RATE:5.1f} % of the rate",
                    f"  emission               {ms(t_e)}   {b_e / 1e9:6.3f} GB (two bytes per voxel, the mesh)  "
                    f"{100 * b_e / (t_e[0] * 1e-3) / STREAM_RATE:5.1f} % of the rate", ""]
        del F, Wt, C
    out.append("a launch of V views costs less than V launches of one view, at every V: " + ("yes" if batched_cheaper else "NO"))
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
