#!/usr/bin/env python3
"""Times the mesh-rendering kernels at sizes a user would run and writes profiles/mesh_render.txt (commit and device name in the
header).

The mesh is the one tools/bench_tsdf.py extracts: a 512^3 volume (voxel 0.006 around the tests' analytic scene A) after 32 views of
768 x 1152 from cameras on a ring, about 2.6 M vertices and 4.8 M triangles of about one pixel each.  It is rendered back into those
cameras at 768 x 1152, alone and with a ground quad behind it that fills every image (two triangles far larger than the image: the
wave path and full-image occlusion), in one process on one GPU:
  (a) per stage (project; rasterise = key fill, setup + lane path, scans, list, wave path; resolve) and for the whole call, at
      V = 1, 4 and 32 views per call, each as the median over --repeats HIP-event brackets after --warmup; per stage the algorithmic
      bytes and the share of 5 TB/s, the mixed read/write stream rate of DESIGN.md section 8, they amount to.  The bytes of the
      atomics themselves are not in that figure: the rate of 64-bit integer min atomics on this part is not in the guides and has
      not been measured apart from these kernels;
  (b) max_small swept from 0 (every triangle on the wave path) to H W (every triangle on its lane) against the default, at V = 1 and 4;
  (c) the plain load of the key before the atomic on and off;
  (d) the only baseline there is: render_numpy (float64, the CPU of the same box) on the tests' sphere+plane mesh at 96 x 131, three
      views, against the kernels on the same input."""
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
import render_cases as RC  # noqa: E402
from robustmvd_amd import _lib as L  # noqa: E402
from robustmvd_amd import ops  # noqa: E402
from robustmvd_amd import render as R  # noqa: E402
from robustmvd_amd import tsdf as TS  # noqa: E402
from bench_tsdf import ring_scene  # noqa: E402
from bench_vis_mvsnet import event_ms, tree_label  # noqa: E402

STREAM_RATE = 5.0e12  # mixed read/write streams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--n", type=int, default=512, help="the volume is n^3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_render.txt"))
    ap.add_argument("--commit", default=None, help="commit to name in the header (default: the checkout's)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, H, W, VMAX = args.n, 768, 1152, 32
    voxel, origin = 3.072 / n, (-1.5, -1.5, 2.4)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    K, Ts, depths = ring_scene(H, W, VMAX)
    vol = TS.TSDFVolume(origin, voxel, (n, n, n), device=dev)
    vol.integrate([up(d) for d in depths], [K] * VMAX, Ts)
    mesh = vol.extract_mesh()
    del vol
    torch.cuda.empty_cache()
    quad = up(np.array([[-9, -9, 5.0], [9, -9, 5.0], [9, 9, 5.0], [-9, 9, 5.0]], dtype=np.float32))
    M0, T0 = len(mesh.vertices), len(mesh.triangles)
    meshes = {"mesh alone": (mesh.vertices, mesh.triangles),
              "mesh + ground quad": (torch.cat([mesh.vertices, quad]),
                                     torch.cat([mesh.triangles, torch.tensor([[0, 2, 1], [0, 3, 2]], dtype=torch.int32, device=dev) + M0]))}
    mats = up(np.stack([R.compose_projection(K, T) for T in Ts]).astype(np.float32))
    ms = lambda t: f"{t[0]:9.4f} ms ({t[1]:.4f}, {t[2]:.4f})"
    timed = lambda fn, repeats=args.repeats: event_ms(fn, args.warmup, repeats)

    out = [f"mesh rendering, {H} x {W}, the {n}^3 mesh of tools/bench_tsdf.py (M = {M0} vertices, T = {T0} triangles), on "
           f"{torch.cuda.get_device_name(0)}; commit {args.commit or tree_label()}; tools/bench_render.py --warmup {args.warmup} --repeats "
           f"{args.repeats}",
           f"ms = median (min, max) per call over HIP-event brackets; share = algorithmic bytes / time / {STREAM_RATE / 1e12:.0f} TB/s.  "
           "Bytes: project 12 M V read + 16 M V written; rasterise 8 H W V (key fill) + (12 + 48 + 1) T V (indices, three records, "
           "flag), without the atomics and the plain loads before them, whose rate nobody has measured apart from these kernels; resolve "
           "(8 + 8) H W V, + (12 + 48 + 12) H W V with bary and + (12 + 36 + 12) H W V with normals on covered pixels", ""]

    def runner(v, t, V, **kw):
        """-> call(stages, **more): one ops.mesh_render on a workspace and maps that are allocated once"""
        Mv, Tv = len(v), len(t)
        ws = ops.workspace(L.load().mvd_mesh_render_workspace_bytes(Mv, Tv, V, H, W), dev)
        first = ops.mesh_render(v, t, mats[:V], (H, W), check_indices=False, workspace_=ws, **kw)

        def call(stages=0, **more):
            ops.mesh_render(v, t, mats[:V], (H, W), check_indices=False, workspace_=ws, out=first, stages=stages, **{**kw, **more})
        return call, first

    for label, (v, t) in meshes.items():
        Mv, Tv = len(v), len(t)
        out.append(f"{label} (M = {Mv}, T = {Tv})")
        for V in (1, 4, 32):
            for maps, kw in (("depth + triangle", {}), ("+ bary + normals", {"bary": True, "normals": True})):
                call, first = runner(v, t, V, **kw)
                covered = float((first["triangle"] >= 0).float().mean())
                if not kw:
                    t_p = timed(lambda: call(L.RENDER_KEEP_KEYS | L.RENDER_NO_RESOLVE))
                    t_r = timed(lambda: call(L.RENDER_KEEP_PROJECT | L.RENDER_NO_RESOLVE))
                    b_p, b_r = 28 * Mv * V, 8 * H * W * V + 61 * Tv * V
                    out.append(f"  V = {V:2d}  project   {ms(t_p)}  {t_p[0] / V:8.4f} ms per view  {b_p / 1e9:6.3f} GB "
                               f"{100 * b_p / (t_p[0] * 1e-3) / STREAM_RATE:5.1f} % of the rate")
                    out.append(f"          rasterise {ms(t_r)}  {t_r[0] / V:8.4f} ms per view  {b_r / 1e9:6.3f} GB "
                               f"{100 * b_r / (t_r[0] * 1e-3) / STREAM_RATE:5.1f} % of the rate   ({100 * covered:.1f} % of the pixels covered)")
                t_s = timed(lambda: call(L.RENDER_KEEP_PROJECT | L.RENDER_KEEP_KEYS))
                t_w = timed(lambda: call(0))
                b_s = (16 + (132 * covered if kw else 0)) * H * W * V
                out.append(f"          resolve   {ms(t_s)}  {t_s[0] / V:8.4f} ms per view  {b_s / 1e9:6.3f} GB "
                           f"{100 * b_s / (t_s[0] * 1e-3) / STREAM_RATE:5.1f} % of the rate   [{maps}]")
                out.append(f"          whole     {ms(t_w)}  {t_w[0] / V:8.4f} ms per view   [{maps}]")
                del call, first
                torch.cuda.empty_cache()
        out.append("  max_small (rasterise stage alone; 0: every triangle on the wave path, H W: every triangle on its lane)")
        for V in (1, 4):
            call, _ = runner(v, t, V)
            row = []
            for max_small in (0, 4, 16, 64, 256, 1024, 4096, H * W):
                few = max_small in (0, H * W)  # the two extremes are slow by design
                tm = event_ms(lambda: call(L.RENDER_KEEP_PROJECT | L.RENDER_NO_RESOLVE, max_small=max_small), 1, 5 if few else args.repeats)
                row.append(f"{max_small}: {tm[0]:.4f}")
            out.append(f"    V = {V}  " + "   ".join(row) + "  ms")
            row = []
            for load_first in (False, True):
                tm = timed(lambda: call(L.RENDER_KEEP_PROJECT | L.RENDER_NO_RESOLVE, load_first=load_first))
                row.append(f"plain load before the atomic {'on ' if load_first else 'off'} {ms(tm)}")
            out.append(f"    V = {V}  default max_small = {L.MESH_RENDER_MAX_SMALL}:  " + "   ".join(row))
            del call
            torch.cuda.empty_cache()
        out.append("")

    # the baseline: render_numpy on the host against the kernels on the tests' mesh
    v, t, c = RC.mesh("sphere+plane")
    size = (96, 131)
    Ks, Tc = RC.cameras(*size)
    t0 = time.perf_counter()
    for _ in range(3):
        ref = R.render_numpy(v, t, Ks, Tc, size, colors=c, normals=True, bary=True)
    host_ms = (time.perf_counter() - t0) / 3 * 1e3
    dv, dt, dc = up(v), up(t), up(c)
    small = up(np.stack([R.compose_projection(Kc, T) for Kc, T in zip(Ks, Tc)]).astype(np.float32))
    got = ops.mesh_render(dv, dt, small, size, dc, True, True)
    agree = float(np.mean([np.mean(got["triangle"][i].cpu().numpy() == ref.triangle[i]) for i in range(3)]))
    t_k = timed(lambda: ops.mesh_render(dv, dt, small, size, dc, True, True, check_indices=False))
    out += [f"baseline: the tests' sphere+plane mesh (M = {len(v)}, T = {len(t)}) into three {size[0]} x {size[1]} views with every map: "
            f"render_numpy (float64, this box's CPU) {host_ms:.1f} ms; ops.mesh_render {ms(t_k)} including its allocations; the "
            f"triangle maps agree on {100 * agree:.3f} % of the pixels", ""]
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
