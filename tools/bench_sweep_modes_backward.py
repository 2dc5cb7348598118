#!/usr/bin/env python3
"""Times the VJPs of the sweep consumers (mvd_sweep_reduce_backward_f32, mvd_sweep_warp_backward_f32) with HIP events at
tools/bench_sweep_modes.py's sizes, next to their forward and to torch autograd through a grid_sample restatement of the same
operator on the same GPU in the same process.  Prints one line per case; `> profiles/sweep_modes_backward.txt` keeps them.  GPU only."""
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from robustmvd_amd import _lib as L, ops, sweep_modes as SM  # noqa: E402
from bench_sweep_modes import timed, B, C, h, w, D, V, dev  # noqa: E402


def torch_reduce(key, srcs, Ms, depth, mode, groups, pix_offset, stretch):
    """sweep_reduce in torch: the kernel's positions turned into a grid_sample grid (zero padding, align_corners=False)."""
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32) + pix_offset,
                            torch.arange(w, device=dev, dtype=torch.float32) + pix_offset, indexing="ij")
    xyz = torch.stack((xs, ys, torch.ones_like(xs))).reshape(1, 3, 1, h * w)
    dep = depth.reshape(B, 1, D, -1)
    sx, sy = (w / (w - 1), h / (h - 1)) if stretch else (1.0, 1.0)
    k = key.unsqueeze(2)
    outs, s1, s2 = [], (k * k if mode == L.REDUCE_VARIANCE_KEYSQ else k), k * k
    for s, M in zip(srcs, Ms):
        with torch.no_grad():
            p = (M[:, :, :3] @ xyz.reshape(1, 3, h * w)).unsqueeze(2) * dep + M[:, :, 3].reshape(B, 3, 1, 1)
            ix, iy = p[:, 0] / p[:, 2] * sx - 0.5, p[:, 1] / p[:, 2] * sy - 0.5
            grid = torch.stack(((2 * ix + 1) / w - 1, (2 * iy + 1) / h - 1), -1).reshape(B, D * h, w, 2)
        sv = F.grid_sample(s, grid, mode="bilinear", padding_mode="zeros", align_corners=False).view(B, C, D, h, w)
        if mode == L.REDUCE_GROUPCORR:
            outs.append((k * sv).view(B, groups, C // groups, D, h, w).sum(2))
        else:
            s1, s2 = s1 + sv, s2 + sv * sv
    return outs if mode == L.REDUCE_GROUPCORR else [s2 / (V + 1) - (s1 / (V + 1)) ** 2]


def torch_warp(srcs, K, Ts, invd):
    """the warp-only sweep in torch: pinhole projection of the key pixels' plane points, grid_sample, sampling mask"""
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32) + 0.5, torch.arange(w, device=dev, dtype=torch.float32) + 0.5, indexing="ij")
    Kp = K[0] * torch.tensor([[w], [h], [1.0]], device=dev)
    rays = torch.inverse(Kp) @ torch.stack((xs, ys, torch.ones_like(xs))).reshape(3, -1)
    outs = []
    for s, T in zip(srcs, Ts):
        with torch.no_grad():
            pts = rays.unsqueeze(0) / invd.reshape(-1, 1, 1)                       # (S,3,hw)
            q = Kp @ (T[0, :3, :3] @ pts + T[0, :3, 3:4])
            grid = torch.stack((2 * q[:, 0] / q[:, 2] / w - 1, 2 * q[:, 1] / q[:, 2] / h - 1), -1).reshape(1, D * h, w, 2)
            mask = (F.grid_sample(torch.ones(1, 1, h, w, device=dev), grid, padding_mode="zeros", align_corners=False) >= 0.9999).float()
        sv = F.grid_sample(s, grid, mode="bilinear", padding_mode="zeros", align_corners=False) * mask
        outs.append(sv.view(1, C, D, h, w).transpose(1, 2))
    return outs


def report(name, forward, torch_forward, inputs):
    with torch.no_grad():
        t_fwd = timed(forward)
    outs = forward()
    outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
    cots = [torch.randn_like(o) for o in outs]
    t_bwd = timed(lambda: torch.autograd.grad(outs, inputs, cots, retain_graph=True))
    got = torch.autograd.grad(outs, inputs, cots, retain_graph=True)
    del outs
    touts = torch_forward()
    t_tfwd = timed(torch_forward, n=4)
    t_tbwd = timed(lambda: torch.autograd.grad(touts, inputs, cots, retain_graph=True), n=4)
    want = torch.autograd.grad(touts, inputs, cots)
    err = max(float((a - b).abs().max()) for a, b in zip(got, want))
    print(f"{name:52s} forward {t_fwd:8.3f} ms  VJP {t_bwd:8.3f} ms | torch grid_sample: forward {t_tfwd:8.3f} ms  autograd backward "
          f"{t_tbwd:8.3f} ms | max |grad diff| {err:.2e}")


def main():
    import gen_common as gc
    from test_hip_shapes import mvs_inputs
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    print(f"# python tools/bench_sweep_modes_backward.py   (commit {commit} + working tree; {torch.cuda.get_device_name(0)})")
    print(f"# B{B} C{C} {h}x{w} D{D} V{V}; medians of HIP-event times; VJP = torch.autograd.grad through the engine's Function")
    feats, projs, key_inv, depth = mvs_inputs(B, C, h, w, D, V, seed=3)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ft = [T(f).requires_grad_(True) for f in feats]
    Ms = [T((p @ key_inv)[:, :3, :4].astype(np.float32)) for p in projs]
    dv = T(depth)
    dpp = (dv[:, :, None, None] * (1 + 0.01 * torch.rand(B, D, h, w, device=dev))).contiguous()
    cases = [("sweep_reduce variance, shared planes", dv, L.REDUCE_VARIANCE, dict()),
             ("sweep_reduce variance, per-pixel hypotheses (cvp)", dpp, L.REDUCE_VARIANCE, dict()),
             ("sweep_reduce key-squared aliasing (cvp quirk)", dpp, L.REDUCE_VARIANCE_KEYSQ, dict()),
             ("sweep_reduce group-wise correlation, 8 groups (vis)", dv, L.REDUCE_GROUPCORR, dict(groups=8, pix_offset=0.5, stretch=False))]
    for name, dep, mode, kw in cases:
        report(name, lambda: SM.sweep_reduce(ft[0], ft[1:], Ms, dep, mode, **kw),
               lambda: torch_reduce(ft[0], ft[1:], Ms, dep, mode, kw.get("groups", 1), kw.get("pix_offset", 0.0), kw.get("stretch", True)), ft)
    rng = np.random.default_rng(4)
    K = T((gc.synthetic_intrinsics(h * 4, w * 4) / np.array([[4.0 * w] * 3, [4.0 * h] * 3, [1.0] * 3])).astype(np.float32)[None])
    Ts = [T(gc.synthetic_pose(rng, 0.05, 0.15).astype(np.float32)[None]) for _ in range(V)]
    invd = T((1.0 / np.linspace(10.0, 0.5, D)).astype(np.float32)[None])
    report("sweep_warp (warp-only correlation block)", lambda: ops.sweep_warp_autograd(ft[1:], K, [K] * V, Ts, invd, (h, w))[0],
           lambda: torch_warp(ft[1:], K, Ts, invd), ft[1:])


if __name__ == "__main__":
    main()
