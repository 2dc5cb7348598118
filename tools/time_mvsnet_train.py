#!/usr/bin/env python3
"""Times one MVSNet training step (forward + backward, B = 1, train mode: BN on batch statistics) at BASELINE configs[1]
(448x640, 2 sources, 128 planes) and configs[2] (768x1152, 4 sources, 256 planes), split by HIP events into
FeatureNet fwd / bwd, K3 fwd / VJP, CostRegNet fwd / bwd and K5 fwd / VJP (the stages are cut at detached tensors, so each
backward runs on its own), next to the unsplit model(**sample) + backward.  Also times K5's VJP kernel against torch autograd of
softmax + depth_regression on the same cost volume, with its rate against 4*B*D*h*w*2 bytes (one read of the cost, one write
of its gradient).  GPU box only.  Usage: python tools/time_mvsnet_train.py [--configs 1 2] [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import gen_common as gc  # noqa: E402
import robustmvd_amd as R  # noqa: E402
from robustmvd_amd import ops  # noqa: E402
from robustmvd_amd.models import _as_batch  # noqa: E402
from robustmvd_amd.registry import add_batch_dim  # noqa: E402

dev = torch.device("cuda:0")
CONFIGS = {1: (448, 640, 2, 128), 2: (768, 1152, 4, 256)}  # H, W, sources, planes (BASELINE.json configs[1], configs[2])


class Events:
    def __init__(self):
        self.marks = []

    def mark(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.marks.append((name, e))

    def spans(self):
        torch.cuda.synchronize()
        return {n1: e0.elapsed_time(e1) for (_, e0), (n1, e1) in zip(self.marks, self.marks[1:])}


def split_step(model, sample):
    """One training step, stage by stage; returns {stage: ms}."""
    model.zero_grad(set_to_none=True)
    n = sample["images"][0].shape[0]
    key_pos = [0] * n
    dv = model.depth_samples(sample["depth_range"], n, dev)
    proj = model.projection_matrices(sample["intrinsics"], sample["poses"], key_pos, dev)
    views, projs = list(sample["images"]), list(proj)
    ev = Events()
    ev.mark("start")
    f = model.feature.forward_autograd(_as_batch(views))
    ev.mark("FeatureNet fwd")
    fd = f.detach().requires_grad_(True)
    feats = list(torch.split(fd, n, 0))
    v = ops.warp_variance_autograd(feats[0], feats[1:], projs[1:], projs[0], dv)
    ev.mark("K3 fwd")
    vd = v.detach().requires_grad_(True)
    c = model.cost_regularization.forward_autograd(vd).squeeze(1)
    ev.mark("CostRegNet fwd")
    cd = c.detach().requires_grad_(True)
    d, _ = ops.softmax_regress_autograd(cd, dv)
    ev.mark("K5 fwd")
    d.backward(torch.ones_like(d))
    ev.mark("K5 VJP")
    c.backward(cd.grad)
    ev.mark("CostRegNet bwd")
    v.backward(vd.grad)
    ev.mark("K3 VJP")
    f.backward(fd.grad)
    ev.mark("FeatureNet bwd")
    return ev.spans()


def full_step(model, sample):
    model.zero_grad(set_to_none=True)
    ev = Events()
    ev.mark("start")
    pred, _ = model(**sample)
    pred["depth"].sum().backward()
    ev.mark("step")
    return ev.spans()["step"]


def k5_vjp_vs_torch(cost, dv, reps, n=50):
    """Per call, averaged over n back-to-back calls between two events: the K5 VJP kernel alone (its C entry point), the
    autograd backward of ops.softmax_regress_autograd (kernel + autograd engine), and torch autograd of softmax +
    depth_regression on the same tensors."""
    from robustmvd_amd import _lib as L
    lib = L.load()
    B, D, h, w = cost.shape
    G = torch.randn(B, h, w, device=dev)
    c1 = cost.detach().clone().requires_grad_(True)
    d1, _ = ops.softmax_regress_autograd(c1, dv)
    c2 = cost.detach().clone().requires_grad_(True)
    d2 = torch.sum(torch.softmax(c2, 1) * dv.view(B, D, 1, 1), 1)
    stats = torch.empty((B, 2, h, w), device=dev)
    depth = torch.empty((B, h, w), device=dev)
    L.check(lib.mvd_softmax_regress_stats_f32(L.ptr(cost), L.ptr(dv), B, D, h, w, L.ptr(depth), None, L.ptr(stats),
                                              L.stream_of(cost)), "stats")
    g_cost = torch.empty_like(cost)

    def kernel():
        lib.mvd_softmax_regress_backward_f32(L.ptr(cost), L.ptr(dv), L.ptr(depth), L.ptr(stats), L.ptr(G), B, D, h, w,
                                             L.ptr(g_cost), L.stream_of(cost))

    def t_of(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            ev = Events()
            ev.mark("a")
            for _ in range(n):
                fn()
            ev.mark("b")
            ts.append(ev.spans()["b"] / n)
        return float(np.median(ts))

    t_kernel = t_of(kernel)
    t_hip = t_of(lambda: torch.autograd.grad(d1, c1, G, retain_graph=True))
    t_torch = t_of(lambda: torch.autograd.grad(d2, c2, G, retain_graph=True))
    nbytes = 4.0 * B * D * h * w * 2
    return {"k5_vjp_kernel_ms": t_kernel, "k5_vjp_kernel_gbs": nbytes / t_kernel / 1e6, "k5_vjp_autograd_ms": t_hip,
            "torch_softmax_regression_bwd_ms": t_torch, "k5_vjp_bytes": nbytes}


def run(cfg, reps, warmup):
    H, W, V, D = CONFIGS[cfg]
    model = R.MVSNet(num_sampling_steps=D).to(dev).train()
    s = gc.synthetic_sample(cfg, H, W, V)
    im, key, po, intr, dr = add_batch_dim(s["images"], 0, s["poses"], s["intrinsics"], (np.float32(0.5), np.float32(10.0)))
    sample = model.input_adapter(images=im, keyview_idx=key, poses=po, intrinsics=intr, depth_range=dr)
    for i in range(warmup):
        split_step(model, sample)
        print(f"  configs[{cfg}] warm-up step {i + 1}/{warmup} done", flush=True)
    runs, fulls = [], []
    for i in range(reps):
        runs.append(split_step(model, sample))
        fulls.append(full_step(model, sample))
        print(f"  configs[{cfg}] timed step {i + 1}/{reps}: split {sum(runs[-1].values()):.1f} ms, full {fulls[-1]:.1f} ms", flush=True)
    stages = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    full = float(np.median(fulls))
    with torch.no_grad():
        cost = torch.randn(1, D, H // 4, W // 4, device=dev) * 3
    dv = model.depth_samples(sample["depth_range"], 1, dev)
    out = {"config": cfg, "H": H, "W": W, "V": V, "D": D, "stages_ms": stages, "sum_of_stages_ms": sum(stages.values()),
           "full_step_ms": full, "peak_mem_gb": torch.cuda.max_memory_allocated() / 1e9}
    out.update(k5_vjp_vs_torch(cost, dv, reps))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    for cfg in a.configs:
        r = run(cfg, a.reps, a.warmup)
        print(f"configs[{cfg}] {r['H']}x{r['W']} V{r['V']} D{r['D']}: training step {r['full_step_ms']:.2f} ms "
              f"(stages sum {r['sum_of_stages_ms']:.2f} ms, peak {r['peak_mem_gb']:.1f} GB)")
        for k, v in r["stages_ms"].items():
            print(f"  {k:16s} {v:9.3f} ms  {100 * v / r['sum_of_stages_ms']:5.1f} %")
        print(f"  K5 VJP kernel {r['k5_vjp_kernel_ms'] * 1e3:.1f} us = {r['k5_vjp_kernel_gbs']:.0f} GB/s of {r['k5_vjp_bytes'] / 1e6:.1f} MB; "
              f"through autograd {r['k5_vjp_autograd_ms'] * 1e3:.1f} us; torch softmax + depth_regression backward "
              f"{r['torch_softmax_regression_bwd_ms'] * 1e3:.1f} us")
        print("JSON " + json.dumps(r), flush=True)
        torch.cuda.empty_cache()
