#!/usr/bin/env python3
"""Times one MVSNet training step (forward + backward, B = 1, train mode: BN on batch statistics) at BASELINE configs[1]
(448x640, 2 sources, 128 planes) and configs[2] (768x1152, 4 sources, 256 planes), split by HIP events into
FeatureNet fwd / bwd, K3 fwd / VJP, CostRegNet fwd / bwd and K5 fwd / VJP (the stages are cut at detached tensors, so each
backward runs on its own), next to the unsplit model(**sample) + backward.  Also times K5's VJP kernel against torch autograd of
softmax + depth_regression on the same cost volume, with its rate against 4*B*D*h*w*2 bytes (one read of the cost, one write
of its gradient).  --regulariser engine runs CostRegNet's convolutions on the engine in both directions
(MVSNet(train_regulariser="engine")) and splits `CostRegNet bwd` into data-gradient, weight-gradient and BN / elementwise time
(events around the two engine calls inside the backward; the rest is torch's BatchNorm, ReLU and add backward), with the
weight-gradient kernels' rate against the fp32-matrix peak (157 TFLOP/s) and HBM bandwidth (8 TB/s) for their bytes.
--sweep-backward gather runs K3's VJP as the fixed-order gather (MVSNet(sweep_backward="gather")) and splits `K3 VJP` into its
stage A (means, key gradient, window check), stage B (the gather) and fallback (scatter of flagged views) kernels, timed by
torch.profiler over one more K3 backward after the timed steps; it also prints the model's fallback counter.
GPU box only.  Usage: python tools/time_mvsnet_train.py [--configs 1 2] [--reps 5] [--warmup 2] [--regulariser vendor|engine]
[--sweep-backward atomic|gather]"""
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


class BackwardSplit:
    """Events around ops._conv3d_blocked (data gradient) and ops.conv3d_weight_grad inside the regulariser's backward."""

    def __init__(self):
        self.spans = {"data": [], "weight": []}
        self.on = False
        self._blocked, self._wgrad = ops._conv3d_blocked, ops.conv3d_weight_grad
        ops._conv3d_blocked = self._timed("data", self._blocked)
        ops.conv3d_weight_grad = self._timed("weight", self._wgrad)

    def _timed(self, kind, fn):
        def wrapper(*args):
            if not self.on:
                return fn(*args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args)
            e1.record()
            self.spans[kind].append((e0, e1))
            return out
        return wrapper

    def take(self):
        torch.cuda.synchronize()
        out = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self.spans.items()}
        self.spans = {"data": [], "weight": []}
        return out


SPLIT = BackwardSplit()


def weight_grad_work(model, D, h, w):
    """(FLOPs, bytes) of the eleven weight-gradient reductions at a (D,h,w) cost volume: 2 * 27 * Cin * Cout per voxel of the
    smaller of the layer's two tensors; bytes = one read of the layer's input and of its output gradient."""
    from robustmvd_amd.blocks import CostRegNet
    flops = nbytes = 0
    lvl = 1
    for _, cin, cout, stride in CostRegNet.LAYERS + [("prob", 8, 1, 1)]:
        vin = (D // lvl) * (h // lvl) * (w // lvl)
        lvl *= stride
        vout = (D // lvl) * (h // lvl) * (w // lvl)
        flops += 2 * 27 * cin * cout * vout
        nbytes += 4 * (vin * cin + vout * cout)
    lvl = 8
    for _, cin, cout in CostRegNet.UPS:
        vin = (D // lvl) * (h // lvl) * (w // lvl)
        lvl //= 2
        vout = (D // lvl) * (h // lvl) * (w // lvl)
        flops += 2 * 27 * cin * cout * vin
        nbytes += 4 * (vin * cin + vout * cout)
    return flops, nbytes


def k3_forward(model, feats, projs, dv):
    if model.sweep_backward == "gather":
        return ops.warp_variance_autograd(feats[0], feats[1:], projs[1:], projs[0], dv, backward="gather",
                                          fallback_count=model.sweep_backward_fallbacks)
    return ops.warp_variance_autograd(feats[0], feats[1:], projs[1:], projs[0], dv)


K3_GATHER_KERNELS = {"stage A": "gather_stage_a", "stage B": "gather_stage_b", "fallback": "warp_variance_backward_kernel",
                     "plane inverses": "plane_inverse"}


def k3_vjp_split(model, sample):
    """Device time of the gather VJP's kernels over one K3 backward, by kernel name, from torch.profiler -> {part: ms}."""
    from torch.profiler import ProfilerActivity, profile
    n = sample["images"][0].shape[0]
    dv = model.depth_samples(sample["depth_range"], n, dev)
    proj = model.projection_matrices(sample["intrinsics"], sample["poses"], [0] * n, dev)
    with torch.no_grad():
        f = model.feature.forward_autograd(_as_batch(list(sample["images"])))
    feats = list(torch.split(f.detach().requires_grad_(True), n, 0))
    v = k3_forward(model, feats, list(proj), dv)
    g = torch.randn_like(v)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        v.backward(g)
        torch.cuda.synchronize()
    out = {k: 0.0 for k in K3_GATHER_KERNELS}
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", None)
        if t is None:
            t = getattr(e, "cuda_time_total", 0.0)
        for part, pat in K3_GATHER_KERNELS.items():
            if pat in e.key:
                out[part] += t / 1e3
    return out


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
    v = k3_forward(model, feats, projs, dv)
    ev.mark("K3 fwd")
    vd = v.detach().requires_grad_(True)
    if model.train_regulariser == "engine":
        c = model.cost_regularization.forward_autograd_engine(vd.permute(0, 2, 3, 4, 1).contiguous())
    else:
        c = model.cost_regularization.forward_autograd(vd).squeeze(1)
    ev.mark("CostRegNet fwd")
    cd = c.detach().requires_grad_(True)
    d, _ = ops.softmax_regress_autograd(cd, dv)
    ev.mark("K5 fwd")
    d.backward(torch.ones_like(d))
    ev.mark("K5 VJP")
    SPLIT.on = True
    c.backward(cd.grad)
    SPLIT.on = False
    ev.mark("CostRegNet bwd")
    v.backward(vd.grad)
    ev.mark("K3 VJP")
    f.backward(fd.grad)
    ev.mark("FeatureNet bwd")
    out = ev.spans()
    if model.train_regulariser == "engine":
        sp = SPLIT.take()
        out["bwd data-gradient"], out["bwd weight-gradient"] = sp["data"], sp["weight"]
    return out


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


def run(cfg, reps, warmup, regulariser="vendor", sweep_backward="atomic"):
    H, W, V, D = CONFIGS[cfg]
    model = R.MVSNet(num_sampling_steps=D, train_regulariser=regulariser, sweep_backward=sweep_backward).to(dev).train()
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
    split = {k: stages.pop(k) for k in list(stages) if k.startswith("bwd ")}  # parts of CostRegNet bwd, not stages of their own
    full = float(np.median(fulls))
    with torch.no_grad():
        cost = torch.randn(1, D, H // 4, W // 4, device=dev) * 3
    dv = model.depth_samples(sample["depth_range"], 1, dev)
    out = {"config": cfg, "H": H, "W": W, "V": V, "D": D, "stages_ms": stages, "sum_of_stages_ms": sum(stages.values()),
           "full_step_ms": full, "peak_mem_gb": torch.cuda.max_memory_allocated() / 1e9, "regulariser": regulariser,
           "sweep_backward": sweep_backward}
    if sweep_backward == "gather":
        try:
            out["k3_vjp_split_ms"] = k3_vjp_split(model, sample)
        except Exception as e:  # no profiler in this build of torch: the stage total above still stands
            print(f"  K3 VJP split unavailable: {type(e).__name__}: {e}", flush=True)
        out["sweep_backward_fallbacks"] = int(model.sweep_backward_fallbacks.item())
    if split:
        split["bwd BN / elementwise"] = stages["CostRegNet bwd"] - sum(split.values())
        flops, nbytes = weight_grad_work(model, D, H // 4, W // 4)
        t = split["bwd weight-gradient"] * 1e-3
        out.update({"costregnet_bwd_split_ms": split, "weight_grad_tflops": flops / t / 1e12, "weight_grad_gbs": nbytes / t / 1e9,
                    "weight_grad_flops": flops, "weight_grad_bytes": nbytes})
    out.update(k5_vjp_vs_torch(cost, dv, reps))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--regulariser", choices=["vendor", "engine"], default="vendor")
    ap.add_argument("--sweep-backward", choices=["atomic", "gather"], default="atomic")
    a = ap.parse_args()
    for cfg in a.configs:
        r = run(cfg, a.reps, a.warmup, a.regulariser, a.sweep_backward)
        print(f"configs[{cfg}] {r['H']}x{r['W']} V{r['V']} D{r['D']} regulariser={a.regulariser} sweep_backward={a.sweep_backward}: training step {r['full_step_ms']:.2f} ms "
              f"(stages sum {r['sum_of_stages_ms']:.2f} ms, peak {r['peak_mem_gb']:.1f} GB)")
        for k, v in r["stages_ms"].items():
            print(f"  {k:16s} {v:9.3f} ms  {100 * v / r['sum_of_stages_ms']:5.1f} %")
        for k, v in r.get("k3_vjp_split_ms", {}).items():
            print(f"    K3 VJP {k:15s} {v:9.3f} ms (kernel time, one backward under the profiler)")
        if "sweep_backward_fallbacks" in r:
            print(f"    K3 VJP views that fell back to the atomic scatter, all steps: {r['sweep_backward_fallbacks']}")
        for k, v in r.get("costregnet_bwd_split_ms", {}).items():
            print(f"    {k:22s} {v:9.3f} ms  {100 * v / r['stages_ms']['CostRegNet bwd']:5.1f} % of CostRegNet bwd")
        if "weight_grad_tflops" in r:
            print(f"    weight gradients: {r['weight_grad_flops'] / 1e9:.1f} GFLOP at {r['weight_grad_tflops']:.1f} TFLOP/s = "
                  f"{100 * r['weight_grad_tflops'] / 157:.1f} % of 157 TFLOP/s; {r['weight_grad_bytes'] / 1e6:.0f} MB at "
                  f"{r['weight_grad_gbs']:.0f} GB/s = {100 * r['weight_grad_gbs'] / 8000:.1f} % of 8 TB/s")
        print(f"  K5 VJP kernel {r['k5_vjp_kernel_ms'] * 1e3:.1f} us = {r['k5_vjp_kernel_gbs']:.0f} GB/s of {r['k5_vjp_bytes'] / 1e6:.1f} MB; "
              f"through autograd {r['k5_vjp_autograd_ms'] * 1e3:.1f} us; torch softmax + depth_regression backward "
              f"{r['torch_softmax_regression_bwd_ms'] * 1e3:.1f} us")
        print("JSON " + json.dumps(r), flush=True)
        torch.cuda.empty_cache()
