#!/usr/bin/env python3
"""Times vis_mvsnet on the GPU and writes profiles/vis_mvsnet.txt (commit and device name in the header).

  (a) whole frame: ms per frame of model.forward at 768 x 1152 with 4 source views and at 384 x 576 with 2, with the share per part
      (FeatExt, and summed over the three stages: cost volumes, Reg, pair head, UncertNet, fusion, RegFuse, regression, the in-place
      ReLUs of the residual blocks, the torch arithmetic between the stages) from device events recorded through the model's
      measurement hook (VisMvsnet._mark) in the same forwards;
  (b) each of the three kernels the model adds against the stock-torch composition it replaces, in the same process and alternating,
      at the stage-1 and stage-3 shapes of both frames:
        ops.sweep_groupcorr_nhwc  vs  sweep_modes.vis_cost_volumes (its NCHW repack included) + permute(0,2,3,4,1).contiguous() per view
        ops.soft_argmin           vs  torch softmax, index sum, depth, clamp / log entropy sum, window mask sum (blocks/utils.py:51-68)
        ops.vis_fuse              vs  torch exp / mul / add per view and one division (vis_mvsnet_singlestage.py:263-266,302-303)
      after checking that both sides give the same result.

Every shape is warmed up before it is timed; a figure is the median over --repeats windows of device-event time.
Random weights (timing does not depend on them)."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_common as gc  # noqa: E402
import robustmvd_amd as R  # noqa: E402
from robustmvd_amd import ops, sweep_modes as SM  # noqa: E402


def event_ms(fn, warmup, repeats, inner=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def frame(model, H, W, V, warmup, repeats, dev, out):
    s = gc.synthetic_sample(1, H, W, V)
    sample = model.input_adapter(images=[im[None] for im in s["images"]], keyview_idx=np.array([0]), poses=[p[None] for p in s["poses"]],
                                 intrinsics=[k[None] for k in s["intrinsics"]], depth_range=(np.float32(0.5), np.float32(10.0)))
    with torch.no_grad():
        for _ in range(warmup):
            model(**sample)
        torch.cuda.synchronize()
        total, parts = [], {}
        for _ in range(repeats):
            marks = [("start", torch.cuda.Event(enable_timing=True))]
            marks[0][1].record()

            def mark(name):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append((name, e))

            model._mark = mark
            model(**sample)
            model._mark = None
            torch.cuda.synchronize()
            total.append(marks[0][1].elapsed_time(marks[-1][1]))
            one = {}
            for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
                one[name] = one.get(name, 0.0) + e0.elapsed_time(e1)
            # a "relu" mark closes the span that holds the block's layers AND its ReLU: the ReLU alone is timed in (a')
            for name, t in one.items():
                parts.setdefault(name, []).append(t)
        plain, lo, hi = event_ms(lambda: model(**sample), 1, repeats)
    out.append(f"(a) {H} x {W}, {V} source views: {plain:.2f} ms per frame (median of {repeats}; min {lo:.2f}, max {hi:.2f}); "
               f"with the part events {np.median(total):.2f} ms")
    names = {"relu": "Reg/RegFuse blocks", "Reg": "Reg rest + pair conv", "RegFuse": "RegFuse rest + conv"}
    for name, ts in parts.items():
        m = float(np.median(ts))
        out.append(f"      {names.get(name, name):<22s} {m:8.3f} ms  {100 * m / np.median(total):5.1f} %")
    # (a') the in-place ReLUs alone: the passes a residual-before-ReLU epilogue of the 3-D convolution would save
    relu_ms = 0.0
    for i, (D, sc) in enumerate(zip((64, 32, 16), (8, 4, 2))):
        h, w = H // sc, W // sc
        for M in (V, 1):  # Reg over the V pairs, RegFuse over the fused volume
            e0 = torch.randn((M, D, h, w, 8), device=dev)
            e1 = torch.randn((M, D // 2, h // 2, w // 2, 16), device=dev)
            relu_ms += event_ms(lambda: (torch.relu_(e0), torch.relu_(e1)), warmup, repeats, inner=5)[0]
            del e0, e1
    out.append(f"(a') the twelve in-place ReLUs of that frame, timed alone on tensors of their shapes: {relu_ms:.3f} ms = "
               f"{100 * relu_ms / plain:.1f} % of the frame (the known cost of adding the residual outside the convolution kernel)")


def kernels(h, w, D, V, per_pixel, warmup, repeats, dev, out, label):
    B, C, G = 1, 32, 8
    g = torch.Generator(device="cpu").manual_seed(5)
    feats = [torch.randn((B, C, h, w), generator=g).to(dev) for _ in range(V + 1)]
    rng = np.random.default_rng(5)
    K = gc.synthetic_intrinsics(h, w)

    def cam(pose):
        c = np.zeros((1, 2, 4, 4), np.float32)
        c[0, 0], c[0, 1, :3, :3] = pose, K
        return torch.from_numpy(c).to(dev)

    ref_cam, src_cams = cam(np.eye(4, dtype=np.float32)), [cam(gc.synthetic_pose(rng)) for _ in range(V)]
    start = torch.full((B, 1, 1, 1), 0.5, device=dev)
    if per_pixel:
        start = (start * (1 + 0.05 * torch.rand((B, 1, h, w), device=dev))).contiguous()
    interval = torch.full((B, 1, 1, 1), 9.5 / D, device=dev)
    k = torch.arange(D, dtype=torch.float32, device=dev).view(1, D, 1, 1)
    depth = start + interval * k
    depth = depth.expand(B, D, h, w).contiguous() if per_pixel else depth.reshape(B, D)
    Ms = [SM._vis_transform(ref_cam, c) for c in src_cams]
    key = feats[0].permute(0, 2, 3, 1).contiguous()
    srcs = []
    for f in feats[1:]:
        buf = torch.zeros((B, h + 3, w + 3, C), device=dev)
        buf[:, 1:h + 1, 1:w + 1] = f.permute(0, 2, 3, 1)
        srcs.append(buf)
    vol = torch.empty((V * B, D, h, w, G), device=dev)
    new = lambda: ops.sweep_groupcorr_nhwc(key, srcs, Ms, depth, G, pix_offset=0.5, stretch=False, out=vol)
    old = lambda: [c.permute(0, 2, 3, 4, 1).contiguous() for c in SM.vis_cost_volumes(feats[0], ref_cam, feats[1:], src_cams, D, start, interval, G)]
    assert all(torch.equal(a, b) for a, b in zip(new(), old()))

    def versus(what, shape, name_new, f_new, name_old, f_old):
        tn, to = [], []
        for _ in range(3):  # alternate the two sides
            tn.append(event_ms(f_new, warmup, repeats, inner=5)[0])
            to.append(event_ms(f_old, warmup, repeats, inner=5)[0])
        tn, to = float(np.median(tn)), float(np.median(to))
        out.append(f"(b) {label}: {what} {shape}: {name_new} {tn:.3f} ms  vs  {name_old} {to:.3f} ms  ({to / tn:.2f}x)"
                   + ("" if tn <= to else "   <-- the new kernel is SLOWER"))

    versus("cost volumes", f"{V} x (1,{D},{h},{w},8)", "sweep_groupcorr_nhwc", new, "vis_cost_volumes + repack + permute", old)
    del vol

    score = (torch.randn((V * B, D, h, w), device=dev) * 4).contiguous()
    st = start.reshape(B, -1).repeat(V, 1)
    iv = interval.reshape(B).repeat(V)
    idx = torch.arange(D, dtype=torch.float32, device=dev).view(1, D, 1, 1)

    def torch_argmin():
        p = torch.softmax(score, 1)
        o = torch.sum(idx * p, 1, keepdim=True)
        d = o * iv.view(-1, 1, 1, 1) + st.view(V * B, 1, *([1, 1] if st.shape[1] == 1 else [h, w]))
        ent = torch.sum(-p * p.clamp(1e-9, 1.0).log(), 1, keepdim=True)
        prob = torch.sum(p * ((idx - o).abs() <= 2.0).float(), 1, keepdim=True)
        return d[:, 0], ent[:, 0], prob[:, 0]

    d_new, e_new, _ = ops.soft_argmin(score, st, iv, with_entropy=True, window=2.0)
    d_old, e_old, _ = torch_argmin()
    assert torch.allclose(d_new, d_old, atol=1e-5, rtol=1e-5) and torch.allclose(e_new, e_old, atol=1e-5, rtol=1e-5)
    versus("scores", f"({V},{D},{h},{w})", "soft_argmin (depth, entropy, window)", lambda: ops.soft_argmin(score, st, iv, with_entropy=True, window=2.0),
           "torch softmax / sum / entropy / mask chain", torch_argmin)
    del score

    xs = [torch.randn((B, D, h, w, 8), device=dev) for _ in range(V)]
    us = [torch.rand((B, 1, h, w), device=dev) * 6 - 3 for _ in range(V)]

    def torch_fuse():
        wsum = torch.zeros((B, 1, h, w, 1), device=dev)
        fused = torch.zeros((B, D, h, w, 8), device=dev)
        for x, u in zip(xs, us):
            wt = (-u).exp().unsqueeze(-1)
            wsum = wsum + wt
            fused = fused + x * wt
        fused /= wsum
        return fused

    assert torch.allclose(ops.vis_fuse(xs, us), torch_fuse(), atol=1e-5, rtol=1e-5)
    versus("volumes", f"{V} x (1,{D},{h},{w},8)", "vis_fuse", lambda: ops.vis_fuse(xs, us), "torch exp / mul / add / div chain", torch_fuse)


def tree_label():
    """The checkout's commit, with a note when git reports uncommitted changes; `--commit` overrides it where the tree under test
    is a copy without its .git."""
    git = lambda *a: subprocess.run(["git", "-C", ROOT, *a], capture_output=True, text=True)
    head = git("rev-parse", "--short", "HEAD")
    if head.returncode != 0:
        return "unknown (not a git checkout)"
    dirty = git("status", "--porcelain").stdout.strip() != ""
    return head.stdout.strip() + (" + uncommitted changes" if dirty else "")


def main():
    if "--print-commit" in sys.argv:
        print(tree_label())
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vis_mvsnet.txt"))
    ap.add_argument("--commit", default=None, help="commit to name in the header (default: tree_label() of the checkout)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    commit = args.commit or tree_label()
    out = [f"vis_mvsnet on {torch.cuda.get_device_name(0)}; commit {commit}; tools/bench_vis_mvsnet.py "
           f"--warmup {args.warmup} --repeats {args.repeats}", ""]
    torch.manual_seed(0)
    model = R.VisMvsnet().eval().to(dev)
    for H, W, V in ((768, 1152, 4), (384, 576, 2)):
        frame(model, H, W, V, args.warmup, args.repeats, dev, out)
        out.append("")
    for H, W, V in ((768, 1152, 4), (384, 576, 2)):
        kernels(H // 8, W // 8, 64, V, False, args.warmup, args.repeats, dev, out, f"stage 1 of {H} x {W}")
        kernels(H // 2, W // 2, 16, V, True, args.warmup, args.repeats, dev, out, f"stage 3 of {H} x {W}")
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
