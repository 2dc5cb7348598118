#!/usr/bin/env python3
"""Times cvp_mvsnet on the GPU and writes profiles/cvp_mvsnet.txt (commit and device name in the header).

  (a) whole frame: ms per frame of model.forward at 768 x 1152 with 4 source views and at 384 x 576 with 2, with a per-stage split
      (pyramid, and per level: hypothesis schedule, cost volume, regulariser, regression) from device events recorded through the
      model's measurement hook (CVPMVSNet._mark) in the same forwards;
  (b) the two kernels the model adds against what they replace on the operators the engine had before, in the same process and
      alternating, at the level-0 and coarse shapes of both frames:
        ops.sweep_reduce_nhwc   vs  sweep_modes.sweep_reduce_inference (its NCHW repack included) + permute(0,2,3,4,1).contiguous()
        ops.softmax_regress_pp  vs  torch softmax + sum + avg_pool3d + gather (cvp_mvsnet.py:210-236 of the reference)
      after checking that both sides give the same result;
  (c) the share of the frame the hypothesis schedule (pure torch) takes.

Every shape is warmed up before it is timed; a figure is the median over --repeats windows of device-event time.
Random weights (timing does not depend on them; depths are then meaningless but finite arithmetic is not required for timing)."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_common as gc  # noqa: E402
import robustmvd_amd as R  # noqa: E402
from robustmvd_amd import _lib as L, ops, sweep_modes as SM  # noqa: E402


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
        total, stages = [], {}
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
            for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
                stages.setdefault(name, []).append(e0.elapsed_time(e1))
        # the same frame without the hook's events, as one window per forward
        plain, lo, hi = event_ms(lambda: model(**sample), 1, repeats)
    out.append(f"(a) {H} x {W}, {V} source views: {plain:.2f} ms per frame (median of {repeats}; min {lo:.2f}, max {hi:.2f}); "
               f"with the stage events {np.median(total):.2f} ms")
    sched = 0.0
    for name, ts in stages.items():
        m = float(np.median(ts))
        out.append(f"      {name:<14s} {m:8.3f} ms  {100 * m / np.median(total):5.1f} %")
        if name.startswith("schedule"):
            sched += m
    share = sched / float(np.median(total))
    out.append(f"(c) hypothesis schedule (pure torch, five levels' calibration included): {sched:.3f} ms = {100 * share:.1f} % of the frame"
               + ("  -> MORE than a tenth: the next kernel to write" if share > 0.1 else "  (under a tenth)"))


def kernels(h, w, D, V, per_pixel, warmup, repeats, dev, out, label):
    B, C = 1, 16
    g = torch.Generator(device="cpu").manual_seed(5)
    feats = [torch.randn((B, C, h, w), generator=g).to(dev) for _ in range(V + 1)]
    K = gc.synthetic_intrinsics(h, w).astype(np.float64)
    K4 = np.vstack([np.hstack([K, np.zeros((3, 1))]), [0, 0, 0, 1]])
    rng = np.random.default_rng(5)
    Ms = [torch.from_numpy((K @ gc.synthetic_pose(rng).astype(np.float64)[:3, :4] @ np.linalg.inv(K4))[None, :3, :4].astype(np.float32)).to(dev)
          for _ in range(V)]
    depth = torch.linspace(0.5, 10.0, D, device=dev)[None]
    if per_pixel:
        depth = (depth[:, :, None, None] * (1 + 0.05 * torch.rand((B, D, h, w), device=dev))).contiguous()
    key = feats[0].permute(0, 2, 3, 1).contiguous()
    srcs = []
    for f in feats[1:]:
        buf = torch.zeros((B, h + 3, w + 3, C), device=dev)
        buf[:, 1:h + 1, 1:w + 1] = f.permute(0, 2, 3, 1)
        srcs.append(buf)
    new = lambda: ops.sweep_reduce_nhwc(key, srcs, Ms, depth, L.REDUCE_VARIANCE_KEYSQ)
    old = lambda: SM.sweep_reduce_inference(feats[0], feats[1:], Ms, depth, L.REDUCE_VARIANCE_KEYSQ).permute(0, 2, 3, 4, 1).contiguous()
    assert torch.equal(new(), old())
    tn, to = [], []
    for _ in range(3):  # alternate the two sides
        tn.append(event_ms(new, warmup, repeats, inner=5)[0])
        to.append(event_ms(old, warmup, repeats, inner=5)[0])
    tn, to = float(np.median(tn)), float(np.median(to))
    out.append(f"(b) {label}: cost volume (1,{D},{h},{w},16), {V} sources: sweep_reduce_nhwc {tn:.3f} ms  vs  sweep_reduce + repack + permute {to:.3f} ms"
               f"  ({to / tn:.2f}x)" + ("" if tn <= to else "   <-- the new kernel is SLOWER"))

    cost = (torch.randn((B, D, h, w), device=dev) * 4).contiguous()
    hyp = depth if per_pixel else depth[:, :, None, None].expand(B, D, h, w).contiguous()

    def torch_side():
        p = F.softmax(cost, dim=1)
        d = torch.sum(p * hyp, 1)
        s4 = 4 * F.avg_pool3d(F.pad(p.unsqueeze(1), pad=(0, 0, 0, 0, 1, 2)), (4, 1, 1), stride=1, padding=0).squeeze(1)
        idx = torch.sum(p * torch.arange(D, device=dev, dtype=torch.float32).view(1, D, 1, 1), 1).long()
        return d, torch.gather(s4, 1, idx.unsqueeze(1)).squeeze(1)

    d_new, _ = ops.softmax_regress_pp(cost, hyp)
    assert torch.allclose(d_new, torch_side()[0], atol=1e-5, rtol=1e-5)
    tn, to = [], []
    for _ in range(3):
        tn.append(event_ms(lambda: ops.softmax_regress_pp(cost, hyp), warmup, repeats, inner=5)[0])
        to.append(event_ms(torch_side, warmup, repeats, inner=5)[0])
    tn, to = float(np.median(tn)), float(np.median(to))
    out.append(f"(b) {label}: cost (1,{D},{h},{w}): softmax_regress_pp {tn:.3f} ms  vs  torch softmax + sum + avg_pool3d + gather {to:.3f} ms"
               f"  ({to / tn:.2f}x)" + ("" if tn <= to else "   <-- the new kernel is SLOWER"))


def tree_label():
    """The checkout's commit, with a note when git reports uncommitted changes; `--commit` overrides it where the tree under test
    is a copy without its .git (pass this function's answer from the checkout: `python tools/bench_cvp_mvsnet.py --print-commit`)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cvp_mvsnet.txt"))
    ap.add_argument("--commit", default=None, help="commit to name in the header (default: tree_label() of the checkout)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    commit = args.commit or tree_label()
    out = [f"cvp_mvsnet on {torch.cuda.get_device_name(0)}; commit {commit}; tools/bench_cvp_mvsnet.py "
           f"--warmup {args.warmup} --repeats {args.repeats}", ""]
    torch.manual_seed(0)
    model = R.CVPMVSNet().eval().to(dev)
    for H, W, V in ((768, 1152, 4), (384, 576, 2)):
        frame(model, H, W, V, args.warmup, args.repeats, dev, out)
        out.append("")
    for H, W, V in ((768, 1152, 4), (384, 576, 2)):
        kernels(H, W, 8, V, True, args.warmup, args.repeats, dev, out, f"level 0 of {H} x {W}")
        kernels(H // 16, W // 16, 48, V, False, args.warmup, args.repeats, dev, out, f"coarse level of {H} x {W}")
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
