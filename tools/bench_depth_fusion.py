#!/usr/bin/env python3
"""Times one key view's depth fusion and writes profiles/depth_fusion.txt (commit and device name in the header).

For 768 x 1152 and 384 x 576 maps of the tests' analytic scene A (plane, occluding patch, depth noise), each with V = 4 and V = 10
source views, in one process on one GPU:
  (a) the consistency kernel (mvd_geo_consistency_f32 into preallocated outputs) and the compaction with colours
      (mvd_compact_points_f32), each as the median over --repeats HIP-event brackets of --inner launches after --warmup brackets;
  (b) a straightforward torch composition of the same definition: per source the projection arithmetic, F.grid_sample(align_corners=
      True) on the depth map and on its validity, boolean tensors; then torch.nonzero and indexing for the points.  Timed the same way;
  (c) fuse_numpy and points_numpy on the host (median of --numpy-repeats);
  (d) the algorithmic bytes of both kernels and the time they would take at the streaming rate bench.py measures
      (measured_stream_gbs: the library's store pass over 2 GiB).  Every bracket launches the same 7-48 MB working set again, so after
      the warm-up the kernels and the torch composition alike read it from the 256 MB Infinity Cache: the shares of the streaming
      rate compare cache-warm launches with an HBM rate and say how far a launch is from that floor, not what HBM delivers.
The torch composition treats a sample as valid when the interpolated validity is above 0.999, so it differs from the definition on
a few pixels next to holes; the tool prints the agreement and refuses a composition that disagrees on more than 0.5 % of the pixels.

Merge mode and normals (profiles/depth_merge.txt, same process, 768 x 1152): the normals kernel (mvd_depth_normals_f32), the merge kernel
(mvd_geo_merge_f32 with colours and normals, all-zero claimed maps: every passing pixel is emitted and runs the second loop, the most
work the kernel can have) at V = 4 and V = 10 next to the plain mvd_geo_consistency_f32 of the same bracket series, and the compaction
with colours and normals (mvd_compact_points_attr_f32) next to mvd_compact_points_f32.  Then the scene level, host clock around whole
calls that end in a device synchronise: DepthFusion(merge=True) over all five views of the V = 4 scene against what served the
purpose before, plain DepthFusion followed by ops.voxel_downsample at a voxel of one pixel's footprint at the median depth, with the
point counts of both."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import fusion_cases as FC  # noqa: E402
from robustmvd_amd import _lib as L  # noqa: E402
from robustmvd_amd import depth_fusion as DF  # noqa: E402
from robustmvd_amd import ops  # noqa: E402
from bench import measured_stream_gbs  # noqa: E402
from bench_vis_mvsnet import event_ms, tree_label  # noqa: E402


def bench_scene(H, W, V):
    """Scene A seen by a key camera and V sources on a ring around it (centres 0.25-0.35 away, rotations of a few hundredths)."""
    rng = np.random.default_rng(V)
    K = FC.intrinsics(H, W)
    Ts = [FC.pose(np.eye(3), (0, 0, 0))]
    for i in range(V):
        a = 2 * np.pi * i / V
        r = 0.25 + 0.1 * rng.random()
        Ts.append(FC.pose(FC.rot_x(0.03 * np.sin(a + 1)) @ FC.rot_y(-0.03 * np.cos(a)), (r * np.cos(a), r * np.sin(a), 0.02 * np.sin(3 * a))))
    depths = [(FC.render(K, T, H, W, patch=True) * (1 + FC.NOISE_SIGMA * rng.standard_normal((H, W)))).astype(np.float32) for T in Ts]
    image = rng.random((3, H, W)).astype(np.float32) * 255
    return K, Ts, depths, image


def torch_consistency(d, srcs, mats, H, W, x, y, min_views, max_err=1.0, max_rel=0.01):
    """The definition from torch ops; mats: (V,24) on the host (python floats in the arithmetic, no device reads)."""
    d_ok = torch.isfinite(d) & (d > 0)
    bits = torch.zeros((H, W), dtype=torch.int64, device=d.device)
    count = torch.zeros((H, W), dtype=torch.int32, device=d.device)
    total = d.clone()
    for s, (m, src) in enumerate(zip(mats.tolist(), srcs)):
        q = [d * (m[3 * i] * x + m[3 * i + 1] * y + m[3 * i + 2]) + m[9 + i] for i in range(3)]
        u, v = q[0] / q[2], q[1] / q[2]
        valid = d_ok & (q[2] > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        grid = torch.stack([u * (2.0 / (W - 1)) - 1, v * (2.0 / (H - 1)) - 1], dim=-1)[None]
        src_ok = (torch.isfinite(src) & (src > 0)).float()
        ds = F.grid_sample(src[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0]
        taps_ok = F.grid_sample(src_ok[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0] > 0.999
        q2 = [ds * (m[12 + 3 * i] * u + m[13 + 3 * i] * v + m[14 + 3 * i]) + m[21 + i] for i in range(3)]
        err = torch.hypot(q2[0] / q2[2] - x, q2[1] / q2[2] - y)
        rel = (q2[2] - d).abs() / d
        ok = valid & taps_ok & (err < max_err) & (rel < max_rel)
        bits |= ok.to(torch.int64) << s
        count += ok
        total = total + torch.where(ok, q2[2], torch.zeros_like(d))
    fused = torch.where(d_ok, total / (count + 1), torch.zeros_like(d))
    return bits, fused, (count >= min_views).to(torch.uint8), count


def torch_points(mask, fused, image, bp):
    """torch.nonzero (row-major) and indexing; bp: the 12 floats of the back-projection, already on the device like the kernel's"""
    idx = torch.nonzero(mask)
    ys, xs = idx[:, 0], idx[:, 1]
    B, c = bp[:9].view(3, 3), bp[9:]
    ray = torch.stack([xs.float(), ys.float(), torch.ones_like(xs, dtype=torch.float32)], dim=1) @ B.T
    return fused[ys, xs][:, None] * ray + c, image[:, ys, xs].T


def numpy_ms(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(1000 * (time.perf_counter() - t0))
    return float(np.median(times))


def host_ms(fn, warmup, repeats):
    """Median (min, max) of a host clock around fn and a device synchronise: for whole calls that read counts back in between."""
    times = []
    for k in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(1000 * (time.perf_counter() - t0))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def merge_rows(args, dev, lib, stream_gbs):
    H, W = 768, 1152
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ms = lambda t: f"{t[0]:8.4f} ms ({t[1]:.4f}, {t[2]:.4f})"
    out = [f"depth fusion, merge mode and normals, {H} x {W} on {torch.cuda.get_device_name(0)}; commit {args.commit or tree_label()}; "
           f"tools/bench_depth_fusion.py --warmup {args.warmup} --repeats {args.repeats} --inner {args.inner}",
           "kernel rows: ms = median (min, max) per launch over HIP-event brackets, cache-warm like profiles/depth_fusion.txt; the plain "
           "kernels are timed again here, next to the new ones", ""]
    for V in (4, 10):
        K, Ts, depths, image = bench_scene(H, W, V)
        mats = up(DF.compose_matrices(K, Ts[0], [K] * V, Ts[1:]).astype(np.float32))
        maps = [up(d) for d in depths]
        bps = [up(DF.compose_backprojection(K, T).astype(np.float32)) for T in Ts]
        rng = np.random.default_rng(100 + V)
        images = [up(rng.random((3, H, W)).astype(np.float32) * 255) for _ in Ts]
        min_views = min(3, V)
        bits = torch.empty((H, W), dtype=torch.uint32, device=dev)
        fused, mask, count = torch.empty((H, W), device=dev), torch.empty((H, W), dtype=torch.uint8, device=dev), torch.empty((H, W), dtype=torch.uint8, device=dev)
        m_rgb, m_nrm = torch.empty((3, H, W), device=dev), torch.empty((3, H, W), device=dev)
        normals = [torch.empty((3, H, W), device=dev) for _ in Ts]
        key_claimed = torch.zeros((H, W), dtype=torch.uint8, device=dev)
        src_claimed = [torch.zeros((H, W), dtype=torch.uint8, device=dev) for _ in range(V)]
        xyz, rgb, nrm = (torch.empty((H * W, 3), device=dev) for _ in range(3))
        m_dev = torch.empty(1, dtype=torch.int64, device=dev)
        ws_bytes = lib.mvd_compact_points_workspace_bytes(H, W)
        ws = ops.workspace(ws_bytes, dev)

        def k_normals():
            ops.call("mvd_depth_normals_f32", dev, maps[0], bps[0], H, W, normals[0])

        def k_plain():
            ops.call("mvd_geo_consistency_f32", dev, maps[0], maps[1:], mats, None, V, H, W, 1.0, 0.01, min_views, 0.0, bits, fused, mask, count)

        def k_merge():
            ops.call("mvd_geo_merge_f32", dev, maps[0], maps[1:], mats, None, V, H, W, 1.0, 0.01, min_views, 0.0, key_claimed, src_claimed,
                     images[0], images[1:], normals[0], normals[1:], bits, fused, mask, count, m_rgb, m_nrm)

        def k_merge_claims_only():
            ops.call("mvd_geo_merge_f32", dev, maps[0], maps[1:], mats, None, V, H, W, 1.0, 0.01, min_views, 0.0, key_claimed, src_claimed,
                     None, None, None, None, bits, fused, mask, count, None, None)

        def k_points():
            ops.call("mvd_compact_points_f32", dev, mask, fused, m_rgb, bps[0], H, W, xyz, rgb, m_dev, ws, int(ws_bytes))

        def k_points_attr():
            ops.call("mvd_compact_points_attr_f32", dev, mask, fused, m_rgb, m_nrm, bps[0], H, W, xyz, rgb, nrm, m_dev, ws, int(ws_bytes))

        for i in range(V + 1):
            ops.call("mvd_depth_normals_f32", dev, maps[i], bps[i], H, W, normals[i])
        k_merge()
        k_points_attr()
        M = int(m_dev.item())
        pairs = int(count.to(torch.int64)[mask.bool()].sum().item())
        t = {name: event_ms(fn, args.warmup, args.repeats, args.inner)
             for name, fn in (("plain", k_plain), ("merge", k_merge), ("claims", k_merge_claims_only), ("plain2", k_plain),
                              ("normals", k_normals), ("points", k_points), ("attr", k_points_attr))}
        plain = min(t["plain"][0], t["plain2"][0])
        bytes_n = (4 + 12) * H * W
        out += [f"V = {V}: {M} of {H * W} pixels emitted (all-zero claimed maps), {pairs} consistent pairs of emitted pixels",
                f"  mvd_geo_consistency_f32                {ms(t['plain'])}   again after the merge rows {ms(t['plain2'])}",
                f"  mvd_geo_merge_f32, claims only         {ms(t['claims'])}   {t['claims'][0] / plain:5.2f}x the plain kernel",
                f"  mvd_geo_merge_f32, colours + normals   {ms(t['merge'])}   {t['merge'][0] / plain:5.2f}x the plain kernel",
                f"  mvd_depth_normals_f32 (one view)       {ms(t['normals'])}   bytes {bytes_n / 1e6:.2f} MB = {bytes_n / stream_gbs * 1e-6:.4f} ms at the "
                f"streaming rate of {stream_gbs:.0f} GB/s",
                f"  mvd_compact_points_f32 (colours)       {ms(t['points'])}",
                f"  mvd_compact_points_attr_f32 (+normals) {ms(t['attr'])}   {t['attr'][0] / t['points'][0]:5.2f}x", ""]
        if V == 4:
            voxel = float(np.median(depths[0][depths[0] > 0]) / K[0, 0])
            Ks = [K] * (V + 1)
            res = {}

            def scene_merge():
                res["merge"] = DF.DepthFusion(merge=True, normals=True)(maps, Ks, Ts, images=images)

            def scene_merge_no_normals():
                res["merge_c"] = DF.DepthFusion(merge=True)(maps, Ks, Ts, images=images)

            def scene_plain():
                res["plain"] = DF.DepthFusion()(maps, Ks, Ts, images=images)

            def scene_voxel():
                r = DF.DepthFusion()(maps, Ks, Ts, images=images)
                res["voxel"] = ops.voxel_downsample(r.points, voxel, r.colors)

            s = {name: host_ms(fn, args.warmup, args.repeats) for name, fn in (("plain", scene_plain), ("voxel", scene_voxel),
                                                                               ("merge_c", scene_merge_no_normals), ("merge", scene_merge))}
            ms3 = lambda t: f"{t[0]:8.3f} ms ({t[1]:.3f}, {t[2]:.3f})"
            scene_rows = [f"scene level, {V + 1} views, every view against the other {V}; host clock around the whole call and a synchronise, median (min, max) "
                          f"of {args.repeats}:",
                          f"  DepthFusion()                                   {ms3(s['plain'])}   {len(res['plain'].points)} points",
                          f"  DepthFusion() + ops.voxel_downsample({voxel:.5f})  {ms3(s['voxel'])}   {len(res['voxel'][0])} points (voxel = median depth / fx, "
                          "one pixel's footprint)",
                          f"  DepthFusion(merge=True)                         {ms3(s['merge_c'])}   {len(res['merge_c'].points)} points",
                          f"  DepthFusion(merge=True, normals=True)           {ms3(s['merge'])}   {len(res['merge'].points)} points, "
                          f"{int((res['merge'].normals != 0).any(1).sum())} with a valid normal", ""]
    return out + scene_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10, help="launches per HIP-event bracket")
    ap.add_argument("--numpy-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_fusion.txt"))
    ap.add_argument("--merge-out", default=os.path.join(ROOT, "profiles", "depth_merge.txt"))
    ap.add_argument("--commit", default=None, help="commit to name in the header (default: the checkout's)")
    args = ap.parse_args()
    assert args.repeats >= 20, "the figures are medians of at least 20 brackets"
    dev = torch.device("cuda:0")
    lib = L.load()
    stream_gbs = measured_stream_gbs(dev, lib)
    out = [f"depth fusion of one key view on {torch.cuda.get_device_name(0)}; commit {args.commit or tree_label()}; "
           f"tools/bench_depth_fusion.py --warmup {args.warmup} --repeats {args.repeats} --inner {args.inner} "
           f"--numpy-repeats {args.numpy_repeats}",
           f"streaming rate (bench.py measured_stream_gbs, HBM stores over 2 GiB): {stream_gbs:.0f} GB/s; ms = median (min, max) per launch; "
           "all launches cache-warm (the working set of 7-48 MB stays in the 256 MB Infinity Cache between launches)", ""]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    all_faster = True
    for H, W in ((768, 1152), (384, 576)):
        for V in (4, 10):
            K, Ts, depths, image = bench_scene(H, W, V)
            mats = DF.compose_matrices(K, Ts[0], [K] * V, Ts[1:]).astype(np.float32)
            bp = DF.compose_backprojection(K, Ts[0]).astype(np.float32)
            d, srcs, img, t_mats, t_bp = up(depths[0]), [up(s) for s in depths[1:]], up(image), up(mats), up(bp)
            min_views = min(3, V)
            bits = torch.empty((H, W), dtype=torch.uint32, device=dev)
            fused = torch.empty((H, W), dtype=torch.float32, device=dev)
            mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
            count = torch.empty((H, W), dtype=torch.uint8, device=dev)
            xyz, rgb = torch.empty((H * W, 3), device=dev), torch.empty((H * W, 3), device=dev)
            m_dev = torch.empty(1, dtype=torch.int64, device=dev)
            ws_bytes = lib.mvd_compact_points_workspace_bytes(H, W)
            ws = ops.workspace(ws_bytes, dev)

            def kernel_consistency():
                ops.call("mvd_geo_consistency_f32", dev, d, srcs, t_mats, None, V, H, W, 1.0, 0.01, min_views, 0.0, bits, fused, mask, count)

            def kernel_points():
                ops.call("mvd_compact_points_f32", dev, mask, fused, img, t_bp, H, W, xyz, rgb, m_dev, ws, int(ws_bytes))

            y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev),
                                  indexing="ij")
            kernel_consistency()
            kernel_points()
            M = int(m_dev.item())
            tb, tf, tm, tc = torch_consistency(d, srcs, mats, H, W, x, y, min_views)
            agree = float((tm == mask).float().mean())
            assert agree > 0.995, f"the torch composition disagrees with the kernel on {100 * (1 - agree):.2f} % of the masks"
            txyz, trgb = torch_points(mask, fused, img, t_bp)
            assert len(txyz) == M and torch.allclose(txyz, xyz[:M], atol=1e-5) and torch.equal(trgb, rgb[:M])

            k_c = event_ms(kernel_consistency, args.warmup, args.repeats, args.inner)
            k_p = event_ms(kernel_points, args.warmup, args.repeats, args.inner)
            t_c = event_ms(lambda: torch_consistency(d, srcs, mats, H, W, x, y, min_views), args.warmup, args.repeats, args.inner)
            t_p = event_ms(lambda: torch_points(mask, fused, img, t_bp), args.warmup, args.repeats, args.inner)
            r = {}
            n_c = numpy_ms(lambda: r.update(DF.fuse_numpy(depths[0], K, Ts[0], depths[1:], [K] * V, Ts[1:])), args.numpy_repeats)
            n_p = numpy_ms(lambda: DF.points_numpy(r["mask"], r["fused"], K, Ts[0], image), args.numpy_repeats)
            bytes_c = (4 + 4 * V + 4 + 4 + 1 + 1) * H * W          # key, V sources once each, bits, fused, mask, count
            bytes_p = 2 * H * W + 3 * 4 * ((H * W + 255) // 256) + (4 + 12 + 12 + 12) * M  # mask twice, 256-pixel chunk counts, per point
            floor_c, floor_p = bytes_c / stream_gbs * 1e-6, bytes_p / stream_gbs * 1e-6
            all_faster &= k_c[0] < t_c[0] and k_p[0] < t_p[0]
            out += [f"{H} x {W}, V = {V}: {M} of {H * W} pixels pass (min_consistent_views {min_views}); torch composition agrees on "
                    f"{100 * agree:.2f} % of the mask",
                    f"  consistency  kernel {k_c[0]:8.4f} ms ({k_c[1]:.4f}, {k_c[2]:.4f})   torch {t_c[0]:8.3f} ms ({t_c[1]:.3f}, "
                    f"{t_c[2]:.3f})   {t_c[0] / k_c[0]:6.1f}x   numpy {n_c:9.1f} ms   bytes {bytes_c / 1e6:7.2f} MB = {floor_c:.4f} ms at "
                    f"the streaming rate ({100 * floor_c / k_c[0]:.0f} % of it reached)",
                    f"  point cloud  kernel {k_p[0]:8.4f} ms ({k_p[1]:.4f}, {k_p[2]:.4f})   torch {t_p[0]:8.3f} ms ({t_p[1]:.3f}, "
                    f"{t_p[2]:.3f})   {t_p[0] / k_p[0]:6.1f}x   numpy {n_p:9.1f} ms   bytes {bytes_p / 1e6:7.2f} MB = {floor_p:.4f} ms at "
                    f"the streaming rate ({100 * floor_p / k_p[0]:.0f} % of it reached)"]
    out += ["", "every kernel is faster than the torch composition it replaces: " + ("yes" if all_faster else "NO")]
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    text = "\n".join(merge_rows(args, dev, lib, stream_gbs)) + "\n"
    print(text)
    with open(args.merge_out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
