#!/usr/bin/env python3
"""Two sweeps of the split-operand implicit GEMM's launch plan on the experiments library.  GPU box only.

tools/sweep_conv2d_plan.py [layer ...]: the DispNet layers that the default plan splits, over the output-channel tile per workgroup
and the split of the reduction (MVD_C2_BN / MVD_C2_KSPLIT): us per call incl. the reduce pass.

tools/sweep_conv2d_plan.py persist [layer ...]: the twelve implicit-GEMM layers of the headline forward (FeatureNet conv2 .. feature
on 5 images of 768 x 1152, the regulariser's conv1 .. conv6 on 256 planes of 192 x 288): one tile per workgroup (MVD_C2_PERSIST=0)
against the built-in rule (=1) and fixed persistent grids (=n), and for the 3-D layers the channel tiles MVD_C2_BN.  us per call:
median of REPS repeats of ITERS calls, and the repeats' spread; every form is checked to give the same bits."""
import os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP = os.path.join(ROOT, "robustmvd_amd", "lib_exp", "libmvd_hip_exp.so")
LAYERS = {"conv3_key": "3 2 0 128 256 1 192 288", "conv_redir": "1 1 0 256 32 1 96 144", "conv3_1": "3 1 0 288 256 1 96 144",
          "conv4": "3 2 0 256 512 1 96 144", "conv4_1": "3 1 0 512 512 1 48 72", "conv5": "3 2 0 512 512 1 48 72",
          "conv5_1": "3 1 0 512 512 1 24 36", "conv6": "3 2 0 512 1024 1 24 36", "conv6_1": "3 1 0 1024 1024 1 12 18",
          "deconv_1": "4 2 1 1024 512 1 12 18", "rfeat1": "3 1 0 1026 512 1 24 36", "deconv_2": "4 2 1 512 256 1 24 36",
          "rfeat2": "3 1 0 770 256 1 48 72", "deconv_3": "4 2 1 256 128 1 48 72", "rfeat3": "3 1 0 386 128 1 96 144"}


def sweep_plan(names):
    for name in names or list(LAYERS):
        row = []
        for bn in (128, 64):
            for ks in (1, 2, 4, 8, 16, 32):
                env = dict(os.environ, MVD_ALT_LIB=EXP, MVD_C2_BN=str(bn), MVD_C2_KSPLIT=str(ks))
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_conv2d_layer.py")] + LAYERS[name].split() + ["20", "time"],
                                   env=env, capture_output=True, text=True)
                us = r.stdout.strip().split(")")[-1].split("us")[0].strip() if r.returncode == 0 and "us per call" in r.stdout else "err"
                row.append(f"bn{bn}/k{ks}: {us}")
        print(f"{name:10s} " + "  ".join(row), flush=True)


# ---- the persistent form and the channel tiles of the headline forward's layers, in this process ----------------------------------
ITERS, REPS = 20, 3
# name: (dims, k, stride, cin, cout, shape of the input without channels)
FRAME_LAYERS = {
    "F.conv2": (2, 5, 2, 8, 16, (5, 768, 1152)), "F.conv3": (2, 3, 1, 16, 16, (5, 384, 576)), "F.conv4": (2, 3, 1, 16, 16, (5, 384, 576)),
    "F.conv5": (2, 5, 2, 16, 32, (5, 384, 576)), "F.conv6": (2, 3, 1, 32, 32, (5, 192, 288)), "F.feature": (2, 3, 1, 32, 32, (5, 192, 288)),
    "K4.conv1": (3, 3, 2, 8, 16, (256, 192, 288)), "K4.conv2": (3, 3, 1, 16, 16, (128, 96, 144)), "K4.conv3": (3, 3, 2, 16, 32, (128, 96, 144)),
    "K4.conv4": (3, 3, 1, 32, 32, (64, 48, 72)), "K4.conv5": (3, 3, 2, 32, 64, (64, 48, 72)), "K4.conv6": (3, 3, 1, 64, 64, (32, 24, 36)),
}
GRIDS = ("512", "768", "1024", "1536", "2048")


def timed(fn):
    for _ in range(3):
        fn()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / ITERS * 1e3)
    return statistics.median(out), max(out) - min(out)


def layer_fn(dims, k, stride, cin, cout, shape):
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.rand(*((1,) if dims == 3 else ()), *shape, cin, generator=g).to(dev)
    am = ops.absmax(x)
    if dims == 2:
        wt = (torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5).to(dev)

        def make():  # packing reads MVD_C2_BN too: pack under the same environment as the launch
            wts = ops.pack_conv2d_weights_split(wt, torch.zeros(cout, device=dev), stride=stride)
            slot = torch.zeros(1, device=dev)
            return lambda: ops.conv2d_split(x, am, wts, act=2, out_absmax=slot)
    else:
        wt = (torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (cin * 27)) ** 0.5).to(dev)
        sc, sh = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)

        def make():
            pk = ops.pack_conv3d_weights_igemm(wt, stride - 1)
            slot = torch.zeros(1, device=dev)
            return lambda: ops.conv3d_bn_relu_igemm(x, am, pk, cin, cout, sc, sh, stride - 1, relu=True, return_absmax=True, out_absmax=slot)[0]
    return make


def with_env(make, **env):
    for k_, v in env.items():
        os.environ[k_] = v
    try:
        fn = make()
        ref = fn().clone()
        t, spread = timed(fn)
    finally:
        for k_ in env:
            del os.environ[k_]
    return t, spread, ref


def sweep_persist(names):
    with L.use_experiments_library():
        for name in names or list(FRAME_LAYERS):
            spec = FRAME_LAYERS[name]
            make = layer_fn(*spec)
            t0, s0, ref = with_env(make, MVD_C2_PERSIST="0")
            row = [f"one tile {t0:6.1f} (+-{s0:.1f})"]
            t1, s1, y = with_env(make, MVD_C2_PERSIST="1")
            assert torch.equal(y, ref), name
            row.append(f"rule {t1:6.1f} (+-{s1:.1f})")
            for n in GRIDS:
                t, s, y = with_env(make, MVD_C2_PERSIST=n)
                assert torch.equal(y, ref), (name, n)
                row.append(f"g{n} {t:6.1f}")
            if spec[0] == 3 and spec[4] > 16:
                for bn in ("16", "32", "64"):
                    if int(bn) > spec[4]:
                        continue
                    for pv in ("0", "1"):
                        t, s, y = with_env(make, MVD_C2_BN=bn, MVD_C2_PERSIST=pv)
                        assert torch.equal(y, ref), (name, bn, pv)
                        row.append(f"bn{bn}/p{pv} {t:6.1f}")
            print(f"{name:10s} " + "  ".join(row), flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["persist"]:
        import torch
        sys.path.insert(0, ROOT)
        from robustmvd_amd import ops, _lib as L
        dev = torch.device("cuda:0")
        sweep_persist(sys.argv[2:])
    else:
        sweep_plan(sys.argv[1:])
