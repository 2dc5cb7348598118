#!/usr/bin/env python3
"""conv0 alone on the split-operand kernel, several builds of the library and switches of the experiments library in ONE process,
taken alternately: us per launch over three repeats, and whether the output bits equal the first variant's.  GPU box only.

tools/bench_conv0_variants.py [-c CONFIG ...] NAME=LIBRARY[,SWITCH=VALUE ...] ...
  LIBRARY: `product`, `exp`, or the path of another build (the parent commit's library, an EXPFLAGS build of `make exp`)
  SWITCH:  MVD_CONV0_LEGACY (the six-MFMA schedule), MVD_CONV0_SLOTS (persistent runs), MVD_CONV0_TD (march length): the
           experiments library reads them at every call, a product library ignores them
e.g.  parent=parent_build/libmvd_hip.so new=product six=exp,MVD_CONV0_LEGACY=1 persistent=exp,MVD_CONV0_SLOTS=512 td64=exp,MVD_CONV0_TD=64"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robustmvd_amd import ops, _lib as L  # noqa: E402

CONFIGS = {1: (448, 640, 128), 2: (768, 1152, 256), 3: (896, 1216, 256)}
SWITCHES = ("MVD_CONV0_LEGACY", "MVD_CONV0_SLOTS", "MVD_CONV0_TD")

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("-c", "--config", type=int, action="append", choices=sorted(CONFIGS))
ap.add_argument("variants", nargs="+")
args = ap.parse_args()

variants, libs = [], {}
for v in args.variants:
    name, _, rest = v.partition("=")
    lib, *sw = rest.split(",")
    path = {"product": L.LIB_PATH, "exp": L.EXP_LIB_PATH}.get(lib, lib)
    env = dict(s.split("=", 1) for s in sw)
    if set(env) - set(SWITCHES):
        ap.error(f"{name}: unknown switch {sorted(set(env) - set(SWITCHES))}")
    if path not in libs:
        libs[path] = L._bind(path, skip=L.PRODUCT_ONLY)
    variants.append((name, path, env))

dev = torch.device("cuda:0")
for cfg in args.config or [2]:
    H, W, D = CONFIGS[cfg]
    h, w = H // 4, W // 4
    x = torch.rand(1, D, h, w, 32, device=dev) * 2
    wt = torch.randn(8, 32, 3, 3, 3, device=dev) * 0.05
    sc, sh = torch.rand(8, device=dev) + 0.5, torch.randn(8, device=dev) * 0.1
    amax = ops.absmax(x)
    res, ref = {}, None
    for rep in range(3):
        for name, path, env in variants:
            for k in SWITCHES:
                os.environ.pop(k, None)
            os.environ.update(env)
            L._override = libs[path]
            try:
                wsp = ops.pack_conv3d_weights_split(wt)  # a schedule packs its own fragment layout
                for _ in range(3):
                    y = ops.conv3d_bn_relu_split(x, wsp, sc, sh, relu=True, x_absmax=amax)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    y = ops.conv3d_bn_relu_split(x, wsp, sc, sh, relu=True, x_absmax=amax)
                e1.record()
                torch.cuda.synchronize()
            finally:
                L._override = None
            if ref is None:
                ref = y.clone()
            res.setdefault(name, []).append((e0.elapsed_time(e1) * 100.0, bool(torch.equal(y.view(torch.int32), ref.view(torch.int32)))))
    print(f"== config {cfg}: conv0 {D}x{h}x{w}, us per launch, three alternating repeats; bits = equal to the first variant's output", flush=True)
    for name, v in res.items():
        print(f"  {name:24s} " + "  ".join(f"{t:7.1f}" for t, _ in v) + f"   bits {'equal' if all(s for _, s in v) else 'DIFFER'}", flush=True)
