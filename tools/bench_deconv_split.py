#!/usr/bin/env python3
"""K4's transposed layers at a BASELINE config (default configs[2]: 256 planes of 192x288): the split-operand kernel of
csrc/deconv3d_split.hip (ops.deconv3d_bn_relu_split) in each of its built tiles beside the fp32-MFMA kernel (ops.conv3d_bn_relu):
us per layer alone (back-to-back launches; the frame is measured with tools/frame_kernels.py) and the difference of the results.
The tiles are selected with MVD_DS_CFG = 10 NT + MT in the experiments library (`make -C robustmvd_amd/csrc exp`).  GPU box only.
--persist n1,n2,...: then each layer at its shipped tile, one tile per workgroup (MVD_DS_PERSIST=0) and the persistent form on grids
of n workgroups (1 = the product rule; MVD_DS_PERSIST=n), with the layer's own and (--la) its other look-ahead (MVD_DS_LA), taken
alternately, three repeats: us without / with the max |y| by-product.  --only conv9: that layer alone."""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robustmvd_amd import ops, _lib as L
L.use_experiments_library(os.environ.get("MVD_ALT_LIB")).__enter__()  # MVD_ALT_LIB: another build of the library (the product one ignores MVD_DS_CFG)
def _opt(name, default=None):
    """--name value -> value (removed from sys.argv)"""
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


ONLY = _opt("--only")
PERSIST = [a for a in (_opt("--persist") or "").split(",") if a]
ALT_LA = {"conv7": None, "conv9": "1", "conv11": "2"} if "--la" in sys.argv else {}
if "--la" in sys.argv:
    sys.argv.remove("--la")
D, h, w = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (256, 192, 288)
dev = torch.device("cuda:0")
# layer, Cin, Cout, divisor of the input grid, tiles (NT 16-channel tiles per workgroup, MT 16-column tiles per wave)
LAYERS = [("conv7", 64, 32, 8, [(1, 1), (2, 1)]), ("conv9", 32, 16, 4, [(1, 1), (1, 2)]), ("conv11", 16, 8, 2, [(1, 3), (1, 2)])]


def timeit(fn, n=20):
    for _ in range(3):
        y = fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        y = fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3, y


for name, cin, cout, div, tiles in LAYERS:
    if ONLY and name != ONLY:
        continue
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.rand(1, D // div, h // div, w // div, cin, generator=g).to(dev)
    wt = (torch.randn(cin, cout, 3, 3, 3, generator=g) * (2.0 / (cin * 27)) ** 0.5).to(dev)
    sc, sh = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.1).to(dev)
    skip = torch.rand(1, D // div * 2, h // div * 2, w // div * 2, cout, generator=g).to(dev)
    w32, _, _ = ops.pack_conv3d_weights(wt, L.DECONV3D_STRIDE2)
    wsp = ops.pack_deconv3d_weights_split(wt)
    am = ops.absmax(x)
    slot = torch.zeros(1, device=dev)
    t0, y0 = timeit(lambda: ops.conv3d_bn_relu(x, w32, cin, cout, sc, sh, L.DECONV3D_STRIDE2, relu=True, skip=skip))
    print(f"{name:7s} {cin:3d}->{cout:3d} in {D // div}x{h // div}x{w // div}: fp32 MFMA {t0:7.1f} us", flush=True)
    for nt, mt in tiles:
        os.environ["MVD_DS_CFG"] = str(10 * nt + mt)
        t1, y1 = timeit(lambda: ops.deconv3d_bn_relu_split(x, am, wsp, cin, cout, sc, sh, relu=True, skip=skip))
        t2, _ = timeit(lambda: ops.deconv3d_bn_relu_split(x, am, wsp, cin, cout, sc, sh, relu=True, skip=skip, return_absmax=True, out_absmax=slot)[0])
        print(f"        split NT {nt} MT {mt}: {t1:7.1f} us  x{t0 / t1:4.2f}   with max|y| {t2:7.1f} us   "
              f"rel diff {float((y1 - y0).abs().max()) / float(y0.abs().max()):.1e}", flush=True)
    os.environ.pop("MVD_DS_CFG", None)
    if PERSIST:
        plain = lambda: ops.deconv3d_bn_relu_split(x, am, wsp, cin, cout, sc, sh, relu=True, skip=skip)
        vmax = lambda: ops.deconv3d_bn_relu_split(x, am, wsp, cin, cout, sc, sh, relu=True, skip=skip, return_absmax=True, out_absmax=slot)[0]
        os.environ["MVD_DS_PERSIST"] = "0"
        yref = plain()
        forms = [("0", None)] + [(n, la) for n in PERSIST for la in ([None, ALT_LA[name]] if ALT_LA.get(name) else [None])]
        for rep in range(3):
            for n, la in forms:
                os.environ["MVD_DS_PERSIST"] = n
                if la:
                    os.environ["MVD_DS_LA"] = la
                t1, y1 = timeit(plain)
                t2, _ = timeit(vmax)
                os.environ.pop("MVD_DS_LA", None)
                print(f"        repeat {rep} MVD_DS_PERSIST={n:5s} MVD_DS_LA={la or '-'}: {t1:7.1f} us   with max|y| {t2:7.1f} us   "
                      f"same bits {bool(torch.equal(y1.view(torch.int32), yref.view(torch.int32)))}", flush=True)
        os.environ.pop("MVD_DS_PERSIST", None)
