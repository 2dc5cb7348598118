#!/usr/bin/env python3
"""Generate tests/golden/g16_cvp_mvsnet.npz (case a) and g16_cvp_mvsnet_b.npz (case b): whole forwards of the REFERENCE's own
CVPMVSNet (rmvd/models/cvp_mvsnet.py) on the CPU in fp32, with every intermediate the tests compare.

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_cvp.py

The reference is loaded as in make_golden_sweep_grads.py (load_reference(), Tensor.cuda patched to the identity, _load of the two
cvp files) with two more stand-ins this image needs: an `easydict` module with an attribute-dict EasyDict, and torch.range wrapped so
that it accepts one-element tensors (float() on its three arguments).

  case a   B 1, 64 x 96, 2 source views, range 2 .. 10      (torch.range yields 48 coarse hypotheses: asserted)
  case b   B 2, 64 x 64, 2 source views, range 425 .. 935   (also 48), the two batch elements with different images and poses
           (calDepthHypo loops over the batch).  The reference cannot run ONE source view: calDepthHypo's `.squeeze(1)` drops the
           view axis of a (B,1,3,3) tensor and its `[batch][0]` then takes a matrix ROW (IndexError, cvp_mvsnet_components.py:282-323).

Weights: tests/test_cvp_mvsnet_cpu.py::cvp_state_dict from a seed and three gains; only those are stored.  Images are integer-valued
0 .. 255 (stored as uint8) and enter the model as image / 255 in float32.  Every source pose has a rotation (with a pure x translation
calDepthHypo's 2x2 systems are singular) and a baseline large enough for the schedule's intervals to stay a fraction of the depth
(with a short baseline they exceed it, hypotheses go behind the camera and the network turns chaotic: condition 2 fails).

The seeds and gains must make the tests sensitive and stable; three conditions are asserted here:
  1. the level-0 uncertainty has a 5th .. 95th percentile span >= 0.2 (a flat softmax would hide errors);
  2. the same model in float64 (.double(), same inputs): every level's fp32 depth within relative 1e-4 of the float64 one (ten times
     inside the tests' gate, which therefore measures the kernels and not chaos in the network); the maximum is stored as
     ref_f32_vs_f64_rel;
  3. index_f64, the level-0 expected index sum_d p_d d of the float64 run, lies within 1e-3 of an integer for at most 1 % of the
     pixels (those may be excluded from the uncertainty comparison: the 4-bin window jumps there).

Stored per case: images (uint8), poses, intrinsics (views, N, ...), depth_range, depth_0 .. depth_4, hypos_0 .. hypos_4, uncertainty,
index_f64, ref_f32_vs_f64_rel, the weights' seed and gains, the state-dict keys and shapes, and the five regulariser outputs reg_0 ..
reg_4 (forward hook on cost_reg_refine), which the whole-model test compares level by level.  Case a also stores the reference's cost
volumes of the coarse level and of level 3 (cost_4, cost_3) for the regulariser-alone test; its level-0 volume is 3 MB, more than a
committed file may hold, so a third, smaller case provides a level-0 volume:

  case c   B 1, 32 x 64, 2 source views, range 2 .. 10: g16_cvp_mvsnet_c.npz holds only cost_0 (1,16,8,32,64) and reg_0 of that forward
           (and the weights' seed and gains); the three conditions are not asserted for it, it feeds the regulariser alone.

Arrays, seeds and names only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_loader import load_reference, _load, _mod, REF_ROOT  # noqa: E402
import gen_common as gc  # noqa: E402
from test_cvp_mvsnet_cpu import cvp_state_dict  # noqa: E402

WEIGHTS_SEED = 16000
GAINS = dict(gain_feat=1.0, gain_reg=1.0, gain_prob=5.0)
CASES = {
    "a": dict(file="g16_cvp_mvsnet.npz", B=1, H=64, W=96, V=2, depth_range=(2.0, 10.0), seed=16100, trans_sigma=1.0),
    "b": dict(file="g16_cvp_mvsnet_b.npz", B=2, H=64, W=64, V=2, depth_range=(425.0, 935.0), seed=16200, trans_sigma=200.0),
    "c": dict(file="g16_cvp_mvsnet_c.npz", B=1, H=32, W=64, V=2, depth_range=(2.0, 10.0), seed=16300, trans_sigma=1.0),
}


def load_cvp():
    load_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self

    class EasyDict(dict):
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__

    _mod("easydict", EasyDict=EasyDict)
    _range = torch.range
    torch.range = lambda start, end, step=1, **kw: _range(float(start), float(end), float(step), **kw)
    _load("rmvd.models.blocks.cvp_mvsnet_components", "rmvd/models/blocks/cvp_mvsnet_components.py")
    return _load("rmvd.models.cvp_mvsnet", "rmvd/models/cvp_mvsnet.py")


def inputs(cfg):
    B, H, W, V = cfg["B"], cfg["H"], cfg["W"], cfg["V"]
    rng = np.random.default_rng(cfg["seed"])
    images = rng.integers(0, 256, (V + 1, B, 3, H, W), dtype=np.uint8)
    K = np.broadcast_to(gc.synthetic_intrinsics(H, W), (V + 1, B, 3, 3)).copy()
    poses = np.broadcast_to(np.eye(4, dtype=np.float32), (V + 1, B, 4, 4)).copy()
    for v in range(1, V + 1):
        for b in range(B):
            poses[v, b] = gc.synthetic_pose(rng, rot_sigma=0.05, trans_sigma=cfg["trans_sigma"])
    return images, poses, K


def run(mod, cfg, sd, dtype):
    """One forward of the reference model in `dtype` -> dict of recorded arrays."""
    images, poses, K = inputs(cfg)
    model = mod.CVPMVSNet(num_sampling_steps=192).eval()
    full = model.state_dict()
    for k, v in sd.items():
        full[k] = torch.from_numpy(v)
    model.load_state_dict(full, strict=True)
    model = model.to(dtype)
    rec = {"hypos": [], "cost": [], "reg": []}
    cal, sweep = mod.calDepthHypo, mod.calSweepingDepthHypo

    def keep(fn):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            rec["hypos"].append(out.detach().clone())
            return out
        return wrapped

    mod.calDepthHypo, mod.calSweepingDepthHypo = keep(cal), keep(sweep)
    # float64 run: homo_warping / proj_cost build their pixel grids with an explicit float32 dtype and torch.matmul refuses mixed
    # operands; promote them (the grids hold small integers: exact)
    matmul = torch.matmul
    if dtype == torch.float64:
        torch.matmul = lambda a, b: matmul(a.to(dtype), b.to(dtype))
    hook = model.cost_reg_refine.register_forward_hook(
        lambda m, i, o: (rec["cost"].append(i[0].detach().clone()), rec["reg"].append(o.detach().clone())) and None)
    try:
        with torch.no_grad():
            img = [(torch.from_numpy(im).float() / torch.full((1,), 255.0)).to(dtype) for im in images]
            lo, hi = cfg["depth_range"]
            pred, _ = model(images=img, poses=[torch.from_numpy(p).to(dtype) for p in poses],
                            intrinsics=[torch.from_numpy(k).to(dtype) for k in K], keyview_idx=0,
                            depth_range=[torch.tensor([lo], dtype=torch.float32), torch.tensor([hi], dtype=torch.float32)])
    finally:
        mod.calDepthHypo, mod.calSweepingDepthHypo = cal, sweep
        torch.matmul = matmul
        hook.remove()
    assert len(rec["hypos"]) == 5 and len(rec["reg"]) == 5
    assert rec["hypos"][0].shape[1] == 48, f"torch.range gave {rec['hypos'][0].shape[1]} coarse hypotheses"
    out = {"images": images, "poses": poses, "intrinsics": K, "depth_range": np.array(cfg["depth_range"], np.float32)}
    # the forward's five levels, coarse first: level 4, 3, .. 0
    for i, level in enumerate(range(4, -1, -1)):
        hyp, reg = rec["hypos"][i], rec["reg"][i]
        p = torch.softmax(reg, 1)
        depth = (p * (hyp.view(*hyp.shape, 1, 1) if hyp.dim() == 2 else hyp)).sum(1)
        out[f"depth_{level}"] = depth.numpy()
        out[f"hypos_{level}"] = hyp.numpy()
        out[f"cost_{level}"] = rec["cost"][i].numpy()
        out[f"reg_{level}"] = reg.numpy()
    assert np.array_equal(out["depth_0"], pred["depth"][:, 0].numpy())
    out["uncertainty"] = pred["depth_uncertainty"][:, 0].numpy()
    idx = torch.arange(p.shape[1], dtype=p.dtype).view(1, -1, 1, 1)
    out["index"] = (p * idx).sum(1).numpy()
    return out


def main():
    torch.set_num_threads(8)
    mod = load_cvp()
    for name, cfg in CASES.items():
        shapes = {k: tuple(v.shape) for k, v in mod.CVPMVSNet().state_dict().items()}
        sd = cvp_state_dict(shapes, WEIGHTS_SEED, **GAINS)
        r32 = run(mod, cfg, sd, torch.float32)
        if name == "c":  # level-0 cost volume and regulariser output only
            path = os.path.join(HERE, cfg["file"])
            np.savez_compressed(path, weights_seed=np.int64(WEIGHTS_SEED), **{k: np.float64(v) for k, v in GAINS.items()},
                                cost_0=r32["cost_0"], reg_0=r32["reg_0"])
            print(f"{cfg['file']}  {os.path.getsize(path) / 1e6:.2f} MB  (reference: {REF_ROOT})")
            continue
        r64 = run(mod, cfg, sd, torch.float64)
        rel = max(float(np.max(np.abs(r32[f"depth_{l}"] - r64[f"depth_{l}"]) / np.abs(r64[f"depth_{l}"]))) for l in range(5))
        unc = r32["uncertainty"]
        span = float(np.percentile(unc, 95) - np.percentile(unc, 5))
        near = float(np.mean(np.abs(r64["index"] - np.round(r64["index"])) < 1e-3))
        print(f"case {name}: f32 vs f64 depth rel {rel:.3e}; uncertainty 5..95 span {span:.3f}; index within 1e-3 of an integer {near:.4f}; "
              f"depth_0 {r32['depth_0'].min():.3f} .. {r32['depth_0'].max():.3f}")
        if "--dry" in sys.argv:  # print the three figures only (for choosing seeds and gains)
            continue
        assert span >= 0.2, "condition 1: the level-0 softmax is too flat or saturated"
        assert rel <= 1e-4, "condition 2: the network amplifies fp32 rounding beyond 1e-4"
        assert near <= 0.01, "condition 3: too many pixels sit on a window jump"
        keys = sorted(shapes)
        out = {"weights_seed": np.int64(WEIGHTS_SEED), **{k: np.float64(v) for k, v in GAINS.items()},
               "state_dict_keys": np.array(keys), "state_dict_shapes": np.array([list(shapes[k]) + [0] * (5 - len(shapes[k])) for k in keys], np.int64),
               "ref_f32_vs_f64_rel": np.float64(rel), "index_f64": r64["index"].astype(np.float64), "uncertainty": unc}
        for k in ("images", "poses", "intrinsics", "depth_range"):
            out[k] = r32[k]
        for l in range(5):
            out[f"depth_{l}"], out[f"hypos_{l}"], out[f"reg_{l}"] = r32[f"depth_{l}"], r32[f"hypos_{l}"], r32[f"reg_{l}"]
        if name == "a":
            out["cost_4"], out["cost_3"] = r32["cost_4"], r32["cost_3"]
        path = os.path.join(HERE, cfg["file"])
        np.savez_compressed(path, **out)
        print(f"{cfg['file']}  {os.path.getsize(path) / 1e6:.2f} MB  (reference: {REF_ROOT})")


if __name__ == "__main__":
    main()
