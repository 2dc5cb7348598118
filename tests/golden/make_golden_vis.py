#!/usr/bin/env python3
"""Generate tests/golden/g17_vis_mvsnet.npz (case a), g17_vis_mvsnet_b.npz (case b) and g17_vis_mvsnet_c.npz (case c): whole forwards
of the REFERENCE's own VisMvsnet (rmvd/models/vis_mvsnet.py) on the CPU in fp32 and float64, with every intermediate the tests compare.

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_vis.py   (--dry: print the
conditions' figures only)

The reference is loaded as in make_golden_cvp.py (load_reference(), Tensor.cuda patched to the identity: the model hard-codes
.cuda()) with a stand-in for rmvd.models.wrappers.wrappers.ModelWrappers (nn.Module).  The float64 run needs three casts, because the
reference builds its cameras and pixel grids in float32 and torch refuses mixed operands: get_pixel_grids' result, grid_sample's grid,
and the arguments of get_homographies and homography_warping are cast to the run's dtype.

  case a   B 1, 64 x 64, 2 source views, range 2 .. 10
  case b   B 2, 64 x 128, 2 source views, range 2 .. 10, the two batch elements with different images and poses
  case c   B 1, 32 x 32, 2 source views: only the stage-3 cost volume of pair 0 (1,8,16,16,16) and the Reg -> reg_pair and RegFuse
           outputs of it, for the regulariser-alone test (case a's stage-3 volume, 32 x 32 x 16 x 8, is too large next to the rest)

Weights: tests/test_vis_mvsnet_cpu.py::vis_state_dict from a seed and three gains; only those are stored.  Images are uint8 and enter the
model through the adapter's normalisation (test_vis_mvsnet_cpu.normalise_numpy).

Three conditions are asserted for cases a and b:
  1. sensitivity: the stage-3 uncertainty has a 5th .. 95th percentile span >= 0.2, the stage-3 pair entropies one >= 1, and the
     stage-3 fusion weight of view 0, exp(-u_0) / sum_v exp(-u_v), one >= 0.1;
  2. conditioning: every stage's fp32 depth within relative 1e-4 of the float64 run's (stored as ref_f32_vs_f64_rel);
  3. window jumps: the pixels the probability-map comparison may leave out (test_vis_mvsnet_cpu.window_jump_mask on the float64 run's
     probability volume) are at most 1 % of each stage's.

Stored per case (a, b): images (uint8), poses, intrinsics (views, N, ...), depth_range, depth_1 .. depth_3, prob_map_3, uncertainty,
the stage-3 pair depths, entropies and both heads (pair_depth_3 (V,B,h,w), pair_entropy_3 (V,B,h,w), pair_heads_3 (V,2,B,h,w)),
index_f64 and jump_3 (packed bits) of the float64 run's stage 3, jump_fraction (3), ref_f32_vs_f64_rel, the weights' seed and gains,
the state-dict keys and shapes; case a also cost_1 (pair 0's stage-1 cost volume, (1,8,64,8,8)), reg_pair_1 and reg_fuse_1.
Arrays, seeds and names only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_loader import load_reference, _load, _mod, _pkg, REF_ROOT  # noqa: E402
import gen_common as gc  # noqa: E402
from test_vis_mvsnet_cpu import normalise_numpy, vis_state_dict, window_jump_mask  # noqa: E402

WEIGHTS_SEED = 17000
GAINS = dict(gain_final=130.0, gain_feat=4.0, gain_head=3.0)
CASES = {
    "a": dict(file="g17_vis_mvsnet.npz", B=1, H=64, W=64, V=2, depth_range=(2.0, 10.0), seed=17100),
    "b": dict(file="g17_vis_mvsnet_b.npz", B=2, H=64, W=128, V=2, depth_range=(2.0, 10.0), seed=17200),
    "c": dict(file="g17_vis_mvsnet_c.npz", B=1, H=32, W=32, V=2, depth_range=(2.0, 10.0), seed=17300),
}


def load_vis():
    ns = load_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self
    _pkg("rmvd.models.wrappers")
    _mod("rmvd.models.wrappers.wrappers", ModelWrappers=torch.nn.Module)
    for n in ("list_module", "vis_mvsnet_unet_modular", "vis_mvsnet_feature_extractor", "vis_mvsnet_singlestage"):
        _load("rmvd.models.blocks." + n, "rmvd/models/blocks/" + n + ".py")
    return _load("rmvd.models.vis_mvsnet", "rmvd/models/vis_mvsnet.py"), sys.modules["rmvd.models.blocks.vis_mvsnet_singlestage"], ns.blocks_utils


def inputs(cfg):
    B, H, W, V = cfg["B"], cfg["H"], cfg["W"], cfg["V"]
    rng = np.random.default_rng(cfg["seed"])
    images = rng.integers(0, 256, (V + 1, B, 3, H, W), dtype=np.uint8)
    K = np.broadcast_to(gc.synthetic_intrinsics(H, W), (V + 1, B, 3, 3)).copy()
    poses = np.broadcast_to(np.eye(4, dtype=np.float32), (V + 1, B, 4, 4)).copy()
    for v in range(1, V + 1):
        for b in range(B):
            poses[v, b] = gc.synthetic_pose(rng, rot_sigma=0.05, trans_sigma=0.3)
    return images, poses, K


def run(mods, cfg, sd, dtype):
    """One forward of the reference model in `dtype` -> dict of recorded arrays (numpy, in `dtype`)."""
    mod, stage_mod, bu = mods
    images, poses, K = inputs(cfg)
    model = mod.VisMvsnet(num_sampling_steps=192).eval()
    full = model.state_dict()
    for k, v in sd.items():
        full[k] = torch.from_numpy(v)
    model.load_state_dict(full, strict=True)
    model = model.to(dtype)
    cast = lambda a: a.to(dtype) if isinstance(a, torch.Tensor) and a.is_floating_point() else a
    saved = (bu.get_pixel_grids, stage_mod.get_homographies, stage_mod.homography_warping, bu.F.grid_sample)
    grids, homs, warp, sample = saved
    bu.get_pixel_grids = lambda *a: cast(grids(*a))
    stage_mod.get_homographies = lambda *a, **k: homs(*[cast(x) for x in a], **k)
    stage_mod.homography_warping = lambda *a: warp(*[cast(x) for x in a])
    bu.F.grid_sample = lambda inp, grid, **k: sample(inp, grid.to(inp.dtype), **k)
    rec = {s: {"cost": [], "interm": [], "entropy": [], "heads": [], "score": []} for s in (1, 2, 3)}
    hooks = []
    for s in (1, 2, 3):
        st = getattr(model, f"stage{s}")
        r = rec[s]
        hooks.append(st.reg.register_forward_hook(lambda m, i, o, r=r: (r["cost"].append(i[0].detach().clone()), r["interm"].append(o.detach().clone())) and None))
        hooks.append(st.uncert_net.register_forward_hook(
            lambda m, i, o, r=r: (r["entropy"].append(i[0].detach().clone()), r["heads"].append([h.detach().clone() for h in o])) and None))
        hooks.append(st.reg_fuse.register_forward_hook(lambda m, i, o, r=r: r["score"].append(o.detach().clone()) and None))
    try:
        with torch.no_grad():
            img = [torch.from_numpy(normalise_numpy(im)).to(dtype) for im in images]
            lo, hi = cfg["depth_range"]
            pred, aux = model(images=img, poses=[torch.from_numpy(p) for p in poses], intrinsics=[torch.from_numpy(k) for k in K],
                              keyview_idx=0, depth_range=[torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)])
            out = {"images": images, "poses": poses, "intrinsics": K, "depth_range": np.array(cfg["depth_range"], np.float32)}
            for s in (1, 2, 3):
                est, pairs = aux["outputs"][s - 1]
                out[f"depth_{s}"] = est[:, 0].numpy()
                p = torch.softmax(rec[s]["score"][0][:, 0].double(), 1).numpy()
                out[f"index_{s}"], out[f"jump_{s}"] = window_jump_mask(p)
            out["prob_map_3"] = aux["prob_maps"][2][:, 0].numpy()
            out["uncertainty"] = pred["depth_uncertainty"][:, 0].numpy()
            assert np.array_equal(pred["depth"].numpy(), aux["outputs"][2][0].numpy())
            _, pairs = aux["outputs"][2]
            out["pair_depth_3"] = np.stack([pd[:, 0].numpy() for pd, _ in pairs])
            out["pair_heads_3"] = np.stack([np.stack([h[:, 0].numpy() for h in heads]) for _, heads in pairs])
            out["pair_entropy_3"] = np.stack([e[:, 0].numpy() for e in rec[3]["entropy"]])
            for s in (1, 3):  # regulariser alone: pair 0's cost volume through Reg -> reg_pair and through RegFuse
                st = getattr(model, f"stage{s}")
                cost = rec[s]["cost"][0]
                out[f"cost_{s}"] = cost.numpy()
                out[f"reg_pair_{s}"] = st.reg_pair(st.reg(cost)).numpy()
                out[f"reg_fuse_{s}"] = st.reg_fuse(cost).numpy()
    finally:
        bu.get_pixel_grids, stage_mod.get_homographies, stage_mod.homography_warping, bu.F.grid_sample = saved
        for h in hooks:
            h.remove()
    return out


def main():
    torch.set_num_threads(8)
    mods = load_vis()
    pct = lambda x: float(np.percentile(x, 95) - np.percentile(x, 5))
    for name, cfg in CASES.items():
        shapes = {k: tuple(v.shape) for k, v in mods[0].VisMvsnet().state_dict().items()}
        assert len(shapes) == 367
        sd = vis_state_dict(shapes, WEIGHTS_SEED, **GAINS)
        r32 = run(mods, cfg, sd, torch.float32)
        common = {"weights_seed": np.int64(WEIGHTS_SEED), **{k: np.float64(v) for k, v in GAINS.items()}}
        if name == "c":  # the stage-3 cost volume and the regulariser outputs only
            path = os.path.join(HERE, cfg["file"])
            np.savez_compressed(path, **common, cost_3=r32["cost_3"], reg_pair_3=r32["reg_pair_3"], reg_fuse_3=r32["reg_fuse_3"])
            print(f"{cfg['file']}  {os.path.getsize(path) / 1e6:.2f} MB  (reference: {REF_ROOT})")
            continue
        r64 = run(mods, cfg, sd, torch.float64)
        rels = [float(np.max(np.abs(r32[f"depth_{s}"] - r64[f"depth_{s}"]) / np.abs(r64[f"depth_{s}"]))) for s in (1, 2, 3)]
        rel = max(rels)
        unc, ent = r32["uncertainty"], r32["pair_entropy_3"]
        u = r32["pair_heads_3"][:, 0].astype(np.float64)
        wgt = np.exp(-u[0]) / np.exp(-u).sum(0)
        frac = np.array([r64[f"jump_{s}"].mean() for s in (1, 2, 3)])
        near = [float(np.mean(np.abs(r64[f"index_{s}"] - np.round(r64[f"index_{s}"])) < 1e-3)) for s in (1, 2, 3)]
        print(f"case {name}: f32 vs f64 depth rel per stage {['%.2e' % r for r in rels]}; uncertainty 5..95 {np.percentile(unc, 5):.3f} .. "
              f"{np.percentile(unc, 95):.3f}; entropies 5..95 {np.percentile(ent, 5):.3f} .. {np.percentile(ent, 95):.3f} (min {ent.min():.3f} max "
              f"{ent.max():.3f}); view-0 fusion weight 5..95 {np.percentile(wgt, 5):.3f} .. {np.percentile(wgt, 95):.3f}; excluded per stage "
              f"{[f'{100 * f:.2f} %' for f in frac]} ('index near an integer' would exclude {[f'{100 * f:.2f} %' for f in near]}); "
              f"depth_3 {r32['depth_3'].min():.3f} .. {r32['depth_3'].max():.3f}")
        if "--dry" in sys.argv:
            continue
        assert pct(unc) >= 0.2 and pct(ent) >= 1.0 and pct(wgt) >= 0.1, "condition 1: the fixture is not sensitive"
        assert rel <= 1e-4, "condition 2: the network amplifies fp32 rounding beyond 1e-4"
        assert (frac <= 0.01).all(), "condition 3: too many pixels sit on a window jump"
        keys = sorted(shapes)
        out = {**common, "state_dict_keys": np.array(keys),
               "state_dict_shapes": np.array([list(shapes[k]) + [0] * (5 - len(shapes[k])) for k in keys], np.int64),
               "ref_f32_vs_f64_rel": np.float64(rel), "index_f64": r64["index_3"].astype(np.float64),
               "jump_3": np.packbits(r64["jump_3"]), "jump_fraction": frac.astype(np.float64)}
        for k in ("images", "poses", "intrinsics", "depth_range", "depth_1", "depth_2", "depth_3", "prob_map_3", "uncertainty", "pair_depth_3",
                  "pair_heads_3", "pair_entropy_3"):
            out[k] = r32[k]
        if name == "a":
            out["cost_1"], out["reg_pair_1"], out["reg_fuse_1"] = r32["cost_1"], r32["reg_pair_1"], r32["reg_fuse_1"]
        path = os.path.join(HERE, cfg["file"])
        np.savez_compressed(path, **out)
        print(f"{cfg['file']}  {os.path.getsize(path) / 1e6:.2f} MB  (reference: {REF_ROOT})")


if __name__ == "__main__":
    main()
