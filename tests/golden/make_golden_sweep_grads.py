#!/usr/bin/env python3
"""Generate tests/golden/g15_sweep_grads.npz: gradients w.r.t. the FEATURE MAPS of the sweep consumers that g11 and g13 record
the forward of, by autograd through the REFERENCE's own functions (CPU, fp32, Tensor.cuda patched to the identity as in
make_golden.py::g11).

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_sweep_grads.py

Inputs are the committed fixtures' (g11_sweep_modes.npz, g13_warp_only.npz + the seeds of make_golden.py::g13).  For every output
`out` one standard-normal cotangent G = gen_common.rng_array(seed, out.shape) is drawn (the seeds are stored) and
autograd.grad(sum(out * G)) is stored:

  cvp_{pp,pl}_dkey, _dsrc{0,1}      proj_cost (cvp_mvsnet_components.py:375-456), i.e. WITH its sum / sum-of-squares aliasing.
                                    proj_cost uses in-place pow_ / div_ on tensors autograd tracks; autograd through it does not
                                    raise (the in-place results are what the later operations save) and is used as it stands.
  cvp_{pp,pl}_noalias_dkey_f64, _dsrc{0,1}_f64
                                    the variance proj_cost meant (reproduce_alias_bug=False).  The reference has no function
                                    for it: float64 torch autograd through the same grid formula and F.grid_sample, written
                                    out below (noalias_variance); the key says so.
  vis_{s,p}_dkey, _dsrc{0,1}        get_homographies + homography_warping + groupwise_correlation (blocks/utils.py:71-186) chained
                                    as SingleStage.build_cost_volume does; one cotangent per source view's volume, summed loss
  warp_{none,before,after}_dsrc{0,1}
                                    PlanesweepCorrelation(warp_only=True) (WarpOnlyCorr, planesweep_corr.py:107-140), one cotangent
                                    per view's warped volume
Arrays only.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_loader import load_reference, _load, REF_ROOT  # noqa: E402
import gen_common as gc  # noqa: E402

SEEDS = {"cvp_pp": 1600, "cvp_pl": 1601, "cvp_pp_noalias": 1602, "cvp_pl_noalias": 1603, "vis_s": 1610, "vis_p": 1620,
         "warp_none": 1630, "warp_before": 1640, "warp_after": 1650}  # per-view outputs: seed + view


def t(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def leaf(x, dtype=torch.float32):
    return t(x, dtype).requires_grad_(True)


def cot(seed, shape, dtype=torch.float32):
    return t(gc.rng_array(seed, tuple(shape)), dtype)


def noalias_variance(ref_f, src_fs, ref_in, src_in, ref_ex, src_ex, hyp):
    """proj_cost's grid (cvp_mvsnet_components.py:397-433) and grid_sample in the dtype of the inputs, with the variance over
    key + sources the function meant: sum starts from the key, sum of squares from its square."""
    B, C, h, w = ref_f.shape
    D, N = hyp.shape[1], len(src_fs) + 1
    key = ref_f.unsqueeze(2).expand(B, C, D, h, w)
    s1, s2 = key, key * key
    last = torch.tensor([[[0, 0, 0, 1.0]]], dtype=ref_f.dtype).repeat(B, 1, 1)
    for v, sf in enumerate(src_fs):
        with torch.no_grad():
            src_proj = torch.cat((src_in[:, v] @ src_ex[:, v, 0:3], last), 1)
            ref_proj = torch.cat((ref_in @ ref_ex[:, 0:3], last), 1)
            proj = src_proj @ torch.inverse(ref_proj)
            y, x = torch.meshgrid(torch.arange(h, dtype=ref_f.dtype), torch.arange(w, dtype=ref_f.dtype), indexing="ij")
            xyz = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones(h * w, dtype=ref_f.dtype))).unsqueeze(0).repeat(B, 1, 1)
            p = (proj[:, :3, :3] @ xyz).unsqueeze(2) * hyp.view(B, 1, D, h * w) + proj[:, :3, 3:4].view(B, 3, 1, 1)
            xy = p[:, :2] / p[:, 2:3]
            grid = torch.stack((xy[:, 0] / ((w - 1) / 2) - 1, xy[:, 1] / ((h - 1) / 2) - 1), dim=3)
        wv = F.grid_sample(sf, grid.view(B, D * h, w, 2), mode="bilinear", padding_mode="zeros", align_corners=False).view(B, C, D, h, w)
        s1, s2 = s1 + wv, s2 + wv * wv
    return s2 / N - (s1 / N) ** 2


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self
    cvp = _load("rmvd.models.blocks.cvp_mvsnet_components", "rmvd/models/blocks/cvp_mvsnet_components.py")
    bu = ref.blocks_utils
    g11 = np.load(os.path.join(HERE, "g11_sweep_modes.npz"))
    g13 = np.load(os.path.join(HERE, "g13_warp_only.npz"))
    out = {k + "_seed": np.int64(v) for k, v in SEEDS.items()}

    # ---- cvp
    settings = types.SimpleNamespace(nsrc=2, mode="train")
    calib = [g11[k] for k in ("cvp_ref_in", "cvp_src_in", "cvp_ref_ex", "cvp_src_ex")]
    for name in ("pp", "pl"):
        key, srcs = leaf(g11["cvp_ref"]), [leaf(g11["cvp_src0"]), leaf(g11["cvp_src1"])]
        # proj_cost squares its first argument in place (repeat() makes the copy it squares): hand it a non-leaf
        cv = cvp.proj_cost(settings, key * 1.0, [[s] for s in srcs], 0, *[t(c) for c in calib], t(g11[f"cvp_hyp_{name}"]))
        assert np.array_equal(cv.detach().numpy(), g11[f"cvp_{name}_cost"])
        gs = torch.autograd.grad((cv * cot(SEEDS[f"cvp_{name}"], cv.shape)).sum(), [key] + srcs)
        out[f"cvp_{name}_dkey"], out[f"cvp_{name}_dsrc0"], out[f"cvp_{name}_dsrc1"] = [x.numpy() for x in gs]
        f64 = torch.float64
        key, srcs = leaf(g11["cvp_ref"], f64), [leaf(g11["cvp_src0"], f64), leaf(g11["cvp_src1"], f64)]
        cv = noalias_variance(key, srcs, *[t(c, f64) for c in calib], t(g11[f"cvp_hyp_{name}"], f64))
        gs = torch.autograd.grad((cv * cot(SEEDS[f"cvp_{name}_noalias"], cv.shape, f64)).sum(), [key] + srcs)
        for k, x in zip(("dkey", "dsrc0", "dsrc1"), gs):
            out[f"cvp_{name}_noalias_{k}_f64"] = x.numpy().astype(np.float32)

    # ---- vis
    B, C, h, w, D, V = 2, 32, 12, 20, 5, 2
    for name in ("s", "p"):
        key, srcs = leaf(g11["vis_ref"]), [leaf(g11["vis_src0"]), leaf(g11["vis_src1"])]
        loss = 0.0
        for v in range(V):
            Hs = bu.get_homographies(t(g11["vis_ref_cam"]), t(g11[f"vis_src_cam{v}"]), D, t(g11[f"vis_ds_{name}"]), t(g11[f"vis_di_{name}"]))
            src_nd = srcs[v].unsqueeze(1).repeat(1, D, 1, 1, 1).view(-1, C, h, w)
            warped = bu.homography_warping(src_nd, Hs.view(-1, *Hs.size()[2:])).view(-1, D, C, h, w).transpose(1, 2)
            vol = bu.groupwise_correlation(key.unsqueeze(2).expand(-1, -1, D, -1, -1), warped, 8, 1)
            assert np.array_equal(vol.detach().numpy(), g11[f"vis_{name}_cost{v}"])
            loss = loss + (vol * cot(SEEDS[f"vis_{name}"] + v, vol.shape)).sum()
        gs = torch.autograd.grad(loss, [key] + srcs)
        out[f"vis_{name}_dkey"], out[f"vis_{name}_dsrc0"], out[f"vis_{name}_dsrc1"] = [x.numpy() for x in gs]

    # ---- warp-only block (inputs: make_golden.py::g13)
    fk = t(gc.rng_array(1501, (1, 16, 12, 18)))
    for name, norm in (("none", False), ("before", "before"), ("after", True)):
        srcs = [leaf(gc.rng_array(1502, (1, 16, 12, 18))), leaf(gc.rng_array(1503, (1, 16, 12, 18)))]
        blk = ref.planesweep_corr.PlanesweepCorrelation(warp_only=True, normalize=norm)
        warped, masks, _ = blk(feat_key=fk, intrinsics_key=t(g13["K"]), feat_sources=srcs,
                               source_to_key_transforms=[t(g13["T0"]), t(g13["T1"])], num_sampling_points=6, min_depth=0.4, max_depth=1000.0)
        loss = 0.0
        for v in range(2):
            assert np.array_equal(warped[v].detach().numpy(), g13[f"{name}_warped{v}"])
            loss = loss + (warped[v] * cot(SEEDS[f"warp_{name}"] + v, warped[v].shape)).sum()
        gs = torch.autograd.grad(loss, srcs)
        out[f"warp_{name}_dsrc0"], out[f"warp_{name}_dsrc1"] = [x.numpy() for x in gs]

    path = os.path.join(HERE, "g15_sweep_grads.npz")
    np.savez_compressed(path, **out)
    print(f"g15_sweep_grads.npz  {os.path.getsize(path) / 1e6:.2f} MB  (reference: {REF_ROOT})")


if __name__ == "__main__":
    main()
