#!/usr/bin/env python3
"""Generate tests/golden/g14_mvsnet_train.npz by running the REFERENCE's own MVSNet with autograd on (CPU, fp32).

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_train.py
The training loop calls model(**sample) with autograd recording (multi_view_depth_training.py:231-246); this records what
one such step computes, on the inputs of gen_common.py:

  B = 2 (two synthetic_sample frames stacked), 64x96, D = 32, V = 2 sources, depth range (0.5, 10), keyview 0,
  weights fill_state_dict(seed 1400), loss = sum(depth * G) with G = rng_array(1403, depth.shape).

  train_*   model.train(): depth, depth_uncertainty, the gradient of every parameter, the BN running statistics after the
            forward (running_mean / running_var / num_batches_tracked)
  eval_*    model.eval() with autograd on (fine-tuning with frozen BN): depth and the gradients of EVAL_GRADS

Parameter gradients are stored as float32 rounded to 24 bits (relative error <= 2^-16): the high 16 bits in
`*_grad_hi` (uint16) and the next 8 in `*_grad_lo` (uint8), all parameters concatenated in the order of `*_grad_names`
(see unpack_f24 in tests/test_hip_mvsnet_train.py).  That keeps the fixture under 1 MiB; full fp32 would be 1.4 MB.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_loader import load_reference  # noqa: E402
import gen_common as gc  # noqa: E402

H, W, D, V, B = 64, 96, 32, 2, 2
WEIGHT_SEED, SAMPLE_SEEDS, G_SEED = 1400, (1401, 1402), 1403
DEPTH_RANGE = (0.5, 10.0)
EVAL_GRADS = ["feature.conv0.conv.weight", "feature.feature.weight", "feature.feature.bias",
              "cost_regularization.conv0.conv.weight", "cost_regularization.conv11.0.weight", "cost_regularization.prob.weight"]


def pack_f24(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x80) & 0xFFFFFF00).astype(np.uint32)  # round to nearest at bit 8 (a carry moves into the exponent correctly)
    return (u >> 16).astype(np.uint16), ((u >> 8) & 0xFF).astype(np.uint8)


def inputs():
    """Normalised images (mvsnet.py:181-183), poses, intrinsics of B stacked synthetic frames."""
    mean = np.array([0.485, 0.456, 0.406], np.float32).reshape(3, 1, 1)
    std = np.array([0.229, 0.224, 0.225], np.float32).reshape(3, 1, 1)
    ss = [gc.synthetic_sample(s, H, W, V) for s in SAMPLE_SEEDS]
    images = [np.stack([((s["images"][v] / 255.0 - mean) / std).astype(np.float32) for s in ss]) for v in range(V + 1)]
    poses = [np.stack([s["poses"][v] for s in ss]) for v in range(V + 1)]
    intr = [np.stack([s["intrinsics"][v] for s in ss]) for v in range(V + 1)]
    return images, poses, intr


def state_dict(model):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = gc.fill_state_dict(shapes, WEIGHT_SEED)
    full = {k: torch.from_numpy(v) for k, v in sd.items()}
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            full[k] = v
    return full


def step(model):
    images, poses, intr = inputs()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    pred, _ = model(images=[t(i) for i in images], poses=[t(p.copy()) for p in poses],  # the reference writes into poses
                    intrinsics=[t(k) for k in intr], keyview_idx=torch.tensor([0] * B),
                    depth_range=[torch.tensor([DEPTH_RANGE[0]] * B), torch.tensor([DEPTH_RANGE[1]] * B)])
    G = torch.from_numpy(gc.rng_array(G_SEED, tuple(pred["depth"].shape)))
    (pred["depth"] * G).sum().backward()
    return pred


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    out = {"shape": np.array([B, H, W, D, V]), "weight_seed": np.int64(WEIGHT_SEED), "sample_seeds": np.array(SAMPLE_SEEDS),
           "g_seed": np.int64(G_SEED), "depth_range": np.array(DEPTH_RANGE, np.float32)}
    with torch.enable_grad():
        model = ref.mvsnet.MVSNet(num_sampling_steps=D)
        model.load_state_dict(state_dict(model))
        model.train()
        pred = step(model)
        out["train_depth"] = pred["depth"].detach().numpy()
        out["train_depth_uncertainty"] = pred["depth_uncertainty"].detach().numpy()
        names = [k for k, _ in model.named_parameters()]
        out["train_grad_names"] = np.array(names)
        out["train_grad_hi"], out["train_grad_lo"] = pack_f24(np.concatenate([p.grad.numpy().ravel() for _, p in model.named_parameters()]))
        for k, v in model.state_dict().items():
            if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
                out["train_bn/" + k] = v.numpy()

        model = ref.mvsnet.MVSNet(num_sampling_steps=D)
        model.load_state_dict(state_dict(model))
        model.eval()
        pred = step(model)
        out["eval_depth"] = pred["depth"].detach().numpy()
        prm = dict(model.named_parameters())
        out["eval_grad_names"] = np.array(EVAL_GRADS)
        out["eval_grad_hi"], out["eval_grad_lo"] = pack_f24(np.concatenate([prm[k].grad.numpy().ravel() for k in EVAL_GRADS]))
    path = os.path.join(HERE, "g14_mvsnet_train.npz")
    np.savez_compressed(path, **out)
    print(f"g14_mvsnet_train.npz  {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
