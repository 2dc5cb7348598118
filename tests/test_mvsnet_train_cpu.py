"""CPU checks of MVSNet training through the engine (no GPU): the differentiable path is taken in training mode, the
g14 fixture matches this package's state dict, and the binding table carries K5's training symbols."""
import numpy as np
import pytest
import torch

import gen_common as gc
from conftest import load_golden


def test_train_mode_forward_reaches_the_engine():
    """MVSNet().train() no longer stops at the folded-BN refusal of the inference path (`call .eval() first`): the reference-form
    FeatureNet runs on the CPU, and the call fails at K3's device check, as every engine entry point does on CPU tensors."""
    import robustmvd_amd as R
    model = R.MVSNet(num_sampling_steps=8).train()
    s = gc.synthetic_sample(0, 32, 64, 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None]
    kw = dict(images=[t(((im / 255.0) - 0.45) / 0.225).float() for im in s["images"]], poses=[t(p) for p in s["poses"]],
              intrinsics=[t(k) for k in s["intrinsics"]], keyview_idx=torch.tensor([0]),
              depth_range=[torch.tensor([0.5]), torch.tensor([10.0])])
    with pytest.raises(ValueError, match="needs a cuda"):
        model(**kw)
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"call \.eval\(\) first"):
        model.feature.forward_layout(kw["images"][0], 0)   # the inference path keeps its refusal
    with pytest.raises(ValueError, match="inference-only"):
        R.MVSNet(num_sampling_steps=8, half_features=True).train()(**kw)


def test_module_autograd_forwards_match_the_reference_form():
    """FeatureNet / CostRegNet.forward_autograd: the reference's layer sequence on the modules' own layers (mvsnet_components.py),
    recording a graph; the inference-only forward keeps refusing in training mode."""
    from robustmvd_amd import blocks as B
    torch.manual_seed(0)
    fn = B.FeatureNet().train()
    y = fn.forward_autograd(torch.randn(2, 3, 32, 32))
    assert y.shape == (2, 32, 8, 8) and y.requires_grad
    cr = B.CostRegNet().train()
    x = torch.randn(1, 32, 8, 16, 16)
    out = cr.forward_autograd(x)
    assert out.shape == (1, 1, 8, 16, 16) and out.requires_grad
    out.sum().backward()
    assert all(p.grad is not None for p in cr.parameters())
    with pytest.raises(RuntimeError, match="inference-only"):
        cr.forward(x)


def test_g14_matches_the_state_dict():
    import robustmvd_amd as R
    g = load_golden("g14_mvsnet_train")
    B, H, W, D, V = (int(v) for v in g["shape"])
    model = R.MVSNet(num_sampling_steps=D)
    sd = model.state_dict()
    params = dict(model.named_parameters())
    assert list(g["train_grad_names"]) == list(params)
    assert g["train_grad_hi"].size == g["train_grad_lo"].size == sum(p.numel() for p in params.values())
    assert all(str(n) in params for n in g["eval_grad_names"])
    assert g["eval_grad_hi"].size == sum(params[str(n)].numel() for n in g["eval_grad_names"])
    bn = {k[len("train_bn/"):]: g[k] for k in g.files if k.startswith("train_bn/")}
    assert set(bn) == {k for k in sd if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    for k, v in bn.items():
        assert v.shape == tuple(sd[k].shape), k
    assert g["train_depth"].shape == g["eval_depth"].shape == (B, 1, H // 4, W // 4)


def test_training_symbols_are_bound():
    from robustmvd_amd import _lib
    assert "mvd_softmax_regress_stats_f32" in _lib.SIGNATURES
    assert "mvd_softmax_regress_backward_f32" in _lib.SIGNATURES
