"""GPU tests of MVSNet training through the engine: K5's training forward (mvd_softmax_regress_stats_f32) and its VJP
(mvd_softmax_regress_backward_f32), and the differentiable MVSNet.forward (reference-form FeatureNet / CostRegNet on the vendor
library's convolutions, K3 and K5 with their VJP kernels) against autograd THROUGH THE REFERENCE
(tests/golden/g14_mvsnet_train.npz, made by tests/golden/make_golden_train.py)."""
import numpy as np
import pytest
import torch

import gen_common as gc
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def unpack_f24(hi, lo):
    """Inverse of make_golden_train.pack_f24: float32 rounded to 24 bits (relative error <= 2^-16)."""
    return ((hi.astype(np.uint32) << 16) | (lo.astype(np.uint32) << 8)).view(np.float32)


def golden_grads(g, prefix, model):
    flat = unpack_f24(g[prefix + "_grad_hi"], g[prefix + "_grad_lo"])
    prm = dict(model.named_parameters())
    out, off = {}, 0
    for name in g[prefix + "_grad_names"]:
        n = prm[str(name)].numel()
        out[str(name)] = flat[off:off + n].reshape(prm[str(name)].shape)
        off += n
    assert off == flat.size
    return out


def costs(B, D, h, w, seed, scale):
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((B, D, h, w)) * scale).astype(np.float32)
    lo = rng.uniform(0.3, 1.0, (B, 1))
    dv = (lo + np.linspace(0.0, 1.0, D)[None] * rng.uniform(5.0, 20.0, (B, 1))).astype(np.float32)
    return c, dv


SHAPES = [(B, D) for B in (1, 2) for D in (8, 37, 256)]


@pytest.mark.parametrize("B,D", SHAPES)
def test_stats_forward_bit_identical(B, D, dev):
    """mvd_softmax_regress_stats_f32 (via ops.softmax_regress_autograd) returns the inference kernel's depth and confidence bit for
    bit; its statistics are the per-pixel max and 1 / sum exp(c - max).  h*w = 13*21 = 273 is not a multiple of 64."""
    from robustmvd_amd import _lib as L
    from robustmvd_amd import ops
    h, w = 13, 21
    c, dv = costs(B, D, h, w, 10 * B + D, 3.0)
    ct, dvt = torch.from_numpy(c).to(dev), torch.from_numpy(dv).to(dev)
    with torch.no_grad():
        d0, c0 = ops.softmax_regress(ct, dvt)
    d1, c1 = ops.softmax_regress_autograd(ct.clone().requires_grad_(True), dvt)
    assert d1.requires_grad and not c1.requires_grad
    assert torch.equal(d0, d1.detach()) and torch.equal(c0, c1)
    stats = torch.empty((B, 2, h, w), dtype=torch.float32, device=dev)
    d2, c2 = torch.empty_like(d0), torch.empty_like(c0)
    rc = L.load().mvd_softmax_regress_stats_f32(L.ptr(ct), L.ptr(dvt), B, D, h, w, L.ptr(d2), L.ptr(c2), L.ptr(stats),
                                                L.stream_of(ct))
    L.check(rc, "mvd_softmax_regress_stats_f32")
    assert torch.equal(d0, d2) and torch.equal(c0, c2)
    s = stats.cpu().numpy()
    c64 = c.astype(np.float64)
    assert np.array_equal(s[:, 0], c.max(1))
    np.testing.assert_allclose(s[:, 1], 1.0 / np.exp(c64 - c64.max(1, keepdims=True)).sum(1), rtol=1e-5)


@pytest.mark.parametrize("scale", [3.0, 30.0])
@pytest.mark.parametrize("B,D", SHAPES)
def test_softmax_regress_vjp(B, D, scale, dev):
    """K5 VJP against float64 autograd of softmax + depth_regression on the CPU (mvsnet.py:139-141, blocks/utils.py:271-274).
    Bound: max |g - g_ref| <= 2e-5 * max |g_ref| (fp32 exp / products; the (dv - depth) factor cancels near the soft argmin,
    where the error is absolute, so it is stated relative to max |g|).  scale 30 gives peaked softmaxes.  The depth samples
    get no gradient, like the reference's (linspace of a range without one)."""
    from robustmvd_amd import ops
    h, w = 13, 21
    c, dv = costs(B, D, h, w, 100 * B + D, scale)
    G = gc.rng_array(7 + D, (B, h, w))
    ct = torch.from_numpy(c).to(dev).requires_grad_(True)
    dvt = torch.from_numpy(dv).to(dev)
    depth, _ = ops.softmax_regress_autograd(ct, dvt)
    (depth * torch.from_numpy(G).to(dev)).sum().backward()
    c64 = torch.from_numpy(c).double().requires_grad_(True)
    p = torch.softmax(c64, 1)
    d64 = torch.sum(p * torch.from_numpy(dv).double().view(B, D, 1, 1), 1)
    (d64 * torch.from_numpy(G).double()).sum().backward()
    want = c64.grad.numpy()
    got = ct.grad.double().cpu().numpy()
    err = np.abs(got - want).max() / np.abs(want).max()
    assert err <= 2e-5, err
    np.testing.assert_allclose(depth.detach().cpu().numpy(), d64.detach().numpy(), rtol=1e-5)


def test_softmax_regress_vjp_without_depth_gradient(dev):
    """A null g_depth writes zeros (the loss reaches only the confidence, which has no VJP)."""
    from robustmvd_amd import _lib as L
    from robustmvd_amd import ops
    B, D, h, w = 2, 37, 13, 21
    c, dv = costs(B, D, h, w, 3, 3.0)
    ct, dvt = torch.from_numpy(c).to(dev), torch.from_numpy(dv).to(dev)
    depth, _ = ops.softmax_regress(ct, dvt)
    stats = torch.empty((B, 2, h, w), dtype=torch.float32, device=dev)
    rc = L.load().mvd_softmax_regress_stats_f32(L.ptr(ct), L.ptr(dvt), B, D, h, w, L.ptr(depth), None, L.ptr(stats),
                                                L.stream_of(ct))
    L.check(rc, "mvd_softmax_regress_stats_f32")
    g = torch.full_like(ct, float("nan"))
    rc = L.load().mvd_softmax_regress_backward_f32(L.ptr(ct), L.ptr(dvt), L.ptr(depth), L.ptr(stats), None, B, D, h, w, L.ptr(g),
                                                   L.stream_of(ct))
    L.check(rc, "mvd_softmax_regress_backward_f32")
    assert torch.count_nonzero(g).item() == 0


def _g14_model(dev, train):
    import robustmvd_amd as R
    import make_golden_train as MG
    m = R.MVSNet(num_sampling_steps=MG.D)
    m.load_state_dict(MG.state_dict(m))
    return m.to(dev).train(train), MG


def _g14_step(model, MG, dev):
    images, poses, intr = MG.inputs()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pred, _ = model(images=[t(i) for i in images], poses=[t(p) for p in poses], intrinsics=[t(k) for k in intr],
                    keyview_idx=torch.tensor([0] * MG.B), depth_range=[torch.tensor([MG.DEPTH_RANGE[0]] * MG.B),
                                                                       torch.tensor([MG.DEPTH_RANGE[1]] * MG.B)])
    G = t(gc.rng_array(MG.G_SEED, tuple(pred["depth"].shape)))
    (pred["depth"] * G).sum().backward()
    return pred


def _check_grads(model, want, bound):
    """Relative L2 error <= bound per parameter.  cost_regularization.prob.bias is mathematically zero (a constant added to
    every depth plane leaves the softmax unchanged): what both sides hold is rounding residue, checked as <= 1e-6 of the norm
    of all parameter gradients together."""
    prm = dict(model.named_parameters())
    total = np.sqrt(sum(float(np.sum(v.astype(np.float64) ** 2)) for v in want.values()))
    bad = []
    for name, w in want.items():
        got = prm[name].grad.cpu().numpy()
        if name == "cost_regularization.prob.bias":
            if not np.abs(got).max() <= 1e-6 * total:
                bad.append((name, float(np.abs(got).max()), total))
            continue
        err = np.linalg.norm(got.astype(np.float64) - w) / np.linalg.norm(w.astype(np.float64))
        if not err <= bound:
            bad.append((name, float(err)))
    assert bad == [], bad


def test_mvsnet_train_mode_golden(dev):
    """MVSNet in train mode (B = 2, BN on batch statistics) against the reference's own MVSNet: depth rtol 1e-3 (Path B),
    BN running statistics after the forward rtol 1e-4, every parameter gradient within relative L2 error 1.5e-2.  The gradient bound
    is looser than eval mode's 1e-3 because the fixture itself is only about that accurate: the train-mode BatchNorm backward
    subtracts batch means of the incoming gradient, which cancels most of it, and the reference's fp32 CPU gradients differ from a
    float64 evaluation of the same step by up to 3.6e-3 (cost_regularization.conv7.1.weight; 1e-5 in eval mode).  Measured on an
    MI355X: 7.2e-3 at worst (cost_regularization.conv2.bn.bias), median 2.5e-3; eval mode 9e-6."""
    g = load_golden("g14_mvsnet_train")
    model, MG = _g14_model(dev, True)
    pred = _g14_step(model, MG, dev)
    assert pred["depth"].shape == (MG.B, 1, MG.H // 4, MG.W // 4) and not pred["depth_uncertainty"].requires_grad
    np.testing.assert_allclose(pred["depth"].detach().cpu().numpy(), g["train_depth"], rtol=1e-3)
    np.testing.assert_allclose(pred["depth_uncertainty"].cpu().numpy(), g["train_depth_uncertainty"], atol=2e-3)  # as test_mvsnet_end_to_end_golden
    for k, v in model.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            np.testing.assert_allclose(v.cpu().numpy(), g["train_bn/" + k], rtol=1e-4, atol=1e-7, err_msg=k)
    _check_grads(model, golden_grads(g, "train", model), 1.5e-2)


def test_mvsnet_eval_mode_grad_golden(dev):
    """Eval mode with autograd on (fine-tuning with frozen BN) takes the differentiable path too: depth and the gradients of
    the first / last layers of FeatureNet and CostRegNet and of `prob` against the reference."""
    g = load_golden("g14_mvsnet_train")
    model, MG = _g14_model(dev, False)
    pred = _g14_step(model, MG, dev)
    np.testing.assert_allclose(pred["depth"].detach().cpu().numpy(), g["eval_depth"], rtol=1e-3)
    _check_grads(model, golden_grads(g, "eval", model), 1e-3)


def _sample(seed=3, H=64, W=96):
    from robustmvd_amd.registry import add_batch_dim
    s = gc.synthetic_sample(seed, H, W, 2)
    im, key, po, intr, dr = add_batch_dim(s["images"], 0, s["poses"], s["intrinsics"], (np.float32(0.5), np.float32(10.0)))
    return dict(images=im, keyview_idx=key, poses=po, intrinsics=intr, depth_range=dr)


def test_mvsnet_train_every_parameter_gets_a_gradient(dev):
    """create_model("mvsnet_train", train=True): one forward + backward from input_adapter output gives every parameter a finite,
    non-zero gradient (prob.bias: finite only, its gradient is mathematically zero, see _check_grads)."""
    import robustmvd_amd as R
    model = R.create_model("mvsnet_train", pretrained=False, train=True)
    assert model.training and not R.has_model("mvsnet_train", trainable_only=True)
    pred, _ = model(**model.input_adapter(**_sample()))
    pred["depth"].mean().backward()
    bad = [k for k, p in model.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()
           or (k != "cost_regularization.prob.bias" and not bool((p.grad != 0).any()))]
    assert bad == [], bad


def test_mvsnet_training_lowers_the_loss_and_inference_sees_the_weights(dev):
    """20 RMSprop steps (lr 1e-3, as run_confs/mvsnet.yaml) on one sample against a fixed target depth: the loss stays finite and
    ends below its start.  Then eval() + run() (the engine path, whose packed weights were cached before training) is bit-identical
    to a freshly built eval model loaded with the trained state dict."""
    import robustmvd_amd as R
    model = R.create_model("mvsnet_train", pretrained=False, train=False)
    s = _sample()
    before, _ = model.run(**s)                      # fills the engine's packed-weight caches with the initial weights
    model.train()
    opt = torch.optim.RMSprop(model.parameters(), lr=1e-3)
    sample = model.input_adapter(**s)
    target = torch.linspace(2.0, 8.0, 96 // 4, device=dev).expand(1, 1, 64 // 4, 96 // 4)
    losses = []
    for _ in range(21):
        opt.zero_grad(set_to_none=True)
        pred, _ = model(**sample)
        loss = (pred["depth"] - target).abs().mean()
        losses.append(float(loss.detach()))
        if len(losses) == 21:
            break
        loss.backward()
        opt.step()
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses
    model.eval()
    after, _ = model.run(**s)
    assert not np.array_equal(after["depth"], before["depth"])
    fresh = R.create_model("mvsnet_train", pretrained=False, train=False)
    fresh.load_state_dict(model.state_dict())
    want, _ = fresh.run(**s)
    assert np.array_equal(after["depth"], want["depth"])
    assert np.array_equal(after["depth_uncertainty"], want["depth_uncertainty"])
