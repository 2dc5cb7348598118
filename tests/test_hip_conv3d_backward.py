"""GPU tests of the regulariser's backward on the engine: ops.conv3d_autograd (forward and data gradient on
mvd_conv3d_bn_relu_f32 with adjoint weights, weight gradient on mvd_conv3d_weight_grad_f32) against float64 autograd on the CPU
and against the vendor library's fp32 backward, its determinism, and MVSNet(train_regulariser="engine") against autograd THROUGH
THE REFERENCE (tests/golden/g14_mvsnet_train.npz), against the vendor path and in a short training run."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_common as gc
from conftest import load_golden
from test_hip_mvsnet_train import _check_grads, _g14_step, _sample, golden_grads

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # unit roundoff of fp32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _layers():
    from robustmvd_amd import _lib as L
    from robustmvd_amd.blocks import CostRegNet
    out = [(name, cin, cout, L.CONV3D_STRIDE1 if stride == 1 else L.CONV3D_STRIDE2) for name, cin, cout, stride in CostRegNet.LAYERS]
    out += [(name, cin, cout, L.DECONV3D_STRIDE2) for name, cin, cout in CostRegNet.UPS]
    return out + [("prob", 8, 1, L.CONV3D_STRIDE1)]


def _ref_layer(x, w, mode):
    """The layer on (B,C,D,h,w) tensors, any dtype / device: what the reference's modules compute (mvsnet_components.py:25-41,84-109)."""
    from robustmvd_amd import _lib as L
    if mode == L.DECONV3D_STRIDE2:
        return F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1)
    return F.conv3d(x, w, stride=1 if mode == L.CONV3D_STRIDE1 else 2, padding=1)


def _vjp(x, w, gy, mode):
    """(y, gx, gw) of the layer by torch autograd on the tensors' own device and dtype; channel-first."""
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    y = _ref_layer(x, w, mode)
    y.backward(gy)
    return y.detach(), x.grad, w.grad


def _cl(t):  # (B,C,D,h,w) -> channel-last
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _cf(t):  # channel-last -> (B,C,D,h,w)
    return t.permute(0, 4, 1, 2, 3).contiguous()


def _check(name, got, ref, S, n, vendor):
    """The two assertions of a tensor: the order-independent forward error bound of an fp32 sum of n exactly rounded products,
    |got - ref| <= (n + 2) u S elementwise (S = the same sum over absolute values, float64), and e_engine <= 4 e_vendor with
    e = max |. - ref| / max |ref|, unless the vendor accumulates in higher precision (e_vendor < 1e-7).  Returns (e_engine, e_vendor)."""
    got, vendor = got.double().cpu(), vendor.double().cpu()
    err = (got - ref).abs()
    bound = (n + 2) * U * S
    scale = ref.abs().max().item()
    e_eng, e_ven = err.max().item() / scale, (vendor - ref).abs().max().item() / scale
    print(f"{name}: n={n} e_engine={e_eng:.3e} e_vendor={e_ven:.3e} worst err/bound={(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert bool((err <= bound).all()), (name, "hard bound", (err / bound.clamp_min(1e-300)).max().item())
    if e_ven >= 1e-7:
        assert e_eng <= 4 * e_ven, (name, e_eng, e_ven)
    return e_eng, e_ven


@pytest.mark.parametrize("tensor", ["y", "gx", "gw"])
@pytest.mark.parametrize("name,cin,cout,mode", _layers())
def test_layer_vjp_against_float64(name, cin, cout, mode, tensor, dev):
    """Every (Cin, Cout, mode) of CostRegNet and `prob`, B = 2, on a volume that is no multiple of any tile (6 x 10 x 14 voxels on
    the side the weight-gradient kernel tiles, twice that on the input of a stride-2 layer): forward, gx and gw of
    ops.conv3d_autograd against float64 autograd on the CPU, with the hard bound and the vendor comparison of _check.
    Measured on an MI355X (e = max error / max |ref|; engine / vendor over the eleven layers):
      y  1.0e-7 .. 1.8e-6 / 1.2e-7 .. 5.2e-7;  gx 1.2e-7 .. 5.7e-7 / 1.2e-7 .. 3.6e-7;  gw 1.4e-7 .. 4.0e-7 / 2.5e-7 .. 9.2e-7;
      worst error / hard bound 0.034 (y), 0.12 (gx), 6.2e-4 (gw); worst e_engine / e_vendor 3.4 (conv6 y), 3.1 (conv1 gx), 1.1 (conv1 gw).
    The vendor's data-gradient error does not grow with n (1.2e-7 .. 3.6e-7 from n = 27 to 1728: it adds in blocks or in higher
    precision, yet measures above the 1e-7 below which the comparison would be dropped), while a layer kernel that adds all n
    products into one fp32 chain errs like sqrt(n): with single chains conv3 / conv4 / conv6 gx measured 5.3x / 5.5x / 8.2x the
    vendor's (6.2e-7, 1.07e-6, 1.79e-6).  ops.conv3d_autograd therefore computes gx with blocked accumulation (chains of at most
    27 * 8 products, ops._conv3d_blocked): conv3 / conv4 / conv6 gx now 3.2e-7 / 2.7e-7 / 3.7e-7 (2.8x / 1.4x / 1.7x)."""
    from robustmvd_amd import _lib as L
    from robustmvd_amd import ops
    B, (D, h, w) = 2, ((12, 20, 28) if mode == L.CONV3D_STRIDE2 else (6, 10, 14))
    g = torch.Generator().manual_seed(1000 + 10 * cin + cout + mode)
    x = torch.randn((B, cin, D, h, w), generator=g)
    wt = torch.randn((cin, cout, 3, 3, 3) if mode == L.DECONV3D_STRIDE2 else (cout, cin, 3, 3, 3), generator=g) * 0.2
    gy = torch.randn(_ref_layer(x, wt, mode).shape, generator=g)
    y64, gx64, gw64 = _vjp(x.double(), wt.double(), gy.double(), mode)
    Sy, Sgx, Sgw = _vjp(x.double().abs(), wt.double().abs(), gy.double().abs(), mode)  # all three are bilinear: sums of |products|
    yv, gxv, gwv = _vjp(x.to(dev), wt.to(dev), gy.to(dev), mode)                        # the vendor library, fp32

    xe = _cl(x).to(dev).requires_grad_(True)
    we = wt.to(dev).requires_grad_(True)
    ye = ops.conv3d_autograd(xe, we, mode)
    ye.backward(_cl(gy).to(dev))
    nvox = gy.numel() // gy.shape[1] if mode != L.DECONV3D_STRIDE2 else x.numel() // cin
    taps_f = 8 if mode == L.DECONV3D_STRIDE2 else 27   # terms per output voxel and input channel
    taps_b = 8 if mode == L.CONV3D_STRIDE2 else 27
    if tensor == "y":
        _check(name + " y", _cf(ye.detach()), y64, Sy, taps_f * cin, yv)
    elif tensor == "gx":
        _check(name + " gx", _cf(xe.grad), gx64, Sgx, taps_b * cout, gxv)
    else:
        _check(name + " gw", we.grad, gw64, Sgw, nvox, gwv)


def _large_case(dev):
    B, D, h, w, cin, cout = 1, 32, 160, 200, 32, 8
    g = torch.Generator().manual_seed(5)
    x = torch.randn((B, D, h, w, cin), generator=g)
    gy = torch.randn((B, D, h, w, cout), generator=g)
    return x, gy


def test_weight_gradient_large_reduction(dev):
    """Stride-1 32 -> 8 over 1,024,000 voxels (many partial sums): gw against the per-tap float64 reduction
    gw[co,ci,k] = sum_o gy[o,co] xpad[o+k,ci] on the CPU, same two assertions.
    Measured on an MI355X: e_engine 1.0e-6, e_vendor 3.8e-5, worst error / hard bound 1.1e-7."""
    from robustmvd_amd import _lib as L
    from robustmvd_amd import ops
    x, gy = _large_case(dev)
    B, D, h, w, cin = x.shape
    cout = gy.shape[-1]
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1, 1, 1))
    g2 = gy.double().reshape(-1, cout)
    ref = torch.empty((cout, cin, 3, 3, 3), dtype=torch.float64)
    S = torch.empty_like(ref)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                xs = xp[:, kd:kd + D, kh:kh + h, kw:kw + w].reshape(-1, cin)
                ref[:, :, kd, kh, kw] = g2.t() @ xs
                S[:, :, kd, kh, kw] = g2.abs().t() @ xs.abs()
    got = ops.conv3d_weight_grad(x.to(dev), gy.to(dev), L.CONV3D_STRIDE1)
    xv = x.to(dev).permute(0, 4, 1, 2, 3).contiguous()
    wv = torch.zeros((cout, cin, 3, 3, 3), device=dev, requires_grad=True)
    F.conv3d(xv, wv, padding=1).backward(gy.to(dev).permute(0, 4, 1, 2, 3).contiguous())
    _check("large gw", got, ref, S, B * D * h * w, wv.grad)


def _engine_model(dev, train, D, state=None):
    import robustmvd_amd as R
    m = R.MVSNet(num_sampling_steps=D, train_regulariser="engine")
    if state is not None:
        m.load_state_dict(state(m))
    return m.to(dev).train(train)


def test_weight_gradient_and_model_backward_are_deterministic(dev):
    """Two calls of mvd_conv3d_weight_grad_f32 on the large case are bit-identical (no atomics: partials added in a fixed order), and
    so are two full training steps of the model: every gradient the regulariser's backward produces — all of CostRegNet's
    parameters and the gradient it hands back to the cost volume — is torch.equal between the two.  (FeatureNet's gradients come
    out of K3's VJP, a scatter-add with float atomics that include/mvd.h documents as order-dependent: they are compared to 1e-4
    of their norm instead; measured 1.6e-7 .. 8.1e-7 between two steps on an MI355X.)"""
    from robustmvd_amd import _lib as L
    from robustmvd_amd import ops
    x, gy = _large_case(dev)
    x, gy = x.to(dev), gy.to(dev)
    a = ops.conv3d_weight_grad(x, gy, L.CONV3D_STRIDE1)
    b = ops.conv3d_weight_grad(x, gy, L.CONV3D_STRIDE1)
    assert torch.equal(a, b)
    del x, gy

    import make_golden_train as MG
    model = _engine_model(dev, True, MG.D, MG.state_dict)
    reg = model.cost_regularization
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        kept = []

        def tapped(v, kept=kept):  # the gradient the regulariser hands back to the cost volume
            v.register_hook(lambda g: kept.append(g.clone()))
            return type(reg).forward_autograd_engine(reg, v)

        reg.forward_autograd_engine = tapped
        try:
            _g14_step(model, MG, dev)
        finally:
            del reg.forward_autograd_engine
        assert len(kept) == 1
        runs.append(({k: p.grad.clone() for k, p in model.named_parameters()}, kept[0]))
    (g0, v0), (g1, v1) = runs
    assert torch.equal(v0, v1)
    for k in g0:
        if k.startswith("cost_regularization."):
            assert torch.equal(g0[k], g1[k]), k
        else:
            assert (g0[k] - g1[k]).norm().item() <= 1e-4 * g0[k].norm().item(), k


def test_mvsnet_engine_train_mode_golden(dev):
    """test_mvsnet_train_mode_golden with train_regulariser="engine", same fixture and bounds: depth rtol 1e-3, BN running statistics
    rtol 1e-4, num_batches_tracked equal, every parameter gradient within relative L2 1.5e-2 (prob.bias <= 1e-6 of the total norm).
    Measured on an MI355X: worst gradient error 3.6e-3 (cost_regularization.conv7.1.weight); the vendor path measures 7.2e-3."""
    import make_golden_train as MG
    g = load_golden("g14_mvsnet_train")
    model = _engine_model(dev, True, MG.D, MG.state_dict)
    pred = _g14_step(model, MG, dev)
    assert pred["depth"].shape == (MG.B, 1, MG.H // 4, MG.W // 4) and not pred["depth_uncertainty"].requires_grad
    np.testing.assert_allclose(pred["depth"].detach().cpu().numpy(), g["train_depth"], rtol=1e-3)
    np.testing.assert_allclose(pred["depth_uncertainty"].cpu().numpy(), g["train_depth_uncertainty"], atol=2e-3)
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert np.array_equal(v.cpu().numpy(), g["train_bn/" + k]), k
        elif k.endswith(("running_mean", "running_var")):
            np.testing.assert_allclose(v.cpu().numpy(), g["train_bn/" + k], rtol=1e-4, atol=1e-7, err_msg=k)
    print("worst train-mode gradient error", _worst(model, golden_grads(g, "train", model)))
    _check_grads(model, golden_grads(g, "train", model), 1.5e-2)


def test_mvsnet_engine_eval_mode_grad_golden(dev):
    """test_mvsnet_eval_mode_grad_golden with train_regulariser="engine": depth rtol 1e-3, gradients within relative L2 1e-3.
    Measured on an MI355X: worst gradient error 9.2e-6 (feature.feature.weight); the vendor path measures 9e-6."""
    import make_golden_train as MG
    g = load_golden("g14_mvsnet_train")
    model = _engine_model(dev, False, MG.D, MG.state_dict)
    pred = _g14_step(model, MG, dev)
    np.testing.assert_allclose(pred["depth"].detach().cpu().numpy(), g["eval_depth"], rtol=1e-3)
    print("worst eval-mode gradient error", _worst(model, golden_grads(g, "eval", model)))
    _check_grads(model, golden_grads(g, "eval", model), 1e-3)


def _worst(model, want):
    prm = dict(model.named_parameters())
    errs = {k: float(np.linalg.norm(prm[k].grad.cpu().numpy().astype(np.float64) - w) / np.linalg.norm(w.astype(np.float64)))
            for k, w in want.items() if k != "cost_regularization.prob.bias"}
    k = max(errs, key=errs.get)
    return k, errs[k]


def test_engine_step_matches_vendor_step(dev):
    """128 x 160, 2 sources, 32 planes, eval mode with gradients, seeded weights and sample: every parameter gradient of the engine
    path within relative L2 1e-3 of the vendor path's (the project's eval-mode bound, prob.bias as in _check_grads), depth rtol 1e-3.
    Measured on an MI355X: 5.5e-6 at worst (feature.conv0.bn.bias)."""
    import robustmvd_amd as R
    from robustmvd_amd.registry import add_batch_dim
    H, W, V, D = 128, 160, 2, 32
    s = gc.synthetic_sample(11, H, W, V)
    im, key, po, intr, dr = add_batch_dim(s["images"], 0, s["poses"], s["intrinsics"], (np.float32(0.5), np.float32(10.0)))
    grads, depths = {}, {}
    for which in ("vendor", "engine"):
        model = R.MVSNet(num_sampling_steps=D, train_regulariser=which)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        full = model.state_dict()
        for k, v in gc.fill_state_dict(shapes, 1).items():
            full[k] = torch.from_numpy(v)
        model.load_state_dict(full)
        model = model.to(dev).eval()
        sample = model.input_adapter(images=im, keyview_idx=key, poses=po, intrinsics=intr, depth_range=dr)
        pred, _ = model(**sample)
        G = torch.from_numpy(gc.rng_array(17, tuple(pred["depth"].shape))).to(dev)
        (pred["depth"] * G).sum().backward()
        depths[which] = pred["depth"].detach().cpu().numpy()
        grads[which] = model
    np.testing.assert_allclose(depths["engine"], depths["vendor"], rtol=1e-3)
    want = {k: p.grad.cpu().numpy() for k, p in grads["vendor"].named_parameters()}
    print("worst engine-vs-vendor gradient error", _worst(grads["engine"], want))
    _check_grads(grads["engine"], want, 1e-3)


def test_engine_training_lowers_the_loss_and_inference_sees_the_weights(dev):
    """test_mvsnet_training_lowers_the_loss_and_inference_sees_the_weights with the regulariser's backward on the engine: 20 RMSprop
    steps, finite and decreasing loss; afterwards eval() + run() is bit-identical to a fresh eval model with the trained weights."""
    import robustmvd_amd as R
    model = R.create_model("mvsnet_train", pretrained=False, train=False, train_regulariser="engine")
    s = _sample()
    before, _ = model.run(**s)
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
