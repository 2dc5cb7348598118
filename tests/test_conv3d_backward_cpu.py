"""CPU checks of the regulariser's training path on the engine: the adjoint-weight identities behind the data gradient
(ops.conv3d_adjoint, include/mvd.h "K4 for training") against float64 autograd, and the argument checks of
ops.conv3d_autograd and MVSNet(train_regulariser=...).  tests/test_abi.py covers the new C symbols."""
import pytest
import torch
import torch.nn.functional as F

from robustmvd_amd import _lib as L
from robustmvd_amd import ops


def _layer(x, w, mode):
    if mode == L.DECONV3D_STRIDE2:
        return F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1)
    return F.conv3d(x, w, stride=1 if mode == L.CONV3D_STRIDE1 else 2, padding=1)


@pytest.mark.parametrize("mode,cin,cout,size", [(L.CONV3D_STRIDE1, 5, 3, (4, 5, 6)), (L.CONV3D_STRIDE2, 4, 6, (4, 6, 8)),
                                                (L.DECONV3D_STRIDE2, 6, 4, (2, 3, 4)), (L.CONV3D_STRIDE1, 8, 1, (3, 4, 5))])
def test_adjoint_layer_is_the_input_gradient(mode, cin, cout, size):
    """The forward of the layer ops.conv3d_adjoint names equals autograd's gradient w.r.t. the layer's input, in float64 to 1e-12."""
    g = torch.Generator().manual_seed(7 + mode)
    x = torch.randn((2, cin) + size, dtype=torch.float64, generator=g, requires_grad=True)
    w = torch.randn((cin, cout, 3, 3, 3) if mode == L.DECONV3D_STRIDE2 else (cout, cin, 3, 3, 3), dtype=torch.float64, generator=g)
    y = _layer(x, w, mode)
    gy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    y.backward(gy)
    w2, mode2 = ops.conv3d_adjoint(w, mode)
    got = _layer(gy, w2, mode2)
    assert got.shape == x.shape
    assert (got - x.grad).abs().max().item() <= 1e-12


def test_adjoint_rejects_other_kernels():
    with pytest.raises(ValueError):
        ops.conv3d_adjoint(torch.zeros(4, 4, 1, 1, 1), L.CONV3D_STRIDE1)
    with pytest.raises(ValueError):
        ops.conv3d_adjoint(torch.zeros(4, 4, 3, 3, 3), 7)


def test_conv3d_autograd_refuses_cpu_and_other_dtypes():
    x, w = torch.zeros(1, 2, 2, 2, 8), torch.zeros(8, 8, 3, 3, 3)
    with pytest.raises(ValueError, match="cuda"):
        ops.conv3d_autograd(x, w, L.CONV3D_STRIDE1)
    with pytest.raises(ValueError):
        ops.conv3d_autograd(x.double(), w.double(), L.CONV3D_STRIDE1)


def test_train_regulariser_switch():
    import robustmvd_amd as R
    assert R.MVSNet().train_regulariser == "vendor"
    assert R.MVSNet(train_regulariser="engine").train_regulariser == "engine"
    with pytest.raises(ValueError, match="train_regulariser"):
        R.MVSNet(train_regulariser="nope")
    m = R.create_model("mvsnet_train", pretrained=False, train=True, train_regulariser="engine", num_gpus=0)
    assert m.train_regulariser == "engine" and m.training
