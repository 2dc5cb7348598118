"""CPU checks of what tests/test_hip_conv3d_weight_grad.py stands on (tests/wgrad_cases.py): the case table names every
instantiation of conv3d_weight_grad_kernel and states the plan the library reports (mvd_conv3d_weight_grad_plan_field is a host
function: no GPU is touched), the float64 reduction is the layer's weight gradient, and integer data keeps fp32 exact."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as WC
from robustmvd_amd import _lib as L


def test_table_names_every_instantiation_and_the_networks_layers():
    assert (WC.STRIDE1, WC.STRIDE2, WC.DECONV) == (L.CONV3D_STRIDE1, L.CONV3D_STRIDE2, L.DECONV3D_STRIDE2)
    assert len(WC.LAYER_CASES) == 11 and len(WC.CASES) == 11 + 3 + 7
    assert {c[3] for c in WC.CASES.values()} == set(itertools.product((1, 2), (1, 2), (1, 2)))
    assert {c[3] for c in WC.LAYER_CASES.values()} == {(1, 2, 1), (1, 1, 2), (1, 1, 1), (2, 1, 2), (2, 2, 1), (2, 2, 2)}
    assert {c[4] for c in WC.LAYER_CASES.values()} == {(1, 1), (2, 1), (2, 2)}
    assert {c[3] for c in WC.UNREACHED_CASES.values()} == {(2, 1, 1), (1, 2, 2)}
    for name, case in WC.CASES.items():
        assert WC.expected_plan(name) == case[3:], name
    assert {WC.sides(n)[0] for n in WC.CONTRACT_CASES} == {1, 2}
    assert set(WC.ROUNDING_CASES) == set(WC.LAYER_CASES) | set(WC.UNREACHED_CASES)


@pytest.mark.parametrize("regime", WC.REGIMES, ids=lambda r: f"B{r[0]}")
@pytest.mark.parametrize("name", list(WC.CASES))
def test_library_plans_the_regimes(name, regime):
    WC.assert_plan(name, regime)


def test_regimes_are_what_their_names_say():
    """one item per workgroup at DZ = 1; more items than workgroups at DZ = 2, 4, 8; at DZ = 8 ten workgroups take a second item"""
    assert [r[1] for r in WC.REGIMES] == [1, 2, 4, 8]
    assert WC.REGIMES[0][2] <= WC.MAX_PARTIALS and all(r[2] > WC.MAX_PARTIALS for r in WC.REGIMES[1:])
    assert WC.MARCH8[2] - WC.MAX_PARTIALS == 10
    for S, (d, h, w) in WC.SMALL_DHW.items():
        TW = 16 if S == 1 else 8
        assert (d, h, w) == (9, 9, 2 * TW + 1)
    for B, DZ, items, _ in WC.REGIMES:
        assert items == B * 3 * 3 * -(-9 // DZ)


def test_plan_query_refuses_what_the_launch_refuses():
    fn = L.load().mvd_conv3d_weight_grad_plan_field
    ws = L.load().mvd_conv3d_weight_grad_workspace_bytes
    ok = (2, 9, 9, 33, 8, 8, L.CONV3D_STRIDE1)
    assert fn(*ok, L.WGRAD_PLAN_DZ) == 1 and fn(*ok, L.WGRAD_PLAN_ITEMS) == 162 and ws(*ok) > 0
    assert fn(*ok, 8) == 0 and fn(*ok, -1) == 0                              # unknown field
    for bad in ((2, 9, 9, 33, 65, 8, L.CONV3D_STRIDE1), (2, 9, 9, 33, 8, 0, L.CONV3D_STRIDE1), (0, 9, 9, 33, 8, 8, L.CONV3D_STRIDE1),
                (2, 9, 9, 33, 8, 8, L.CONV3D_STRIDE2), (2, 9, 9, 33, 8, 8, 3)):
        assert ws(*bad) == 0
        for f in range(8):
            assert fn(*bad, f) == 0, (bad, f)
    # the workspace is what the reported plan needs: blocks x partials x 27 taps x (16 COT) x (16 CIT) floats, rounded up to 256 B
    for name in WC.CASES:
        for regime in WC.REGIMES:
            p = WC.plan(name, regime[0])
            mode, cin, cout = WC.CASES[name][:3]
            need = p["CS_BLOCKS"] * p["CG_BLOCKS"] * p["PARTIALS"] * 27 * 16 * p["COT"] * 16 * p["CIT"] * 4
            assert ws(regime[0], *WC.input_dhw(name), cin, cout, mode) == -(-need // 256) * 256, (name, regime)


@pytest.mark.parametrize("name", list(WC.CASES))
def test_reduction_is_the_layers_weight_gradient(name):
    """WC.reduction on gaussian elements against float64 autograd through the layer (F.conv3d / F.conv_transpose3d), to 1e-12 of
    the sum of absolute products; shapes as the device test builds them."""
    mode, cin, cout = WC.CASES[name][:3]
    S = WC.sides(name)[0]
    sm, bg = WC.elements(name, "gauss")
    x, gy = WC.x_gy(name, sm, bg)
    assert tuple(x.shape) == (3, *WC.input_dhw(name), cin) and gy.shape[-1] == cout
    gw, sa = WC.reduction(sm, bg, S)
    cf = lambda t: t.double().permute(0, 4, 1, 2, 3).contiguous()
    w = torch.zeros((cin, cout, 3, 3, 3) if mode == WC.DECONV else (cout, cin, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    for e in range(WC.ELEMENTS):
        w.grad = None
        xe = cf(x[e:e + 1])
        y = F.conv_transpose3d(xe, w, stride=2, padding=1, output_padding=1) if mode == WC.DECONV else F.conv3d(xe, w, stride=S, padding=1)
        assert y.shape == cf(gy[e:e + 1]).shape
        y.backward(cf(gy[e:e + 1]))
        assert gw[e].shape == w.grad.shape
        assert bool(((gw[e] - w.grad).abs() <= 1e-12 * sa[e]).all()), (name, e)
    assert not torch.equal(gw[0], gw[1]) and not torch.equal(gw[1], gw[2])


@pytest.mark.parametrize("name", list(WC.CASES))
def test_integer_data_keeps_fp32_exact(name):
    """Integers in -2..2: every entry of the reference is an integer and, at the largest batch, the sum of |products| per entry
    stays below 2^24, so fp32 products and fp32 sums in any order are exact."""
    sm, bg = WC.elements(name, "int")
    for t in (sm, bg):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and t.abs().max().item() == 2 and t.min().item() == -2
    gw, sa = WC.reduction(sm, bg, WC.sides(name)[0])
    assert torch.equal(gw, gw.round())
    B = max(r[0] for r in WC.REGIMES)
    assert WC.batch_counts(B).tolist() == [10, 10, 9]
    assert WC.batch_reference(sa, B).max().item() < 2 ** 24
    ref = WC.batch_reference(gw, B)
    assert torch.equal(ref.float().double(), ref) and ref.abs().max().item() > 0
