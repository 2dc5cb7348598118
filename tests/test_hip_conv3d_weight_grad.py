"""GPU tests of conv3d_weight_grad_kernel<COT, CIT, S> (csrc/conv3d_backward.hip, behind mvd_conv3d_weight_grad_f32) on its
marching and persistent paths: all eight instantiations, the channel counts off the network's grid and the three modes, each at
DZ = 1, 2, 4 and 8 planes per march (tests/wgrad_cases.py: the work items come from the batch, so the float64 reference stays
three small reductions).  Every test first asserts, through mvd_conv3d_weight_grad_plan_field, that the library runs the
instantiation and the regime it is about."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as WC
from test_hip_conv3d_backward import _check

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
_RID = lambda r: f"B{r[0]}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wgrad_elements():
    """per (case, kind), built on first use and shared by the regimes and tests: the three elements on the device and their
    float64 reductions (gw_e, sum of |products|_e) on the CPU; read-only; released with the module"""
    cache = {}

    def get(name, kind, dev):
        if (name, kind) not in cache:
            sm, bg = WC.elements(name, kind)
            cache[name, kind] = (sm.to(dev), bg.to(dev)) + WC.reduction(sm, bg, WC.sides(name)[0])
        return cache[name, kind]

    yield get
    cache.clear()


def _batch(name, sm, bg, B):
    """(x, gy) of B batch elements, element b being element b % 3"""
    idx = torch.arange(B, device=sm.device) % WC.ELEMENTS
    return WC.x_gy(name, sm[idx], bg[idx])


@pytest.mark.parametrize("regime", WC.REGIMES, ids=_RID)
@pytest.mark.parametrize("name", list(WC.CASES))
def test_weight_gradient_is_exact_on_integers(name, regime, dev, wgrad_elements):
    """x and gy integers in -2..2: every product and every partial sum is an integer below 2^24 (asserted), so the kernel's fp32
    products and sums are exact in any order and gw must equal the float64 reference bit for bit, in the layer's own layout.  A
    dropped or doubled voxel, a wrong tap, a stale ring slot or a wrong batch offset is an integer difference."""
    from robustmvd_amd import ops
    WC.assert_plan(name, regime)
    B = regime[0]
    mode = WC.CASES[name][0]
    sm, bg, gw_e, sa_e = wgrad_elements(name, "int", dev)
    ref = WC.batch_reference(gw_e, B)
    assert WC.batch_reference(sa_e, B).max().item() < 2 ** 24
    x, gy = _batch(name, sm, bg, B)
    got = ops.conv3d_weight_grad(x, gy, mode).cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    if not torch.equal(got.double(), ref):
        diff = got.double() - ref
        bad = diff.nonzero()
        rows = [f"[{','.join(map(str, i.tolist()))}] got {got[tuple(i)].item():.0f} want {ref[tuple(i)].item():.0f}" for i in bad[:12]]
        taps = sorted({tuple(i[2:].tolist()) for i in bad})
        pytest.fail(f"{name} {_RID(regime)} ({regime[3]}): {len(bad)} of {ref.numel()} entries differ, max |diff| {diff.abs().max().item():.0f}, "
                    f"{len(taps)} taps (kd,kh,kw) affected, first {taps[:6]}; entries [cs,cg,kd,kh,kw]: " + "; ".join(rows))


@pytest.mark.parametrize("name", WC.ROUNDING_CASES)
def test_weight_gradient_rounding_at_eight_plane_marches(name, dev, wgrad_elements):
    """CostRegNet's eleven layers and the three cases of the instantiations no layer reaches, gaussian x and gy, B = 29 (DZ = 8,
    522 items on 512 workgroups): the two assertions of test_hip_conv3d_backward._check against the float64 reduction — the hard
    bound (n + 2) u sum|products| with n = 29 x 9 x 9 x 33 = 77,517 (S = 1) or 29 x 9 x 9 x 17 = 39,933 (S = 2) voxels, and
    e_engine <= 4 e_vendor, the vendor being torch's fp32 backward on the GPU over the whole batch.
    Measured on an MI355X over the fourteen cases (e = max error / max |ref|): e_engine 8.5e-7 .. 1.8e-6, e_vendor 3.3e-7 .. 9.7e-7,
    worst error / hard bound 1.1e-5 .. 7.1e-5.  e_engine / e_vendor is 1.1 .. 1.7 in the stride-1 cases and 2.2 .. 3.9 where
    S = 2 (conv1 1.50e-6 / 3.85e-7 and stride 2 32 -> 16 1.77e-6 / 4.53e-7, both 3.9 of the 4 allowed): the engine's error is the
    same in both, the vendor's halves.  The engine adds 512 partials in one fp32 chain (conv3d_weight_grad_reduce_kernel)."""
    from robustmvd_amd import ops
    WC.assert_plan(name, WC.MARCH8)
    B = WC.MARCH8[0]
    mode, cin, cout = WC.CASES[name][:3]
    S = WC.sides(name)[0]
    sm, bg, gw_e, sa_e = wgrad_elements(name, "gauss", dev)
    x, gy = _batch(name, sm, bg, B)
    got = ops.conv3d_weight_grad(x, gy, mode)
    cf = lambda t: t.permute(0, 4, 1, 2, 3).contiguous()
    wv = torch.zeros((cin, cout, 3, 3, 3) if mode == WC.DECONV else (cout, cin, 3, 3, 3), device=dev, requires_grad=True)
    y = F.conv_transpose3d(cf(x), wv, stride=2, padding=1, output_padding=1) if mode == WC.DECONV else F.conv3d(cf(x), wv, stride=S, padding=1)
    y.backward(cf(gy))
    n = B * int(np.prod(WC.SMALL_DHW[S]))
    _check(f"{name} gw B={B}", got, WC.batch_reference(gw_e, B), WC.batch_reference(sa_e, B), n, wv.grad)


def _raw_call(name, x, gy, ws_bytes, gw_buf, ws_buf):
    from robustmvd_amd import ops
    mode, cin, cout = WC.CASES[name][:3]
    B, Di, hi, wi, _ = x.shape
    ops.call("mvd_conv3d_weight_grad_f32", x.device, x, gy, gw_buf, B, Di, hi, wi, cin, cout, mode, ws_buf, ws_bytes)


@pytest.mark.parametrize("name", WC.CONTRACT_CASES)
def test_call_contract_workspace_and_output_extents(name, dev, wgrad_elements):
    """mvd_conv3d_weight_grad_f32 through ops.call at DZ = 8, one case per S, gaussian data.  The workspace is the first
    workspace_bytes of a larger buffer, pre-filled with NaN, and gw the front of a larger buffer; behind both lies a sentinel
    tail.  gw is bit-identical to ops.conv3d_weight_grad (so every partial is written before the reduction reads it: a NaN
    would spread), both tails are untouched, and the same call with one byte less is refused with the workspace error before
    anything is written."""
    from robustmvd_amd import _lib as L
    from robustmvd_amd import ops
    WC.assert_plan(name, WC.MARCH8)
    B = WC.MARCH8[0]
    mode, cin, cout = WC.CASES[name][:3]
    sm, bg, _, _ = wgrad_elements(name, "gauss", dev)
    x, gy = _batch(name, sm, bg, B)
    x, gy = x.contiguous(), gy.contiguous()
    want = ops.conv3d_weight_grad(x, gy, mode)
    nbytes = int(L.load().mvd_conv3d_weight_grad_workspace_bytes(B, *x.shape[1:4], cin, cout, mode))
    assert nbytes > 0 and nbytes % 4 == 0
    tail = 4096
    ws = torch.full((nbytes // 4 + tail,), SENTINEL, dtype=torch.float32, device=dev)
    ws[:nbytes // 4] = float("nan")
    gw = torch.full((want.numel() + tail,), SENTINEL, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="workspace"):
        _raw_call(name, x, gy, nbytes - 1, gw, ws)
    torch.cuda.synchronize(dev)
    assert bool((gw == SENTINEL).all()) and bool((ws[nbytes // 4:] == SENTINEL).all()) and bool(ws[:nbytes // 4].isnan().all())
    _raw_call(name, x, gy, nbytes, gw, ws)
    assert torch.equal(gw[:want.numel()].view_as(want), want)
    assert not bool(want.isnan().any())
    assert bool((gw[want.numel():] == SENTINEL).all()), "gw written past its extent"
    assert bool((ws[nbytes // 4:] == SENTINEL).all()), "workspace written past workspace_bytes"


@pytest.mark.parametrize("regime", WC.REGIMES, ids=_RID)
@pytest.mark.parametrize("name", WC.CONTRACT_CASES)
def test_two_calls_give_the_same_bits(name, regime, dev, wgrad_elements):
    """no atomics, a fixed item order and a fixed order of the partials: in each regime two calls on gaussian data are torch.equal"""
    from robustmvd_amd import ops
    WC.assert_plan(name, regime)
    mode = WC.CASES[name][0]
    sm, bg, _, _ = wgrad_elements(name, "gauss", dev)
    x, gy = _batch(name, sm, bg, regime[0])
    a = ops.conv3d_weight_grad(x, gy, mode)
    b = ops.conv3d_weight_grad(x, gy, mode)
    assert torch.equal(a, b) and bool(a.isfinite().all()) and a.abs().max().item() > 0
