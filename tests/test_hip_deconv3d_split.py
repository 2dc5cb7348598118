"""The transposed layers' split-operand kernel (csrc/deconv3d_split.hip: ops.pack_deconv3d_weights_split / ops.deconv3d_bn_relu_split)
against a float64 transposed convolution of the same fp32 data, gated by the fp32-MFMA kernel's own error (the gate of
tests/test_hip_f16.py: max |error| of the new kernel <= 1.5 x max |error| of ops.conv3d_bn_relu, mode DECONV3D_STRIDE2).

Shapes (B, Di, hi, wi): (2, 3, 6, 19) = a batch of two, a partial row tile (6 = 4 + 2), a partial column tile and the + 1 halo column
inside the volume (19 = 16 + 3), the last plane (plane zd + 1 beyond the volume); (1, 2, 4, 33) = whole row tiles, 33 = two / one
column tiles + 1 column.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_common as gc

pytestmark = pytest.mark.gpu

PAIRS = [(64, 32), (32, 16), (16, 8)]
SHAPES = [(2, 3, 6, 19), (1, 2, 4, 33)]
GATE = 1.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(cin, cout, shape, amag=1.0, wmag=1.0, bad=False):
    """Inputs of one layer (fp32, read-only) and its float64 results before the affine: x (B,Di,hi,wi,cin) channel-last,
    wt (cin,cout,3,3,3) with per-output-channel magnitudes 64 x apart, scale, shift, skip, conv64 (B,2Di,2hi,2wi,cout)."""
    B, Di, hi, wi = shape
    rng = np.random.default_rng(cin * 1000 + cout + Di * 7 + wi)
    x = (rng.standard_normal((B, Di, hi, wi, cin)) * amag).astype(np.float32)
    if bad:
        x[0, Di - 1, 1, 2, 5] = np.inf
        x[B - 1, 0, hi - 1, wi - 2, 3] = np.nan
    wt = rng.standard_normal((cin, cout, 3, 3, 3)) * np.sqrt(2 / (cin * 27)) * wmag
    wt[:, 1] /= 8.0
    wt[:, 3] *= 8.0
    wt = wt.astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    skip = rng.standard_normal((B, 2 * Di, 2 * hi, 2 * wi, cout)).astype(np.float32)
    conv64 = F.conv_transpose3d(torch.from_numpy(x).double().permute(0, 4, 1, 2, 3), torch.from_numpy(wt).double(), stride=2, padding=1,
                                output_padding=1).permute(0, 2, 3, 4, 1).numpy()
    for a in (x, wt, scale, shift, skip, conv64):
        a.setflags(write=False)
    return x, wt, scale, shift, skip, conv64


def ref64(c, relu, use_skip, scale=None, shift=None):
    x, wt, sc, sh, skip, conv64 = c
    sc = sc if scale is None else scale
    sh = sh if shift is None else shift
    with np.errstate(invalid="ignore", over="ignore"):
        y = conv64 * sc.astype(np.float64) + sh.astype(np.float64)
        if relu:
            y = np.where(np.isnan(y), y, np.maximum(y, 0.0))
        if use_skip:
            y = y + skip.astype(np.float64)
    return y


def T(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # a copy: the cached inputs are read-only


def run_both(c, cin, cout, relu, use_skip, dev, scale=None, shift=None, return_absmax=False):
    """(new kernel's output, fp32-MFMA kernel's output[, max |y| of the new kernel]) as float64 numpy / a device tensor"""
    from robustmvd_amd import ops, _lib as L
    x, wt, sc, sh, skip, _ = c
    sc = sc if scale is None else scale
    sh = sh if shift is None else shift
    xt, wtt, sct, sht = T(x, dev), T(wt, dev), T(sc, dev), T(sh, dev)
    skt = T(skip, dev) if use_skip else None
    new = ops.deconv3d_bn_relu_split(xt, ops.absmax(xt), ops.pack_deconv3d_weights_split(wtt), cin, cout, sct, sht, relu=relu, skip=skt,
                                     return_absmax=return_absmax)
    w32, _, _ = ops.pack_conv3d_weights(wtt, L.DECONV3D_STRIDE2)
    base = ops.conv3d_bn_relu(xt, w32, cin, cout, sct, sht, L.DECONV3D_STRIDE2, relu=relu, skip=skt)
    if return_absmax:
        return new[0], base, new[1]
    return new.cpu().numpy().astype(np.float64), base.cpu().numpy().astype(np.float64)


def check_gate(new, base, ref, what):
    assert new.shape == ref.shape
    err_n, err_b = np.abs(new - ref).max(), np.abs(base - ref).max()
    mag = np.abs(ref).max()
    print(f"{what}: split {err_n / mag:.2e}  fp32-MFMA {err_b / mag:.2e} (max |error| relative to max |y|)")
    assert np.isfinite(base).all() and np.isfinite(new).all()
    assert err_n <= GATE * err_b, (err_n, err_b)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("use_skip", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_against_float64(cin, cout, shape, use_skip, relu, dev):
    c = case(cin, cout, shape)
    new, base = run_both(c, cin, cout, relu, use_skip, dev)
    check_gate(new, base, ref64(c, relu, use_skip), f"{cin}->{cout} {shape} skip={use_skip} relu={relu}")


@pytest.mark.parametrize("wmag", [1e-7, 1.0, 1e6])
@pytest.mark.parametrize("amag", [1e-30, 1.0, 1e30])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_range(cin, cout, amag, wmag, dev):
    """activations of magnitude 1e-30 .. 1e30, weights of 1e-7 .. 1e6 with channels 64 x apart: the power-of-two scalings make
    the error independent of both (no affine, no ReLU: the convolution itself)"""
    c = case(cin, cout, SHAPES[0], amag, wmag)
    one, zero = np.ones(cout, np.float32), np.zeros(cout, np.float32)
    new, base = run_both(c, cin, cout, False, False, dev, one, zero)
    check_gate(new, base, ref64(c, False, False, one, zero), f"{cin}->{cout} amag {amag:g} wmag {wmag:g}")


@pytest.mark.parametrize("cin,cout", PAIRS)
def test_non_finite_inputs(cin, cout, dev):
    """one inf and one NaN input value (no ReLU: fmaxf(NaN, 0) is 0 on either kernel, NaN in the reference): whatever the
    reference makes non-finite is non-finite; whatever the fp32 kernel leaves finite is finite and within the gate"""
    c = case(cin, cout, SHAPES[0], 1.0, 1.0, True)
    new, base = run_both(c, cin, cout, False, True, dev)
    ref = ref64(c, False, True)
    bad_ref, ok_base = ~np.isfinite(ref), np.isfinite(base)
    assert bad_ref.any() and ok_base.any()
    assert not np.isfinite(new[bad_ref]).any()
    assert np.isfinite(new[ok_base]).all()
    err_n, err_b = np.abs(new[ok_base] - ref[ok_base]).max(), np.abs(base[ok_base] - ref[ok_base]).max()
    print(f"{cin}->{cout} non-finite input: split {err_n:.2e}  fp32-MFMA {err_b:.2e}; finite outputs {ok_base.mean():.2f}")
    assert err_n <= GATE * err_b, (err_n, err_b)


@pytest.mark.parametrize("bad", [False, True])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_absmax_by_product(cin, cout, bad, dev):
    """max |y| over the finite outputs after the skip addition, bit for bit (a maximum: no arithmetic), and the same output bits
    as the plain variant"""
    from robustmvd_amd import ops
    c = case(cin, cout, SHAPES[0], 1.0, 1.0, bad)
    y, _, ya = run_both(c, cin, cout, not bad, True, dev, return_absmax=True)
    assert tuple(ya.shape) == (1,)
    assert torch.equal(ya, ops.absmax(y))
    assert float(ya) > 0 and np.isfinite(float(ya))
    x, wt, sc, sh, skip, _ = c
    xt = T(x, dev)
    plain = ops.deconv3d_bn_relu_split(xt, ops.absmax(xt), ops.pack_deconv3d_weights_split(T(wt, dev)), cin, cout, T(sc, dev), T(sh, dev),
                                       relu=not bad, skip=T(skip, dev))
    assert torch.equal(plain.view(torch.int32), y.view(torch.int32))
    # a caller-supplied slot is raised, not overwritten
    slot = torch.full((1,), 3.0e38, dtype=torch.float32, device=dev)
    ops.deconv3d_bn_relu_split(xt, ops.absmax(xt), ops.pack_deconv3d_weights_split(T(wt, dev)), cin, cout, T(sc, dev), T(sh, dev),
                               relu=not bad, skip=T(skip, dev), return_absmax=True, out_absmax=slot)
    assert float(slot) == np.float32(3.0e38)


@pytest.mark.parametrize("cin,cout", PAIRS)
def test_deterministic(cin, cout, dev):
    c = case(cin, cout, SHAPES[0])
    a = run_both(c, cin, cout, True, True, dev, return_absmax=True)
    b = run_both(c, cin, cout, True, True, dev, return_absmax=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[2], b[2])


def test_unsupported_channels_are_an_error(dev):
    from robustmvd_amd import ops
    with pytest.raises(ValueError, match="not built"):
        ops.pack_deconv3d_weights_split(torch.zeros(8, 8, 3, 3, 3, device=dev))


def test_model_against_float64(dev):
    """CostRegNet at (1, 16, 16, 24): the default path (conv7 and conv9 on the new kernel) against the module's own forward_autograd
    in float64 on the CPU, no further from it than 1.5 x CostRegNet(conv0_split=False) (every layer on fp32 arithmetic)"""
    import robustmvd_amd as R
    from test_oracle_golden import costreg_shapes
    sd = {k: torch.from_numpy(v) for k, v in gc.fill_state_dict(costreg_shapes(), 77).items()}

    def net(**kw):
        m = R.CostRegNet(**kw).eval()
        full = m.state_dict()
        full.update(sd)
        m.load_state_dict(full)
        return m

    x = torch.from_numpy(np.abs(gc.rng_array(78, (1, 32, 16, 16, 24), 0.7)))
    with torch.no_grad():
        ref = net().double().forward_autograd(x.double()).numpy()
    new_net = net().to(dev)
    assert "conv7_dsplit" in new_net._prepare() and "conv9_dsplit" in new_net._prepare()
    new = new_net(x.to(dev)).cpu().numpy().astype(np.float64)
    base = net(conv0_split=False).to(dev)(x.to(dev)).cpu().numpy().astype(np.float64)
    err_n, err_b = np.abs(new - ref).max(), np.abs(base - ref).max()
    print(f"CostRegNet: default path {err_n:.2e}  conv0_split=False {err_b:.2e} (max |error|, max |y| {np.abs(ref).max():.2e})")
    assert err_n <= GATE * err_b, (err_n, err_b)
