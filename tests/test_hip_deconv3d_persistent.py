"""The persistent, software-pipelined form of the transposed layers' split-operand kernel (deconv3d_split_persist_kernel in
csrc/deconv3d_split.hip: a workgroup walks several tiles with the next slab prefetched, its weights resident or requested steps
ahead, one max-|y| atomic at its end).

Experiments library: the forms selected by MVD_DS_PERSIST (1 = the product rule, 3 = three workgroups, which cross plane, batch and
channel-block boundaries and get unequal tile counts) and MVD_DS_LA (the layer's other look-ahead) are bit-identical to one tile per
workgroup (MVD_DS_PERSIST=0), max |y| included, because every output is the same sum in the same order; with one inf and one NaN
input exactly the same outputs are non-finite.  The tiles no layer runs at (MVD_DS_CFG: three column tiles per wave, two at 32
channels, two channel tiles per workgroup) give the bits of the layer's own tile, one tile per workgroup each.

Product library: per channel pair a long, narrow volume with more tiles than any persistent grid holds (at most 256 CUs x 4
workgroups = 1024), with a ragged row tile and a ragged column tile, against the float64 transposed convolution with the gate of
test_hip_deconv3d_split.py: max |error| <= 1.5 x that of ops.conv3d_bn_relu on the same data; max |y| equals y.abs().max(); the
memory on either side of y is untouched."""
import os

import pytest
import torch
import torch.nn.functional as F

from test_hip_deconv3d_split import GATE, PAIRS, SHAPES, T, case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _exp_or_skip():
    from robustmvd_amd import _lib as L
    if not os.path.exists(L.EXP_LIB_PATH):
        pytest.skip("the experiments library is not built (make -C robustmvd_amd/csrc exp)")
    return L


def _run(c, cin, cout, relu, use_skip, with_absmax, dev):
    """-> (y bits, max |y| bits or None)"""
    from robustmvd_amd import ops
    x, wt, sc, sh, skip, _ = c
    xt = T(x, dev)
    out = ops.deconv3d_bn_relu_split(xt, ops.absmax(xt), ops.pack_deconv3d_weights_split(T(wt, dev)), cin, cout, T(sc, dev), T(sh, dev),
                                     relu=relu, skip=T(skip, dev) if use_skip else None, return_absmax=with_absmax)
    if with_absmax:
        return out[0].view(torch.int32), out[1].view(torch.int32)
    return out.view(torch.int32), None


@pytest.mark.parametrize("bad", [False, True])
@pytest.mark.parametrize("with_absmax", [True, False])
@pytest.mark.parametrize("use_skip", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_persistent_forms_equal_one_tile_per_workgroup(cin, cout, shape, use_skip, with_absmax, bad, dev, monkeypatch):
    L = _exp_or_skip()
    c = case(cin, cout, shape, 1.0, 1.0, bad)
    relu = not bad  # fmaxf(NaN, 0) is 0: without the ReLU the bad input reaches the output
    monkeypatch.setenv("MVD_DS_PERSIST", "0")
    monkeypatch.delenv("MVD_DS_LA", raising=False)
    with L.use_experiments_library():
        ref, ref_amax = _run(c, cin, cout, relu, use_skip, with_absmax, dev)
    finite = torch.isfinite(ref.view(torch.float32))
    assert bool(finite.any()) and bool((~finite).any()) == bad
    for la in (None, "1", "2"):  # the layer's own look-ahead, then the two values one of which selects its other instance
        if la is not None:
            monkeypatch.setenv("MVD_DS_LA", la)
        for v in ("1", "3"):
            monkeypatch.setenv("MVD_DS_PERSIST", v)
            with L.use_experiments_library():
                got, amax = _run(c, cin, cout, relu, use_skip, with_absmax, dev)
            what = f"MVD_DS_PERSIST={v} MVD_DS_LA={la}"
            assert torch.equal(got, ref), what  # as int32: NaN counts
            assert torch.equal(torch.isfinite(got.view(torch.float32)), finite), what
            if with_absmax:
                assert torch.equal(amax, ref_amax), what


# (cin, cout, MVD_DS_CFG = 10 NT + MT): the tiles of the experiments library that no layer runs at: MT = 3, MT = 2 at 32 channels, NT = 2
OTHER_TILES = [(16, 8, 13), (32, 16, 12), (64, 32, 21)]
# (1, 2, 5, 50): for 48 input columns per tile a whole tile whose halo column lies inside the volume and a tile with two live
# columns, for 32 columns per tile 32 + 18; five rows leave a row tile with one live row
TILE_SHAPES = SHAPES + [(1, 2, 5, 50)]


@pytest.mark.parametrize("bad", [False, True])
@pytest.mark.parametrize("shape", TILE_SHAPES)
@pytest.mark.parametrize("cin,cout,cfg", OTHER_TILES)
def test_other_tiles_equal_shipped_tile(cin, cout, cfg, shape, bad, dev, monkeypatch):
    """One tile per workgroup (MVD_DS_PERSIST=0), with the skip and max |y|: the tile MVD_DS_CFG selects gives the bits of the
    layer's own tile, max |y| included, and with one inf and one NaN input the same outputs are non-finite.  NT and MT decide which
    wave holds an output, not its sum: the K content and the order of an output's MFMAs are fixed by (step, kw, K step)."""
    L = _exp_or_skip()
    c = case(cin, cout, shape, 1.0, 1.0, bad)
    relu = not bad  # fmaxf(NaN, 0) is 0: without the ReLU the bad input reaches the output
    monkeypatch.setenv("MVD_DS_PERSIST", "0")
    monkeypatch.delenv("MVD_DS_LA", raising=False)
    monkeypatch.delenv("MVD_DS_CFG", raising=False)
    with L.use_experiments_library():
        ref, ref_amax = _run(c, cin, cout, relu, True, True, dev)
    finite = torch.isfinite(ref.view(torch.float32))
    assert bool(finite.any()) and bool((~finite).any()) == bad
    monkeypatch.setenv("MVD_DS_CFG", str(cfg))
    with L.use_experiments_library():
        got, amax = _run(c, cin, cout, relu, True, True, dev)
    assert torch.equal(got, ref)  # as int32: NaN counts
    assert torch.equal(torch.isfinite(got.view(torch.float32)), finite)
    assert torch.equal(amax, ref_amax)


# (cin, cout) -> (Di, hi, wi): Di planes of 2 x 2 tiles (conv11: 3 x 2), the last row tile and the last column tile ragged, and
# more tiles than 1024 workgroups: 64 -> 32: 2 channel blocks x 136 x 2 x 2 = 1088; 32 -> 16: 264 x 2 x 2 = 1056; 16 -> 8 (tiles of
# 4 x 32): 180 x 3 x 2 = 1080.  The largest tensor is the float64 reference of 16 -> 8: 360 x 20 x 80 x 8 doubles = 37 MB.
LONG = {(64, 32): (136, 6, 20), (32, 16): (264, 6, 20), (16, 8): (180, 10, 40)}
GUARD = 4096  # floats on either side of y


@pytest.mark.parametrize("cin,cout", PAIRS)
def test_product_library_walks_many_tiles(cin, cout, dev):
    from robustmvd_amd import ops, _lib as L
    Di, hi, wi = LONG[(cin, cout)]
    g = torch.Generator().manual_seed(cin * 100 + cout)
    x = torch.randn(1, Di, hi, wi, cin, generator=g)
    wt = torch.randn(cin, cout, 3, 3, 3, generator=g) * (2.0 / (cin * 27)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    skip = torch.randn(1, 2 * Di, 2 * hi, 2 * wi, cout, generator=g)
    ref = F.conv_transpose3d(x.double().permute(0, 4, 1, 2, 3), wt.double(), stride=2, padding=1, output_padding=1).permute(0, 2, 3, 4, 1)
    ref = F.relu(ref * scale.double() + shift.double()) + skip.double()

    xt, wtt, sct, sht, skt = (a.to(dev) for a in (x, wt, scale, shift, skip))
    n = skip.numel()
    buf = torch.full((n + 2 * GUARD,), -3.0, device=dev)
    y = buf[GUARD:GUARD + n].view(skip.shape)
    amax = torch.zeros(1, device=dev)
    ops.call("mvd_deconv3d_bn_relu_f32_split", dev, xt, ops.absmax(xt), ops.pack_deconv3d_weights_split(wtt), sct, sht, skt, y, amax,
             1, Di, hi, wi, cin, cout, 1)
    w32, _, _ = ops.pack_conv3d_weights(wtt, L.DECONV3D_STRIDE2)
    base = ops.conv3d_bn_relu(xt, w32, cin, cout, sct, sht, L.DECONV3D_STRIDE2, relu=True, skip=skt)

    err_n, err_b = float((y.double().cpu() - ref).abs().max()), float((base.double().cpu() - ref).abs().max())
    mag = float(ref.abs().max())
    print(f"{cin}->{cout} {Di}x{hi}x{wi}: split {err_n / mag:.2e}  fp32-MFMA {err_b / mag:.2e} (max |error| relative to max |y|)")
    assert bool(torch.isfinite(y).all())
    assert err_n <= GATE * err_b, (err_n, err_b)
    assert float(amax) == float(y.abs().max())
    assert float(buf[:GUARD].min()) == -3.0 and float(buf[:GUARD].max()) == -3.0
    assert float(buf[GUARD + n:].min()) == -3.0 and float(buf[GUARD + n:].max()) == -3.0
    # without the max-|y| by-product (the other template variant): the same bits
    y2 = ops.deconv3d_bn_relu_split(xt, ops.absmax(xt), ops.pack_deconv3d_weights_split(wtt), cin, cout, sct, sht, relu=True, skip=skt)
    assert torch.equal(y2.view(torch.int32), y.view(torch.int32))
