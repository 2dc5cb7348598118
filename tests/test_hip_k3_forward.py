"""K3 forward (ops.warp_variance, ops.warp_variance_f16, ops.homo_warp) on every path of the tile kernel (csrc/warp_variance_tile.hip)
and at every instantiation of the gather kernel (csrc/warp_variance.hip), at small shapes, on the product library alone.

The cases (tests/k3_forward_cases.py; tests/test_k3_forward_cpu.py checks on the CPU that each is what its label says).  Chunks of 8
planes per class, from the float64 restatement of the PROBE step, as window / gather / behind / marginal (a label counts a chunk only
with a margin: boxes 16 px away from the window size, a corner behind the camera by 1e-3 of the depth), for the fp32 window of
104 px and, in brackets, the fp16 window of 128 px:
  window_ragged    (2,5,9,17,2), far depths     24 / 0 / 0 / 0     [24 / 0 / 0 / 0]    tiles 8x4, 1x4, 8x1, 1x1; chunks 8 + 8 + 1; B = 2
  window_smallest  (1,2,2,1,1)                   1 / 0 / 0 / 0      [1 / 0 / 0 / 0]    one tile, one plane
  gather_only      (1,9,70,3,6), mild            0 / 27 / 0 / 0     [0 / 25 / 0 / 2]
  mixed            (1,13,22,40,4), 1/depth even 26 / 8 / 0 / 26    [48 / 0 / 0 / 12]   both passes inside one march of 5 chunks
  behind           (1,24,40,8,3), wide baseline  0 / 0 / 30 / 0     [0 / 0 / 30 / 0]   most samples leave the map
  all_three        (1,24,40,40,3), wide baseline 49 / 47 / 45 / 9  [55 / 40 / 45 / 10] one launch, marches of 5 chunks
  short_march      (1,13,22,72,11), far depths   81 / 0 / 0 / 27  [108 / 0 / 0 / 0]    nch = 7: chunk groups of 5 and 4, interleaved
  v32              (1,8,12,20,32), mild          7 / 2 / 0 / 3     [10 / 2 / 0 / 0]    nch = 1: three groups (fp16: nch = 8, one)
  xcd_8_tiles      (1,4,64,9,2), mild            9 / 6 / 0 / 1     [10 / 6 / 0 / 0]    8 tiles: one per XCD slot
  xcd_9_tiles      (1,4,66,9,2), mild            16 / 0 / 0 / 2    [18 / 0 / 0 / 0]    9 tiles: 7 of 16 slots idle
  batch_march      (2,9,30,65,11), mild          127 / 24 / 0 / 65 [189 / 14 / 0 / 13] B = 2 x 2 tiles per XCD slot x chunk groups of 5 and 4
C = 4, 8, 16 and 64 (warp_variance_kernel<1, 2, 4, 16>, which have no window path) run the window_ragged, mixed and behind geometries.

What is asserted, with white-noise float32 features, on the folded (default) and on the exact grid:
  1. EQUALITY OF FORMS, on the bits: tile kernel (channel-last) == gather kernel (NCDHW) at C = 32, both layouts of the gather kernel
     at the other C, staged maps == repacked maps, return_absmax returns the same volume and exactly ops.absmax(volume), and
     warp_variance_f16 on fp16-representable features == the fp32 tile kernel's volume rounded once.
  2. HARD BAND against the float64 restatement of the grid asked for: atol = rtol = 1e-4 (fp16: 2e-3), all outputs finite.
  3. SHARP BAND, exact grid only.  Reference: the restatement with the kernel's float32 positions (exact chain, on the transforms as
     compose_transforms_kernel rounds them) and a float64 blend: it shares the kernel's cells and weights.  e = the largest
     deviation of the all-float32 restatement from it, i.e. blend and summation rounding alone; asserted atol = 16 e, rtol = 1e-5
     (SHARP_MULTIPLE and SHARP_RTOL of test_hip_backward_shapes.py, for the reason given there: the kernel blends in fused
     multiply-adds and forms mean and variance with a reciprocal, the float32 restatement is one other such ordering).  e comes from
     the reference alone.  The folded grid has no such band: v_rcp_f32 moves a position by up to 1e-4 px, which on white noise is
     1e-4 of a feature's magnitude; there the equality of forms and the hard band carry the check.
  4. ops.homo_warp (the WARP_ONLY instantiations) at C = 4 .. 64 against homo_warp_restated in the hard band.  homo_warp has no
     exact_grid and a single layout, so it has neither a sharp band nor a second form to equal: the WARP_ONLY EXACT instantiations
     cannot be reached through any entry point.
  5. ONE-HOT VIEWS on all_three: with every source map but one zeroed, a view dropped or read twice in a march is an error of the
     size of the volume, not a 1/V share of one; the float64 reference differs from the key-only variance by more than 1e-2.

Measured on the MI355X, the largest max|diff| / e per kernel form (every comparison prints its own; run with -s):
  tile kernel          1.16  (batch_march: 5.11e-7 on 2.25, e 4.41e-7); short_march 1.10, all_three 1.00, one-hot views 1.00
  gather kernel <8>    1.16  (the same case: the two kernels' volumes are equal on the bits)
  gather kernel <1>    1.00  (C = 4)     <2>  1.06  (C = 8)     <4>  1.22  (C = 16)     <16>  1.46  (C = 64, window_ragged: 1.04e-6 on 5.9)
i.e. the kernels sit where a float32 evaluation of the reference sits; no case is near the 16.  Hard band: at most 9.8e-5 on a value
of 4.95 (folded grid, behind, C = 64; the float32 restatement itself deviates by as much there, from the positions of samples whose
Z nearly cancels); fp16 volume at most 1.5e-3 on 4.9; ops.homo_warp at most 1.0e-4 on 3.3.

A mutation check (not kept; before batch_march joined the table): with the depth table of a march taken from chunk jc instead of
chunk_of(jc), short_march and v32 fail here (and the V = 32 case of test_hip_shapes.py); with `locate`'s weights ux and wx exchanged, or inv_nv = 1 / V, every tile case here
fails; with the absmax by-product leaving out the fourth channel of each lane, only test_k3_forward_absmax_from_every_thread fails."""
import numpy as np
import pytest
import torch

import k3_forward_cases as K
from test_hip_backward_shapes import SHARP_MULTIPLE, SHARP_RTOL
from test_hip_f16 import bordered
from test_hip_shapes import ATOL, RTOL, T

pytestmark = pytest.mark.gpu
HARD = dict(atol=ATOL, rtol=RTOL)
HARD_F16 = dict(atol=2e-3, rtol=2e-3)  # test_hip_f16.py
C32 = [(name, exact) for name in K.CASES for exact in (False, True)]
OTHER = [(name, C, exact) for name in K.OTHER_CHANNEL_GEOMETRIES for C in K.OTHER_CHANNELS for exact in (False, True)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def check(got, refs, what, hard=HARD):
    """got (B,C,D,h,w) against the float64 reference in the hard band and, where the case has a sharp reference, within
    SHARP_MULTIPLE times that reference's own float32 error e"""
    want64, sharp, e = refs
    got = got.detach().float().cpu().numpy().astype(np.float64)
    diff = np.abs(got - want64).max()
    line = f"{what}: hard max |diff| {diff:.3e}, max |want| {np.abs(want64).max():.3e}"
    if sharp is not None:
        sdiff = np.abs(got - sharp).max()
        line += f"; sharp max |diff| {sdiff:.3e}, e {e:.3e}, max |diff| / e {sdiff / e:.2f}"
    print(line)
    assert np.isfinite(got).all(), what
    np.testing.assert_allclose(got, want64, err_msg=what + " (hard band)", **hard)
    if sharp is not None:
        assert e > 0
        np.testing.assert_allclose(got, sharp, atol=SHARP_MULTIPLE * e, rtol=SHARP_RTOL, err_msg=what + f" (sharp band, e = {e:.3e})")


def device_inputs(name, C, dev, half=False, hot=None):
    """the case's features (numpy) and its calibration on the device"""
    _, projs, key_inv, depth = K.case_inputs(name, C)
    return K.case_features(name, C, half, hot), ([T(p, dev) for p in projs], T(key_inv, dev), T(depth, dev))


def ncdhw(x):
    return x.permute(0, 4, 1, 2, 3)


def forms(feats, args, exact, what, dev):
    """the volume through every form of the entry point, each equal on the bits; returns the channel-last and the NCDHW volume"""
    from robustmvd_amd import ops
    ft = [T(f, dev) for f in feats]
    last = ops.warp_variance(ft[0], ft[1:], *args, channels_last=True, exact_grid=exact)
    first = ops.warp_variance(ft[0], ft[1:], *args, channels_last=False, exact_grid=exact)
    assert torch.equal(ncdhw(last), first), what + ": channel-last and NCDHW volumes differ"
    staged = [bordered(f, dev, torch.float32) for f in feats]
    for cl, vol in ((True, last), (False, first)):
        assert torch.equal(ops.warp_variance(staged[0], staged[1:], *args, channels_last=cl, exact_grid=exact, staged=True), vol), \
            what + f": staged maps, channels_last={cl}"
        v2, amax = ops.warp_variance(ft[0], ft[1:], *args, channels_last=cl, exact_grid=exact, return_absmax=True)
        assert torch.equal(v2, vol), what + f": return_absmax changes the volume, channels_last={cl}"
        assert torch.equal(amax, ops.absmax(vol)) and float(amax) == float(vol.abs().max()), what + f": absmax, channels_last={cl}"
    return last, first


@pytest.mark.parametrize("name,exact", C32, ids=lambda x: str(x))
def test_k3_forward_tile_and_gather(name, exact, dev):
    """C = 32: the channel-last call runs the tile kernel, the NCDHW call the gather kernel <8> (REUSE = 2 on the folded grid)"""
    feats, args = device_inputs(name, 32, dev)
    what = f"K3 {name} C=32 exact={exact}"
    last, first = forms(feats, args, exact, what, dev)
    refs = K.references(name, 32, exact)
    check(ncdhw(last), refs, what + " tile")
    check(first, refs, what + " gather")


@pytest.mark.parametrize("name,C,exact", OTHER, ids=lambda x: str(x))
def test_k3_forward_other_channel_counts(name, C, exact, dev):
    feats, args = device_inputs(name, C, dev)
    what = f"K3 {name} C={C} exact={exact}"
    last, first = forms(feats, args, exact, what, dev)
    refs = K.references(name, C, exact)
    check(ncdhw(last), refs, what + " gather NDHWC")
    check(first, refs, what + " gather NCDHW")


def test_k3_forward_absmax_from_every_thread(dev):
    """The cases' own maximum sits wherever the noise puts it (in none of the ten in the fourth channel of a lane's quad, so a tile
    kernel whose by-product left that channel out passed every form above).  Here one key feature at a time is raised to 50, for
    every pixel of the window_ragged map (ragged tiles included, both batch elements) with the channel stepping through all 32: the
    variance there is in the hundreds on every plane, and max |volume| has to come from that pixel's lane and wave, from whichever of
    the three chunks holds it; the gather kernel's separate pass sees the same volumes."""
    from robustmvd_amd import ops
    feats, args = device_inputs("window_ragged", 32, dev)
    ft = [T(f, dev) for f in feats]
    B, C, h, w = feats[0].shape
    for p in range(h * w):
        b, c, y, x = p % B, (7 * p + 3) % C, p // w, p % w
        key = ft[0].clone()
        key[b, c, y, x] = 50.0
        for cl in (True, False):
            vol, amax = ops.warp_variance(key, ft[1:], *args, channels_last=cl, return_absmax=True)
            peak = float((vol[b, :, y, x, c] if cl else vol[b, c, :, y, x]).abs().max())
            assert peak > 100.0 and float(amax) == peak == float(vol.abs().max()), (p, cl)
    assert {(7 * p + 3) % C for p in range(h * w)} == set(range(C))


@pytest.mark.parametrize("name", list(K.CASES))
def test_k3_forward_f16(name, dev):
    """the fp16 tile variant (window of 128 px, folded grid only) on fp16-representable features: the fp32 tile kernel's arithmetic
    and one rounding of the volume"""
    from robustmvd_amd import ops
    (B, h, w, D, V), *_ = K.CASES[name]
    feats, args = device_inputs(name, 32, dev, half=True)
    f32 = [bordered(f, dev, torch.float32) for f in feats]
    f16 = [bordered(f, dev, torch.float16) for f in feats]
    assert all(torch.equal(a.float(), b) for a, b in zip(f16, f32))
    want = ops.warp_variance(f32[0], f32[1:], *args, channels_last=True, staged=True)
    got = ops.warp_variance_f16(f16[0], f16[1:], *args)
    assert got.dtype == torch.float16 and tuple(got.shape) == (B, D, h, w, 32)
    assert torch.equal(got, want.half())
    refs = K.references(name, 32, False, half=True)
    check(ncdhw(want), refs, f"K3 {name} fp32 tile on fp16-representable features")
    check(ncdhw(got), refs, f"K3 {name} f16", HARD_F16)


@pytest.mark.parametrize("C", K.HOMO_WARP_CHANNELS)
@pytest.mark.parametrize("name", K.HOMO_WARP_GEOMETRIES)
def test_homo_warp_vs_restatement(name, C, dev):
    from robustmvd_amd import ops
    feats, projs, key_inv, depth = K.case_inputs(name, C)
    V = len(projs)
    some = 0.0
    for v in range(V):
        got = ops.homo_warp(T(feats[1 + v], dev), T(projs[v], dev), T(key_inv, dev), T(depth, dev))
        want64 = K.homo_warp_restated(feats[1 + v], projs[v], key_inv, depth, "folded", K.F64, K.F64)
        check(got, (want64, None, None), f"homo_warp {name} C={C} view {v}")
        some = max(some, np.abs(want64).max())
    assert some > 1.0  # the geometry warps something into view


@pytest.mark.parametrize("exact", [False, True])
def test_k3_forward_one_hot_views(exact, dev):
    from robustmvd_amd import ops
    name = "all_three"
    (B, h, w, D, V), *_ = K.CASES[name]
    base = K.key_only_variance(K.case_inputs(name)[0][0], D, V)
    for v in range(V):
        feats, args = device_inputs(name, 32, dev, hot=v)
        ft = [T(f, dev) for f in feats]
        refs = K.references(name, 32, exact, hot=v)
        assert np.abs(refs[0] - base).max() > 1e-2
        last = ops.warp_variance(ft[0], ft[1:], *args, channels_last=True, exact_grid=exact)
        first = ops.warp_variance(ft[0], ft[1:], *args, channels_last=False, exact_grid=exact)
        assert torch.equal(ncdhw(last), first)
        check(ncdhw(last), refs, f"K3 {name} exact={exact} only view {v} tile")
        check(first, refs, f"K3 {name} exact={exact} only view {v} gather")
