"""K1 forward (ops.sweep_corr, ops.sweep_corr_nhwc, ops.sweep_corr_autograd, ops.sweep_warp) on every path of the pixel-list kernel
sweep_corr_px_kernel<8, 16, 24, 32>, the cell kernel sweep_corr_kernel<1 .. 8> and sweep_warp_kernel (csrc/sweep_corr.hip, sampling
geometry in csrc/sweep_epipolar.h), at small shapes.

The cases (tests/k1_forward_cases.py; tests/test_k1_forward_cpu.py asserts on the CPU, from a restatement of the kernel's steps 2
and 3, that each is what its label says, and lists the counts):
  full_list   key 2x17, source 32x160, S 64, planes interleaved per pixel: 32 of 34 passes have 64 cells and a list of 256 pixels
  monotone    source 48x64, S 130, per-plane depths: up to 53 cells and 17 steps in a pass; odd and even step counts; tail of 2
  chain4      source 12x16, S 256, every pixel's planes shuffled: 1069 owner-2 taps, 460 in3 reloads, every pass revisits a cell
  invisible   pose (0.3, 1.5), S 70, V 3: 17 % and 58 % of two views' samples invisible with k_inf > 0; passes with no live sample
  turned      source camera turned by 100 degrees: k_inf < 0 on part of the key map, 11 % of the samples invisible there
  behind      the source camera 1.5 ahead of the key's: 74 % of view 0's samples lie behind it, and 55 % of all its samples are
              inside the map, so that the visibility term alone decides their mask
  far_planes  S 65, depths 50 .. 1000: the 64 planes of a pass share one cell, the tail of one plane continues the run
  layout      N 2 with its own planes each, key 3x21 (ragged second tile), source 5x9, V 3, 36 workgroups; all four borders
  pixel       the per-pixel jitter of test_sweep_grads_cpu.K1_CASES
  nonfinite   den == 0 exactly on one plane (positions +-inf and NaN), edge samples with inb >= 0.9999
full_list, chain4, invisible and behind run at C = 64 .. 512, i.e. at every instantiation of both kernels.

What is asserted, on white-noise float32 features:
  1. MASKS equal the restated ones exactly, nothing forgiven, and 0 < mean < 1 per view.
  2. HARD BAND against the float64 restatement: atol = rtol = 1e-4 (FORWARD of test_hip_backward_shapes.py), all outputs finite.
  3. SHARP BAND: the reference is sweep_corr_restated with float64 leaves (float32 positions, float64 blend and sum); e is the largest
     deviation of the same restatement with float32 leaves from it, so e comes from the reference alone; asserted atol = 16 e,
     rtol = 1e-5 (SHARP_MULTIPLE, SHARP_RTOL of test_hip_backward_shapes.py).
  4. EQUALITY OF FORMS, on the bits: two runs; sweep_corr_autograd under no_grad; per-pixel inverse depths that are constant on each
     plane against the (N,S) path; sweep_corr_nhwc (channel-last key, zero-bordered sources, destinations that are channel slices
     of wider buffers) with the neighbouring channels untouched and corr_absmax exactly max |corr| over three views.
  5. THE TWO KERNELS: the experiments library with MVD_K1_CELLS=1 runs sweep_corr_kernel<1 .. 4> on the C <= 256 cases: masks equal
     the pixel-list kernel's, values in the same sharp band against the same reference.
  6. ONE-HOT SOURCES on full_list and chain4: features zero except at one source pixel that the restated list serves through
     owner 1, owner 2, an in3 reload or its last place; a dot product taken from a wrong list place is then an error of the size of
     the output.  The reference is above 1e-3 on the planes that read the pixel through that cell, and zero (as is the kernel's
     output, exactly) on every sample without a tap on it.
  7. ops.sweep_warp on invisible, behind, pixel and nonfinite at C = 1, 5, 64, normalize_after False and True: masks equal the restated
     SAMPLING mask (no visibility term), values in both bands against sweep_warp_restated, masked samples exactly 0.

Measured on the MI355X, the largest max|diff| / e per kernel form (every comparison prints its own; run with -s), and the largest
max|diff| against the float64 reference (the hard band is 1e-4; outputs of magnitude 2 .. 3):
  sweep_corr_px_kernel  <8> 1.69 (chain4: 5.1e-7 on 2.8, e 3.0e-7)   <16> 1.98 (invisible: 4.0e-7, e 2.0e-7)   <24> 1.14   <32> 0.96
                        one-hot runs 1.10; hard band at most 5.1e-7
  sweep_corr_kernel     <1> 1.35   <2> 1.03   <3> 1.40   <4> 0.90 (experiments library)   <5> 1.40   <6> 1.26   <7> 1.36   <8> 0.99
                        hard band at most 5.2e-7 (chain4, C = 256)
  sweep_warp_kernel     2.38 (nonfinite, C = 1, normalize_after: 6.1e-8 on 1.0, e 2.6e-8); hard band at most 4.8e-7
i.e. every form sits where a float32 evaluation of the reference sits; no form is near the 16 and none needed a restatement in the
kernel's chain lengths.  The module runs in 5 s.

The mutation check (not kept; one change at a time in a copy of csrc/sweep_corr.hip, the product library rebuilt from it, the tests of
this module and the K1 tests from before it: test_hip_shapes.py::test_sweep_corr_vs_oracle, test_sweep_corr_backward_vs_restatement,
test_hip_parity.py, test_hip_backward.py and the channel-last test of test_hip_conv2d_split.py):
  (a) owner[k] = isnew ? 0 : 1         here: 33 fail, every case with owner-2 taps (monotone, chain4, invisible, behind, layout, pixel,
                                        turned at each C, against the reference and against the cell kernel) and the one-hot runs of
                                        chain4; full_list, far_planes and nonfinite pass, as they have (nearly) no such tap.
                                        Before: 25 fail too (all five test_sweep_corr_vs_oracle cases, all K1_CASES, the goldens):
                                        a monotone path of more than two cells already has owner-2 taps.
  (b) isnew = !in1                     here: 20 fail: full_list, chain4 and pixel at each C <= 256 and both one-hot tests.  Before:
                                        2 fail, the "pixel" case of K1_CASES and test_sweep_block_options_golden[pp-dim].
  (c) last MVD_WAVE_LDS_SYNC dropped   nothing fails, here or before: with this compiler the kernels' instruction streams are the same
                                        with and without it (the device assembly differs in the compile unit's id alone), so no
                                        test can tell them apart; the barrier only keeps a compiler from moving LDS accesses.
  (d) t.w[1] and t.w[2] exchanged      here: 46 fail, every case of the pixel-list kernel.  Before: 25 fail.
  (e) sweep_corr_mask without visible  here: 14 fail: behind at every C and nonfinite, the cases where the visibility term masks
                                        samples inside the map.  Before: NOTHING fails, the g2_sweep_behind golden included: in
                                        every earlier case the invisible samples are out of the map as well."""
import os

import numpy as np
import pytest
import torch

import k1_forward_cases as K
from test_hip_backward_shapes import FORWARD, SHARP_MULTIPLE, SHARP_RTOL
from test_hip_shapes import T

pytestmark = pytest.mark.gpu
OWN = [(name, K.case_shape(name)[1]) for name in K.CASES]
RUNS = OWN + [(name, C) for name in K.CHANNEL_GEOMETRIES for C in K.PX_CHANNELS + K.CELL_CHANNELS if (name, C) not in OWN]
PX_RUNS = [(name, C) for name, C in RUNS if C <= 256]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def check(got, ref, what):
    """got against the float64 reference in the hard band and within SHARP_MULTIPLE times the reference's own float32 error e"""
    want, e, _ = ref
    got = got.detach().cpu().numpy().astype(np.float64)
    diff = np.abs(got - want).max()
    print(f"{what}: max |diff| {diff:.3e}, max |want| {np.abs(want).max():.3e}, e {e:.3e}, max |diff| / e {diff / e if e > 0 else float(diff > 0):.2f}")
    assert np.isfinite(got).all(), what
    np.testing.assert_allclose(got, want, err_msg=what + " (hard band)", **FORWARD)
    np.testing.assert_allclose(got, want, atol=SHARP_MULTIPLE * e, rtol=SHARP_RTOL, err_msg=what + f" (sharp band, e = {e:.3e})")


def calibration(c, dev, inv=None):
    return T(c["Kk"], dev), [T(k, dev) for k in c["Ks"]], [T(t, dev) for t in c["Ts"]], T(c["inv"] if inv is None else inv, dev)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))


def run(name, C, dev, fs=None, inv=None):
    from robustmvd_amd import ops
    c = K.case_inputs(name, C)
    return ops.sweep_corr(T(c["fk"], dev), [T(f, dev) for f in (c["fs"] if fs is None else fs)], *calibration(c, dev, inv))


def against_reference(out, name, C, what, pick=None):
    corrs, masks = out
    for v, ref in enumerate(K.references(name, C, pick)):
        assert np.array_equal(masks[v].cpu().numpy(), ref[2]), f"{what}: mask of view {v}"
        check(corrs[v], ref, f"{what} corr{v}")


@pytest.mark.parametrize("name,C", RUNS, ids=lambda x: str(x))
def test_k1_forward_vs_restatement(name, C, dev):
    """C <= 256: sweep_corr_px_kernel<C / 8>; above: sweep_corr_kernel<C / 64>"""
    from robustmvd_amd import ops
    c = K.case_inputs(name, C)
    out = run(name, C, dev)
    against_reference(out, name, C, f"K1 {name} C={C}")
    for v, (_, _, mask) in enumerate(K.references(name, C)):
        assert 0 < mask.mean() < 1, v
    assert same(run(name, C, dev), out), "two runs differ"
    with torch.no_grad():
        assert same(ops.sweep_corr_autograd(T(c["fk"], dev), [T(f, dev) for f in c["fs"]], *calibration(c, dev)), out), "sweep_corr_autograd"


@pytest.mark.parametrize("name", ["layout", "monotone", "invisible"])
def test_k1_forward_plane_constant_per_pixel_depths(name, dev):
    """the per-pixel path (one load per lane from the (N,S,h,w) map) on inverse depths that are constant on each plane: the bits of
    the (N,S) path"""
    C = K.case_shape(name)[1]
    inv, per_pixel = K.plane_constant_invdepths(name)
    want = run(name, C, dev)
    assert same(run(name, C, dev, inv=inv), want)
    assert same(run(name, C, dev, inv=per_pixel), want)


@pytest.mark.parametrize("name", ["layout", "invisible"])
def test_k1_forward_nhwc_equals_planar(name, dev):
    """layout: N = 2, w = 21 (a ragged second tile), S = 70; invisible: w = 18, S = 70; both V = 3.  The destinations are channels
    3 .. 3 + S of buffers with S + 8 channels (out_pixel_stride = S + 8)"""
    from robustmvd_amd import ops
    N, C, h, w, hs, ws, S, V = K.case_shape(name)
    c = K.case_inputs(name)
    corrs, masks = run(name, C, dev)
    key_cl = T(c["fk"], dev).permute(0, 2, 3, 1).contiguous()
    bordered = []
    for f in c["fs"]:
        b = torch.zeros(N, hs + 3, ws + 3, C, device=dev)
        b[:, 1:hs + 1, 1:ws + 1] = T(f, dev).permute(0, 2, 3, 1)
        bordered.append(b)
    big_c, big_m = torch.full((V, N, h, w, S + 8), 7.0, device=dev), torch.full((V, N, h, w, S + 8), -7.0, device=dev)
    c2, m2 = [big_c[v, ..., 3:3 + S] for v in range(V)], [big_m[v, ..., 3:3 + S] for v in range(V)]
    cam = torch.zeros(1, device=dev)
    ops.sweep_corr_nhwc(key_cl, bordered, *calibration(c, dev), c2, m2, corr_absmax=cam)
    peaks = [float(x.abs().max()) for x in corrs]
    assert V == 3 and float(cam) == max(peaks) and max(peaks) > min(peaks)
    for v in range(V):
        assert torch.equal(c2[v].permute(0, 3, 1, 2), corrs[v]) and torch.equal(m2[v].permute(0, 3, 1, 2), masks[v])
    for big, fill in ((big_c, 7.0), (big_m, -7.0)):
        assert bool((big[..., :3] == fill).all()) and bool((big[..., 3 + S:] == fill).all())
    # without the by-product, and with a slot that is already higher
    cam2 = torch.full((1,), 1e3, device=dev)
    ops.sweep_corr_nhwc(key_cl, bordered, *calibration(c, dev), c2, m2, corr_absmax=cam2)
    assert float(cam2) == 1e3
    big_c.fill_(7.0)
    ops.sweep_corr_nhwc(key_cl, bordered, *calibration(c, dev), c2, m2)
    assert all(torch.equal(c2[v].permute(0, 3, 1, 2), corrs[v]) for v in range(V))


def _exp_or_skip():
    from robustmvd_amd import _lib as L
    if not os.path.exists(L.EXP_LIB_PATH):
        pytest.skip("the experiments library is not built (make -C robustmvd_amd/csrc exp)")
    return L


@pytest.mark.parametrize("name,C", PX_RUNS, ids=lambda x: str(x))
def test_k1_cell_kernel_against_pixel_list_kernel(name, C, dev, monkeypatch):
    """sweep_corr_kernel<1 .. 4> (experiments library, MVD_K1_CELLS=1) on the cases of sweep_corr_px_kernel: equal masks, the same
    sharp band against the same reference (the dot products are summed in another order)"""
    L = _exp_or_skip()
    product = run(name, C, dev)
    with L.use_experiments_library():
        assert same(run(name, C, dev), product), "the experiments library's pixel-list kernel"
        monkeypatch.setenv("MVD_K1_CELLS", "1")
        cells = run(name, C, dev)
        monkeypatch.delenv("MVD_K1_CELLS")
    assert all(torch.equal(a, b) for a, b in zip(cells[1], product[1]))
    assert not all(torch.equal(a, b) for a, b in zip(cells[0], product[0])), "MVD_K1_CELLS=1 ran the same kernel"
    against_reference(cells, name, C, f"K1 {name} C={C} cell kernel")


@pytest.mark.parametrize("name", ["full_list", "chain4"])
def test_k1_forward_one_hot_sources(name, dev):
    C = K.case_shape(name)[1]
    picks = K.one_hot_picks(name)
    assert len(picks) >= 4
    for pick in picks:
        n, v, y, x, p, j, k, kind, (yy, xx), planes = pick
        refs = K.references(name, C, pick)
        want = refs[v][0]
        hit = K.readers(name, v, n, yy, xx)
        assert (want[~hit] == 0).all() and max(abs(want[n, s, y, x]) for s in planes) > 1e-3, pick
        out = run(name, C, dev, fs=K.one_hot_sources(name, C, pick))
        assert bool((out[0][v].cpu()[torch.from_numpy(~hit)] == 0).all()), pick
        against_reference(out, name, C, f"K1 {name} one-hot {kind} pixel {(yy, xx)} key {(y, x)} pass {p} cell {j} tap {k}", pick)


@pytest.mark.parametrize("normalize_after", [False, True])
@pytest.mark.parametrize("C", K.WARP_CHANNELS)
@pytest.mark.parametrize("name", K.WARP_GEOMETRIES)
def test_sweep_warp_vs_restatement(name, C, normalize_after, dev):
    from robustmvd_amd import ops
    c = K.case_inputs(name, C)
    warped, masks = ops.sweep_warp([T(f, dev) for f in c["fs"]], *calibration(c, dev), c["key_size"], normalize_after)
    refs = K.warp_references(name, C, normalize_after)
    corr_masks = [m for _, _, m in K.references(name)]
    for v, ref in enumerate(refs):
        mask = ref[2]
        assert np.array_equal(masks[v].cpu().numpy(), mask), f"mask of view {v}"
        assert np.array_equal(mask, K.chains(name)[v]["mask"]) and 0 < mask.mean() < 1 and (mask >= corr_masks[v]).all()
        check(warped[v], ref, f"warp-only {name} C={C} normalize_after={normalize_after} view {v}")
        dead = torch.from_numpy(mask == 0)[:, :, None].expand(-1, -1, C, -1, -1)
        assert bool((warped[v].cpu()[dead] == 0).all())
    if "visibility_decides" in K.CASES[name][5]:  # the visibility term is NOT applied: samples are live here that K1's mask drops
        assert any((m > cm).any() for (_, _, m), cm in zip(refs, corr_masks))
    # fully masked samples (every tap out of the map: the norm is 0) are among the dead ones
    assert any((K.chains(name)[v]["inb"] == 0).any() for v in range(len(refs)))
