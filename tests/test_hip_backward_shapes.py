"""Shape sweep of the sweep operators' VJP kernels (csrc/backward.hip) against float64, at every instantiation:
K1 backward <1>..<4> with one to four passes of the lane = plane loop, dead-lane tails, cells pending across a pass boundary, the
three inverse-depth modes, source maps of another size, N > 1 and a caller's corr_scale; the warp-only backward with C off the
multiples of 64; K2 backward over V x S with fully masked pixels and saturated scores; K3 backward (atomic and gather) at
lpp = 1 and 16 and partial chunks of planes.  tests/test_hip_backward.py holds the golden corner of each.

References: K1 and warp-only, the float64 restatement of tests/test_sweep_grads_cpu.py (which pins it against g10_grads.npz,
g15_sweep_grads.npz and the oracle, and checks that no sample of a case sits on a decision boundary of the float32 chain: the
forward masks must therefore EQUAL the restated ones); K2 and K3, the oracle's VJPs.

Two bands, both asserted.  HARD: the project's bands (K1 / warp-only atol 2e-4 rtol 1e-4; K2 3e-4 / 2e-3; K3 3e-4 / 1e-3, its only
band: the K3 oracle rounds its intermediate to float32).  SHARP (K1, warp-only, K2): the same reference evaluated in float32 on the
CPU deviates from its float64 self by at most e per output; the kernel must be within atol = 16 e, rtol = 1e-5.  Sixteen: the
kernel sums up to S x V terms in another order, in fused multiply-adds, its atomics arrive in any order and the device's expf is
not numpy's, while the CPU float32 evaluation is one such ordering: a single-digit multiple of e is plain rounding, two orders of
magnitude are not.  One-hot cotangents (a single plane, or the two planes either side of a pass boundary) make a dropped plane a
100 % error instead of one term of a sum; each asserts that the reference gradient is non-zero.

Measured on the MI355X, the largest max|diff| / e per kernel (every comparison prints its own; run with -s):
  K1 backward         4.1  (d key of the (2,128,6,7,5,9,70,2) case: 1.35e-6 on 2.5, e 3.3e-7); one-hot cases <= 1.8
  warp-only backward  1.7  (C = 1, S = 5: 2.9e-7 on 2.1, e 1.7e-7); one-hot cases <= 1.2
  K2 backward         6.5  at score spread 3 (d score, V = 32, S = 1: 3.5e-8 on 0.27, e 5.5e-9).  At spread 30 one d score
                      output whose e is 1.8e-11 shows 19.8: 3.5e-10 on 1.6e-3, 2e-7 RELATIVE, a few float32 roundings of the value
                      itself; that is inside the rtol term, so no case needed a larger multiple.
  K3 backward         hard band only: at most 1.1e-5 on gradients of magnitude 10 (atomic, C = 64, D = 17)."""
import functools

import numpy as np
import pytest
import torch

import test_sweep_grads_cpu as RS
from oracle import mvd_oracle as O
from test_hip_shapes import mvs_inputs
from test_hip_sweep_grads import GOLD, RAGGED, T

pytestmark = pytest.mark.gpu
K2_HARD = dict(atol=3e-4, rtol=2e-3)   # test_learned_fusion_backward_golden
FORWARD = dict(atol=1e-4, rtol=1e-4)   # test_hip_shapes.py
SHARP_MULTIPLE, SHARP_RTOL = 16, 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def check(got, want64, want32, what, hard, multiple=SHARP_MULTIPLE):
    """got against the float64 reference in the hard band and, where a float32 evaluation of the reference is given, within
    `multiple` times that evaluation's own error e."""
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    diff = np.abs(got - want64).max()
    line = f"{what}: max |diff| {diff:.3e}, max |want| {np.abs(want64).max():.3e}"
    if want32 is not None:
        e = np.abs(want32 - want64).max()
        line += f", e {e:.3e}, max |diff| / e {diff / e if e > 0 else float(diff > 0):.2f}"
    print(line)
    assert np.isfinite(got).all(), what
    np.testing.assert_allclose(got, want64, err_msg=what + " (hard band)", **hard)
    if want32 is not None:
        np.testing.assert_allclose(got, want64, atol=multiple * e, rtol=SHARP_RTOL, err_msg=what + f" (sharp band, e = {e:.3e})")


def gpu_grads(outs, cots, inputs, dev):
    loss = sum((o * T(c, dev)).sum() for o, c in zip(outs, cots))
    return torch.autograd.grad(loss, inputs, retain_graph=True)


def select_planes(cots, planes):
    out = [np.zeros_like(c) for c in cots]
    for o, c in zip(out, cots):
        o[:, list(planes)] = c[:, list(planes)]
    return out


class Restated:
    """One case's restatement, evaluated once with float64 and once with float32 leaves; grads(cots) differentiates both."""
    def __init__(self, c, forward):
        self.c = c
        self.leaves = {dt: [leaf(f) for f in ([c["fk"]] if c["fk"] is not None else []) + c["fs"]] for dt, leaf in
                       ((64, RS.leaf64), (32, RS.leaf32))}
        self.outs = {dt: forward(lv) for dt, lv in self.leaves.items()}
        self.masks = self.outs[64][1]
        for a, b in zip(self.masks, self.outs[32][1]):
            assert np.array_equal(a, b)

    def grads(self, cots):
        return [RS.grads_of(self.outs[dt][0], cots, self.leaves[dt], dtype=np.float64, retain=True) for dt in (64, 32)]


def f32_scale(corr_scale, C):
    """the multiplier as the kernel receives it: rounded to float32"""
    return float(np.float32(corr_scale if corr_scale is not None else 1.0 / float(C) ** 0.5))


@functools.lru_cache(maxsize=None)
def k1_reference(case, corr_scale):
    c = RS.k1_case(case)
    scale = f32_scale(corr_scale, case[1])
    return Restated(c, lambda lv: RS.sweep_corr_restated(lv[0], lv[1:], c["Kk"], c["Ks"], c["Ts"], c["inv"], scale))


@functools.lru_cache(maxsize=None)
def warp_reference(case):
    c = RS.warp_case(case)
    return Restated(c, lambda lv: RS.sweep_warp_restated(lv, c["Kk"], c["Ks"], c["Ts"], c["inv"], c["key_size"], False))


def calibration(c, dev):
    return T(c["Kk"], dev), [T(k, dev) for k in c["Ks"]], [T(t, dev) for t in c["Ts"]], T(c["inv"], dev)


# ------------------------------------------------------------------------------------------------ K1 backward
K1_RUNS = [(case, None) for case in RS.K1_CASES] + [(RS.K1_CASES[0], 0.37)]


@pytest.mark.parametrize("case,corr_scale", K1_RUNS, ids=lambda x: str(x).replace(" ", ""))
def test_sweep_corr_backward_vs_restatement(case, corr_scale, dev):
    from robustmvd_amd import ops
    ref = k1_reference(case, corr_scale)
    c, S, V = ref.c, case[6], case[7]
    Kk, Ks, Ts, inv = calibration(c, dev)
    fk, fs = T(c["fk"], dev, True), [T(f, dev, True) for f in c["fs"]]
    corrs, masks = ops.sweep_corr_autograd(fk, fs, Kk, Ks, Ts, inv, corr_scale)
    assert all(x.requires_grad for x in corrs) and not any(m.requires_grad for m in masks)
    with torch.no_grad():
        corrs0, masks0 = ops.sweep_corr(fk, fs, Kk, Ks, Ts, inv, corr_scale)
    for v in range(V):
        assert torch.equal(corrs[v], corrs0[v]) and torch.equal(masks[v], masks0[v])
        assert np.array_equal(masks[v].cpu().numpy(), ref.masks[v]), f"mask of view {v}"
        assert 0 < ref.masks[v].mean() < 1
        check(corrs[v], ref.outs[64][0][v].detach().numpy(), None, f"K1 {case} corr{v}", FORWARD)
    rng = np.random.default_rng(case[-1] + 1000)
    full = [rng.standard_normal(tuple(x.shape)).astype(np.float32) for x in corrs]
    names = ["dkey"] + [f"dsrc{v}" for v in range(V)]
    for planes in [None] + (RS.one_hot_planes(S) if corr_scale is None else []):
        cots = full if planes is None else select_planes(full, planes)
        want64, want32 = ref.grads(cots)
        got = gpu_grads(corrs, cots, [fk] + fs, dev)
        for a, w64, w32, k in zip(got, want64, want32, names):
            if planes is not None:
                assert np.abs(w64).max() > 1e-3, f"one-hot {planes}: the reference's {k} is zero"
            check(a, w64, w32, f"K1 {case} scale {corr_scale} planes {planes or 'all'} {k}", GOLD)


def test_sweep_corr_autograd_refuses_unsupported_channels_at_forward(dev):
    """C = 320 runs on the forward's cells form but has no backward kernel: with a gradient to come the call itself raises (not
    backward()); without one it is the inference result"""
    from robustmvd_amd import ops
    c = RS.sweep_case(1, 320, 7, 12, 7, 12, 6, 2, "shared", 401)
    Kk, Ks, Ts, inv = calibration(c, dev)
    for grad_on in (0, 2):
        tensors = [T(f, dev, i == grad_on) for i, f in enumerate([c["fk"]] + c["fs"])]
        with pytest.raises(ValueError, match="C=320.*64, 128, 192, 256"):
            ops.sweep_corr_autograd(tensors[0], tensors[1:], Kk, Ks, Ts, inv)
        with torch.no_grad():
            corrs, masks = ops.sweep_corr_autograd(tensors[0], tensors[1:], Kk, Ks, Ts, inv)
            want, wmask = ops.sweep_corr(tensors[0], tensors[1:], Kk, Ks, Ts, inv)
        for a, b in zip(corrs + masks, want + wmask):
            assert torch.equal(a, b)
    plain = [T(f, dev) for f in [c["fk"]] + c["fs"]]
    corrs, _ = ops.sweep_corr_autograd(plain[0], plain[1:], Kk, Ks, Ts, inv)
    assert all(torch.equal(a, b) for a, b in zip(corrs, want)) and not any(x.requires_grad for x in corrs)


# ------------------------------------------------------------------------------------------------ warp-only backward
@pytest.mark.parametrize("case", RS.WARP_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_sweep_warp_backward_vs_restatement(case, dev):
    from robustmvd_amd import ops
    ref = warp_reference(case)
    c, S, V = ref.c, case[5], case[6]
    Kk, Ks, Ts, inv = calibration(c, dev)
    fs = [T(f, dev, True) for f in c["fs"]]
    warped, masks = ops.sweep_warp_autograd(fs, Kk, Ks, Ts, inv, c["key_size"], normalize_after=False)
    assert all(x.requires_grad for x in warped) and not any(m.requires_grad for m in masks)
    with torch.no_grad():
        warped0, masks0 = ops.sweep_warp(fs, Kk, Ks, Ts, inv, c["key_size"], False)
    for v in range(V):
        assert torch.equal(warped[v], warped0[v]) and torch.equal(masks[v], masks0[v])
        assert np.array_equal(masks[v].cpu().numpy(), ref.masks[v]), f"mask of view {v}"
        check(warped[v], ref.outs[64][0][v].detach().numpy(), None, f"warp-only {case} warped{v}", FORWARD)
    rng = np.random.default_rng(case[-1] + 1000)
    full = [rng.standard_normal(tuple(x.shape)).astype(np.float32) for x in warped]
    for planes in [None] + RS.one_hot_planes(S, warp_only=True):
        cots = full if planes is None else select_planes(full, planes)
        want64, want32 = ref.grads(cots)
        got = gpu_grads(warped, cots, fs, dev)
        for v, (a, w64, w32) in enumerate(zip(got, want64, want32)):
            if planes is not None:
                assert np.abs(w64).max() > 1e-3, f"one-hot {planes}: the reference's dsrc{v} is zero"
            check(a, w64, w32, f"warp-only {case} planes {planes or 'all'} dsrc{v}", GOLD)


# ------------------------------------------------------------------------------------------------ K2 backward
K2_MASKED = [(0, 1, 2), (1, 2, 4)]   # (n, y, x): every view masked on every plane, W == 0
K2_ONLY_VIEW0 = (1, 0, 0)


@pytest.mark.parametrize("V,S,spread", [(V, S, 3) for V in (2, 5, 32) for S in (1, 65, 130)] + [(V, 65, 30) for V in (2, 5, 32)])
def test_fuse_views_backward_vs_oracle(V, S, spread, dev):
    """N h w = 30 waves (the last block is half full); S = 1 (63 idle lanes), 65 and 130 (a lane stride with a tail of 1 and 2);
    spread 30: the softmax saturates, most views have a weight below the 1e-9 floor"""
    from robustmvd_amd import ops
    N, h, w = 2, 3, 5
    rng = np.random.default_rng(1000 * V + 10 * S + spread)
    corrs = [rng.standard_normal((N, S, h, w)).astype(np.float32) for _ in range(V)]
    masks = [(rng.uniform(size=(N, S, h, w)) > 0.4).astype(np.float32) for _ in range(V)]
    for v, m in enumerate(masks):
        for n, y, x in K2_MASKED:
            m[n, :, y, x] = 0
        n, y, x = K2_ONLY_VIEW0
        m[n, :, y, x] = 1 if v == 0 else 0
    scores = [(rng.standard_normal((N, 1, h, w)) * spread).astype(np.float32) for _ in range(V)]
    g = rng.standard_normal((N, S, h, w)).astype(np.float32)
    want64 = O.fuse_views_backward(corrs, masks, scores, g, out_dtype=np.float64)
    want32 = O.fuse_views_backward(corrs, masks, scores, g, dtype=np.float32, out_dtype=np.float64)
    assert all(np.isfinite(a).all() for part in want32 for a in part)
    ct, st, mt = [T(x, dev, True) for x in corrs], [T(x, dev, True) for x in scores], [T(m, dev) for m in masks]
    fused, fmask = ops.fuse_views_autograd(ct, mt, st)
    with torch.no_grad():
        fused0, fmask0 = ops.fuse_views(ct, mt, st)
    assert torch.equal(fused, fused0) and torch.equal(fmask, fmask0)
    got = torch.autograd.grad((fused * T(g, dev)).sum(), ct + st)
    for i, (a, w64, w32) in enumerate(zip(got, want64[0] + want64[1], want32[0] + want32[1])):
        what = f"K2 V{V} S{S} x{spread} " + (f"dcorr{i}" if i < V else f"dscore{i - V}")
        check(a, w64, w32, what, K2_HARD)
        a = a.cpu().numpy()
        e = np.abs(w32 - w64).max()
        for n, y, x in K2_MASKED:
            px = a[n, :, y, x]
            if i < V:
                assert np.count_nonzero(px) == 0, what
            else:
                assert np.count_nonzero(w64[n, :, y, x]) == 0 and (np.abs(px) <= SHARP_MULTIPLE * e).all(), what
        if 0 < i < V:  # where only view 0 is valid the others' correlation has no say
            assert np.count_nonzero(a[K2_ONLY_VIEW0[0], :, K2_ONLY_VIEW0[1], K2_ONLY_VIEW0[2]]) == 0, what


# ------------------------------------------------------------------------------------------------ K3 backward
@functools.lru_cache(maxsize=None)
def k3_reference(shape):
    B, C, h, w, D, V = shape
    feats, projs, key_inv, depth = mvs_inputs(B, C, h, w, D, V, seed=sum(shape))
    G = np.random.default_rng(sum(shape) + 1).standard_normal((B, C, D, h, w)).astype(np.float32)
    return feats, projs, key_inv, depth, G, O.warp_variance_backward(feats[0], feats[1:], projs, key_inv, depth, G)


@pytest.mark.parametrize("backward", ["atomic", "gather"])
@pytest.mark.parametrize("shape", [(2, 4, 5, 7, 9, 1), (1, 64, 6, 9, 17, 2), (1, 8, 7, 5, 8, 3), (1, 16, 5, 6, 16, 32)])
def test_warp_variance_backward_vs_oracle(shape, backward, dev):
    """C = 4 and 64 (one and sixteen threads per pixel); D = 9 and 17 (a second / third chunk of one plane), 8 and 16 (full chunks);
    B = 2; V = 1 and the API's maximum"""
    from robustmvd_amd import ops
    feats, projs, key_inv, depth, G, (dkey, dsrcs) = k3_reference(shape)
    ft = [T(f, dev, True) for f in feats]
    args = ([T(p, dev) for p in projs], T(key_inv, dev), T(depth, dev))
    var = ops.warp_variance_autograd(ft[0], ft[1:], *args, backward=backward)
    with torch.no_grad():
        assert torch.equal(var, ops.warp_variance(ft[0], ft[1:], *args))
    got = torch.autograd.grad((var * T(G, dev)).sum(), ft)
    for i, (a, want) in enumerate(zip(got, [dkey] + dsrcs)):
        assert np.abs(want).max() > 0
        check(a, want.astype(np.float64), None, f"K3 {shape} {backward} d feat{i}", RAGGED)
