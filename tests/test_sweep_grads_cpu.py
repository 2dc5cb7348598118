"""CPU side of the differentiable sweep consumers (mvd_sweep_reduce_backward_f32, mvd_sweep_warp_backward_f32):

(a) a float64 restatement of the three sweep reductions and of the warp-only sweep, local to this module, whose autograd
    gradients are pinned against the reference's own (tests/golden/g15_sweep_grads.npz).  The GPU tests
    (tests/test_hip_sweep_grads.py) use it as their checker on the shapes the reference was never run on;
    The same for K1 (sweep_corr_restated: the warp-only gather, the dot product with the key, sampling mask x visibility), pinned
    against g10_grads.npz and the oracle's VJP, with the cases of tests/test_hip_backward_shapes.py and the check that none of
    their samples sits on a decision boundary of the float32 chain.  The restatements' dtype follows their leaves, so one
    function gives the float64 reference and the float32 evaluation that measures the formula's own rounding;
(b) the argument validation of the two C entry points, which runs before any GPU call, and sweep_corr_autograd's refusal of a
    channel count without a backward kernel at the call;
(c) the inference entries still refuse an input that requires grad (ops.inference_only).

The restatement computes the sampling positions in float32 with the kernels' formulas (a fused multiply-add is the exact product and
sum rounded once to float32: _fma) and gathers by index in float64 under autograd."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
import gen_common as gc

f32 = np.float32


# ------------------------------------------------------------------------------------------------ the restatement
def _fma(a, b, c):
    """fmaf of float32 operands, rounded ONCE.  The product is exact in float64; its sum with c is rounded to float64 (s) and
    then to float32, which is the single rounding of the exact value unless s lies exactly half-way between two float32 and the
    float64 rounding error e (Knuth's two-sum, exact) is not zero: then e's sign decides, not the tie rule."""
    p, c = np.asarray(a, np.float64) * np.asarray(b, np.float64), np.asarray(c, np.float64)
    with np.errstate(all="ignore"):
        s = p + c
        r = s.astype(f32)
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        lo, hi = np.nextafter(s, -np.inf).astype(f32), np.nextafter(s, np.inf).astype(f32)
        tie = np.isfinite(s) & (lo != hi) & (lo.astype(np.float64) * 0.5 + hi.astype(np.float64) * 0.5 == s) & (e != 0)
    return np.where(tie, np.where(e > 0, hi, lo), r).astype(f32)


def reduce_positions(M, depth, h, w, pix_offset, stretch):
    """sweep_homography.h sample_position_div in float32: M (B,3,4), depth (B,D) or (B,D,h,w) -> ix, iy (B,D,h,w), clamped."""
    M = np.asarray(M, f32).reshape(-1, 12)
    B = M.shape[0]
    depth = np.asarray(depth, f32)
    if depth.ndim == 2:
        depth = np.broadcast_to(depth[:, :, None, None], (B, depth.shape[1], h, w))
    fx = (np.arange(w, dtype=f32) + f32(pix_offset))[None, None, None, :]
    fy = (np.arange(h, dtype=f32) + f32(pix_offset))[None, None, :, None]
    m = lambda i: M[:, i].reshape(B, 1, 1, 1)
    sx, sy = (f32(w / (w - 1)), f32(h / (h - 1))) if stretch else (f32(1), f32(1))
    ax, ay, az = _fma(m(0), fx, _fma(m(1), fy, m(2))), _fma(m(4), fx, _fma(m(5), fy, m(6))), _fma(m(8), fx, _fma(m(9), fy, m(10)))
    X, Y, Z = _fma(ax, depth, m(3)), _fma(ay, depth, m(7)), _fma(az, depth, m(11))
    with np.errstate(all="ignore"):
        ix, iy = _fma(X / Z, sx, f32(-0.5)), _fma(Y / Z, sy, f32(-0.5))
    clamp = lambda v, hi: np.where(np.isnan(v), f32(-1), np.clip(v, f32(-1), f32(hi))).astype(f32)  # fmed3: NaN -> -1
    return clamp(ix, w), clamp(iy, h)


def _gather4(src, cell_y, cell_x, wts):
    """src (B,C,hs,ws) float64 tensor; cell_y/x (B,D,h,w) integer top-left tap in the map padded by (1 before, 2 after); wts: four
    (B,D,h,w) float32 weights (nw, ne, sw, se) -> (B,C,D,h,w) samples in src's dtype, differentiable w.r.t. src."""
    P = torch.nn.functional.pad(src, (1, 2, 1, 2))
    out = []
    for b in range(src.shape[0]):
        y0, x0 = torch.from_numpy(cell_y[b].astype(np.int64)), torch.from_numpy(cell_x[b].astype(np.int64))
        w4 = [torch.from_numpy(np.ascontiguousarray(wk[b], f32)).to(src.dtype) for wk in wts]
        out.append(P[b][:, y0, x0] * w4[0] + P[b][:, y0, x0 + 1] * w4[1] + P[b][:, y0 + 1, x0] * w4[2] + P[b][:, y0 + 1, x0 + 1] * w4[3])
    return torch.stack(out)


def reduce_sample(src, M, depth, pix_offset, stretch, bounds=None):
    """bounds: (xlo, xhi, ylo, yhi) float32 within [-1, w] x [-1, h], sweep_groupcorr_nhwc_kernel's second clamp of the position."""
    h, w = src.shape[-2:]
    ix, iy = reduce_positions(M, depth, h, w, pix_offset, stretch)
    if bounds is not None:
        xlo, xhi, ylo, yhi = (f32(v) for v in bounds)
        ix, iy = np.clip(ix, xlo, xhi), np.clip(iy, ylo, yhi)
    xf, yf = np.floor(ix), np.floor(iy)
    wx, wy = ix - xf, iy - yf
    ux, uy = f32(1) - wx, f32(1) - wy
    return _gather4(src, yf.astype(np.int64) + 1, xf.astype(np.int64) + 1, (ux * uy, wx * uy, ux * wy, wx * wy))


def sweep_reduce_restated(key, srcs, Ms, depth, mode, groups=1, pix_offset=0.0, stretch=True, bounds=None):
    """key, srcs: float64 tensors (B,C,h,w); Ms, depth: float32 arrays.  mode "variance" | "keysq" | "groupcorr".
    bounds: reduce_sample's (the group correlation's grid_clamp; None: the kernels' clamp to [-1, w] x [-1, h] alone)."""
    sv = [reduce_sample(s, M, depth, pix_offset, stretch, bounds) for s, M in zip(srcs, Ms)]
    k = key.unsqueeze(2)
    if mode == "groupcorr":
        B, C, D, h, w = sv[0].shape
        return [(k * s).view(B, groups, C // groups, D, h, w).sum(2) for s in sv]
    N = len(srcs) + 1
    s2 = k * k + sum(s * s for s in sv)
    s1 = (k * k if mode == "keysq" else k) + sum(sv)
    return s2 / N - (s1 / N) ** 2


def warp_chain(K_key, K_src, T, invd, h, w, hs, ws):
    """sweep_epipolar.h's chain in float32, one rounding per operation: K_* (N,3,3) relative intrinsics, T (N,4,4), invd (1 or N, S)
    or per key pixel (N,S,h,w) -> dict of (N,S,h,w) arrays: cell_y, cell_x, wts (four tap weights, zero where out of bounds), inb
    (their sum), mask (the 0/1 sampling mask), visible (sweep_sample's visibility, bool) and the values it is decided on: k_inf,
    z_pole (N,1,h,w) and zs."""
    Kk, Ks, T = np.asarray(K_key, f32), np.asarray(K_src, f32), np.asarray(T, f32)
    N = Kk.shape[0]
    c = lambda a: a.reshape(N, 1, 1, 1)
    fx, fy, cx, cy = c(Kk[:, 0, 0] * f32(w)), c(Kk[:, 1, 1] * f32(h)), c(Kk[:, 0, 2] * f32(w)), c(Kk[:, 1, 2] * f32(h))
    fxo, fyo, cxo, cyo = c(Ks[:, 0, 0] * f32(ws)), c(Ks[:, 1, 1] * f32(hs)), c(Ks[:, 0, 2] * f32(ws)), c(Ks[:, 1, 2] * f32(hs))
    r = lambda i, j: c(T[:, i, j])
    A, Bq = fxo * r(0, 0) + cxo * r(2, 0), fxo * r(0, 1) + cxo * r(2, 1)
    Ea, Eb = A / fx, Bq / fy
    Ec = -(cx * A / fx) - (cy * Bq / fy) + (fxo * r(0, 2) + cxo * r(2, 2))
    Ee = fxo * r(0, 3) + cxo * r(2, 3)
    Fq, G = fyo * r(1, 0) + cyo * r(2, 0), fyo * r(1, 1) + cyo * r(2, 1)
    Ef, Eg = Fq / fx, G / fy
    Eh = -(cx * Fq / fx) - (cy * G / fy) + (fyo * r(1, 2) + cyo * r(2, 2))
    Ei = fyo * r(1, 3) + cyo * r(2, 3)
    Ej, Ek = r(2, 0) / fx, r(2, 1) / fy
    El = -cx * r(2, 0) / fx - cy * r(2, 1) / fy + r(2, 2)
    Em = r(2, 3)
    xc = (np.arange(w, dtype=f32) + f32(0.5))[None, None, None, :]
    yc = (np.arange(h, dtype=f32) + f32(0.5))[None, None, :, None]
    u_inf, v_inf, k_inf = (Ea * xc + Eb * yc) + Ec, (Ef * xc + Eg * yc) + Eh, (Ej * xc + Ek * yc) + El
    invd = np.asarray(invd, f32)
    if invd.ndim == 4:  # per key pixel
        assert invd.shape[0] == N and invd.shape[2:] == (h, w), invd.shape
        ds = invd
    else:
        ds = np.broadcast_to(invd, (N, invd.shape[1]))[:, :, None, None]
    with np.errstate(all="ignore"):
        den = k_inf + Em * ds
        us, vs = (u_inf + Ee * ds) / den, (v_inf + Ei * ds) / den
        zs = np.broadcast_to(f32(1) / ds, us.shape).astype(f32)
        z_pole = (-(Em / k_inf)).astype(f32)
        visible = (zs > 0) & (((k_inf > 0) & (zs > z_pole)) | ((k_inf < 0) & (zs < z_pole)) | ((k_inf == 0) & (Em > 0)))

    def fix(v):
        v = np.where(np.isinf(v), np.where(v > 0, f32(1e9), f32(-1e9)), v)
        return np.where(np.isnan(v), f32(1e9), v).astype(f32)

    us, vs = fix(us), fix(vs)
    fws, fhs = f32(ws), f32(hs)
    ix = ((f32(2) * us / fws - f32(1) + f32(1)) * fws - f32(1)) / f32(2)
    iy = ((f32(2) * vs / fhs - f32(1) + f32(1)) * fhs - f32(1)) / f32(2)
    x0, y0 = np.floor(ix), np.floor(iy)
    x1, y1 = x0 + f32(1), y0 + f32(1)
    wx1, wx0, wy1, wy0 = ix - x0, x1 - ix, iy - y0, y1 - iy
    wts, inb = [], np.zeros_like(ix)
    for xs, ys, wt in ((x0, y0, wx0 * wy0), (x1, y0, wx1 * wy0), (x0, y1, wx0 * wy1), (x1, y1, wx1 * wy1)):
        ok = (xs >= 0) & (xs <= ws - 1) & (ys >= 0) & (ys <= hs - 1)
        wk = np.where(ok, wt, f32(0)).astype(f32)
        wts.append(wk)
        inb = inb + wk
    mask = np.where(inb < f32(0.9999), f32(0), f32(1)).astype(f32)
    cell_x = np.clip(x0, -1, ws - 1).astype(np.int64) + 1
    cell_y = np.clip(y0, -1, hs - 1).astype(np.int64) + 1
    all_in = (x0 >= 0) & (x1 <= ws - 1) & (y0 >= 0) & (y1 <= hs - 1)
    return dict(cell_y=cell_y, cell_x=cell_x, wts=wts, inb=inb, all_in=all_in, mask=mask, visible=visible, k_inf=k_inf.astype(f32),
                z_pole=z_pole, zs=zs)


def warp_cells(K_key, K_src, T, invd, h, w, hs, ws):
    """warp_chain's cell_y, cell_x (N,S,h,w), four tap weights, the 0/1 sampling mask and the visibility term (bool)."""
    g = warp_chain(K_key, K_src, T, invd, h, w, hs, ws)
    return g["cell_y"], g["cell_x"], g["wts"], g["mask"], g["visible"]


def sweep_warp_restated(srcs, K_key, K_srcs, Ts, invd, key_size, normalize=False):
    """PlanesweepCorrelation(warp_only=True): srcs tensors (N,C,hs,ws) -> (warped[V] (N,S,C,h,w) in their dtype, masks[V])."""
    h, w = key_size
    nrm = lambda x, dim: x / (torch.linalg.norm(x, dim=dim, keepdim=True) + 1e-9)
    warped, masks = [], []
    for s, Ks, T in zip(srcs, K_srcs, Ts):
        hs, ws = s.shape[-2:]
        if normalize == "before":
            s = nrm(s, 1)
        cy, cx, wts, mask, _ = warp_cells(K_key, Ks, T, invd, h, w, hs, ws)
        x = _gather4(s, cy, cx, wts).transpose(1, 2)  # (N,S,C,h,w)
        if normalize is True or normalize == "after":
            x = nrm(x, 2)
        warped.append(x * torch.from_numpy(mask).to(x.dtype).unsqueeze(2))
        masks.append(mask)
    return warped, masks


def sweep_corr_restated(key, srcs, K_key, K_srcs, Ts, invd, corr_scale):
    """PlanesweepCorrelation (K1): key (N,C,h,w), srcs V x (N,C,hs,ws) tensors -> (corrs[V] (N,S,h,w) in the leaves' dtype, masks[V]):
    the warped sample's dot product with the key times corr_scale times the mask, which is sampling mask x visibility, a constant."""
    h, w = key.shape[-2:]
    k = key.unsqueeze(2)
    corrs, masks = [], []
    for s, Ks, T in zip(srcs, K_srcs, Ts):
        cy, cx, wts, mask, visible = warp_cells(K_key, Ks, T, invd, h, w, *s.shape[-2:])
        mask = mask * visible.astype(f32)
        corrs.append((k * _gather4(s, cy, cx, wts)).sum(1) * corr_scale * torch.from_numpy(mask).to(key.dtype))
        masks.append(mask)
    return corrs, masks


def grads_of(outs, cots, inputs, dtype=f32, retain=False):
    """autograd.grad of sum_i sum(outs[i] * cots[i]) w.r.t. inputs -> arrays of `dtype`."""
    loss = sum((o * torch.from_numpy(np.asarray(c, np.float64)).to(o.dtype)).sum() for o, c in zip(outs, cots))
    return [x.numpy().astype(dtype) for x in torch.autograd.grad(loss, inputs, retain_graph=retain)]


def leaf64(a):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)


def leaf32(a):
    return torch.from_numpy(np.array(a, f32)).requires_grad_(True)


def cvp_Ms(g):
    """sweep_modes._cvp_transform on the host (float32 matmuls and inverse like the package's)."""
    last = np.array([[0, 0, 0, 1]], f32)
    out = []
    for v in range(g["cvp_src_in"].shape[1]):
        sp = np.concatenate((g["cvp_src_in"][0, v] @ g["cvp_src_ex"][0, v, :3], last)).astype(f32)
        rp = np.concatenate((g["cvp_ref_in"][0] @ g["cvp_ref_ex"][0, :3], last)).astype(f32)
        out.append((sp @ np.linalg.inv(rp).astype(f32))[None, :3, :4].astype(f32))
    return out


def vis_Ms(ref_cam, srcs_cam):
    from robustmvd_amd import sweep_modes as SM
    return [SM._vis_transform(torch.from_numpy(ref_cam), torch.from_numpy(sc)).numpy() for sc in srcs_cam]


def vis_depth(ds, di, D, h, w):
    d = ds.astype(f32) + di.astype(f32) * np.arange(D, dtype=f32).reshape(1, D, 1, 1)
    return d.reshape(d.shape[0], D) if d.shape[2:] == (1, 1) else np.ascontiguousarray(np.broadcast_to(d, (d.shape[0], D, h, w)))


# Tolerance of (a).  The restatement and the reference differ in (1) the sampling position: the reference normalises the
# coordinate to [-1, 1] and grid_sample un-normalises it again, a handful of float32 roundings of a value of magnitude <= 20
# pixels, i.e. <= ~1e-5 pixel, which moves a sample by <= 1e-5 x (difference of neighbouring features ~ 4) and a gradient, a sum
# of <= D x V such terms times cotangent x feature factors of order 1..10, by a few 1e-5 at most; (2) the reference's float32
# accumulation, relative 6e-8 x sqrt(terms) of gradients of magnitude <= ~70 (the aliased cvp key gradient), ~1e-5.  Vis-MVSNet's
# homographies are a longer float32 matrix chain (get_homographies), so its positions are the least exact.
# Measured here (max |diff| / max |gradient|): vis 8.0e-5 / 12.9 (key), 5.2e-5 / 11.4 (sources); cvp aliased 2.8e-5 / 71;
# cvp without the alias 1.6e-5 / 6.6; warp-only 7e-7 / 6.7 (its grid chain is restated operation by operation).
# 2e-4 / 1e-4 is the GPU tests' tolerance for scatter-add gradients (tests/test_hip_backward.py); this checker is held to half
# its absolute part, which the worst case above still meets without the relative part.
ATOL, RTOL = 1e-4, 1e-4


def _close(got, want, what):
    err = np.abs(got - want)
    print(f"{what}: max |diff| {err.max():.3e}, max |want| {np.abs(want).max():.3e}")
    np.testing.assert_allclose(got, want, atol=ATOL, rtol=RTOL, err_msg=what)


@pytest.mark.parametrize("name", ["pp", "pl"])
@pytest.mark.parametrize("alias", [True, False])
def test_restated_cvp_gradients_match_reference(name, alias):
    g, gr = load_golden("g11_sweep_modes"), load_golden("g15_sweep_grads")
    key, srcs = leaf64(g["cvp_ref"]), [leaf64(g["cvp_src0"]), leaf64(g["cvp_src1"])]
    out = sweep_reduce_restated(key, srcs, cvp_Ms(g), g[f"cvp_hyp_{name}"], "keysq" if alias else "variance")
    tag, suf = (f"cvp_{name}", "") if alias else (f"cvp_{name}_noalias", "_f64")
    got = grads_of([out], [gc.rng_array(int(gr[tag + "_seed"]), tuple(out.shape))], [key] + srcs)
    for a, k in zip(got, ("dkey", "dsrc0", "dsrc1")):
        _close(a, gr[f"{tag}_{k}{suf}"], f"{tag}_{k}")


@pytest.mark.parametrize("name", ["s", "p"])
def test_restated_vis_gradients_match_reference(name):
    g, gr = load_golden("g11_sweep_modes"), load_golden("g15_sweep_grads")
    key, srcs = leaf64(g["vis_ref"]), [leaf64(g["vis_src0"]), leaf64(g["vis_src1"])]
    Ms = vis_Ms(g["vis_ref_cam"], [g["vis_src_cam0"], g["vis_src_cam1"]])
    outs = sweep_reduce_restated(key, srcs, Ms, vis_depth(g[f"vis_ds_{name}"], g[f"vis_di_{name}"], 5, 12, 20), "groupcorr", groups=8,
                                 pix_offset=0.5, stretch=False)
    seed = int(gr[f"vis_{name}_seed"])
    got = grads_of(outs, [gc.rng_array(seed + v, tuple(o.shape)) for v, o in enumerate(outs)], [key] + srcs)
    for a, k in zip(got, ("dkey", "dsrc0", "dsrc1")):
        _close(a, gr[f"vis_{name}_{k}"], f"vis_{name}_{k}")


@pytest.mark.parametrize("name,norm", [("none", False), ("before", "before"), ("after", True)])
def test_restated_warp_only_gradients_match_reference(name, norm):
    g, gr = load_golden("g13_warp_only"), load_golden("g15_sweep_grads")
    srcs = [leaf64(gc.rng_array(1502, (1, 16, 12, 18))), leaf64(gc.rng_array(1503, (1, 16, 12, 18)))]
    warped, masks = sweep_warp_restated(srcs, g["K"], [g["K"]] * 2, [g["T0"], g["T1"]], g["invdepths"].reshape(1, -1), (12, 18), norm)
    for v in range(2):  # the forward itself is the recorded one
        np.testing.assert_allclose(warped[v].detach().numpy(), g[f"{name}_warped{v}"], atol=ATOL, rtol=RTOL)
    seed = int(gr[f"warp_{name}_seed"])
    got = grads_of(warped, [gc.rng_array(seed + v, tuple(o.shape)) for v, o in enumerate(warped)], srcs)
    for v in range(2):
        _close(got[v], gr[f"warp_{name}_dsrc{v}"], f"warp_{name}_dsrc{v}")


# ------------------------------------------------------------------------------------------------ K1 and the shape sweep's cases
# The cases of tests/test_hip_backward_shapes.py, built here so that their inputs are checked without a GPU.
# K1: (N, C, h, w, hs, ws, S, V, inverse-depth mode, seed); warp-only: (N, C, hs, ws, (h, w), S, V, mode, seed).
K1_CASES = [
    (2, 128, 6, 7, 5, 9, 70, 2, "batched", 101),   # <2>, two passes, tail of 6, N = 2, source size differs
    (1, 256, 5, 6, 5, 6, 130, 2, "shared", 102),   # <4>, three passes, tail of 2
    (1, 192, 4, 9, 6, 7, 65, 1, "shared", 103),    # <3>, tail of 1
    (2, 64, 3, 5, 3, 5, 64, 3, "batched", 104),    # exactly one full pass; 30 waves: the last block is partial
    (1, 256, 4, 5, 4, 5, 256, 1, "shared", 105),   # the model's own C and S
    (2, 64, 4, 5, 4, 5, 67, 2, "pixel", 106),      # per key pixel
]
WARP_CASES = [
    (1, 65, 5, 6, (5, 6), 70, 2, "shared", 201),
    (2, 100, 4, 7, (5, 6), 65, 1, "batched", 202),
    (1, 130, 4, 5, (4, 5), 9, 2, "shared", 203),
    (1, 192, 4, 5, (4, 5), 64, 1, "shared", 204),
    (1, 256, 3, 5, (3, 5), 130, 1, "shared", 205),
    (1, 1, 6, 7, (6, 7), 5, 1, "shared", 206),
    (2, 16, 4, 5, (4, 5), 67, 2, "pixel", 207),
]


def one_hot_planes(S, warp_only=False):
    """The cotangent supports of the one-hot cases, which make a dropped plane a 100 % error (K1: the cases with S = 67 and 130,
    warp-only: S = 130): the last plane, the first plane of the second pass, and the two planes either side of the pass boundary
    (a run that may share a cell across it)."""
    return [(S - 1,), (64,), (63, 64)] if S in ((130,) if warp_only else (67, 130)) else []


def sweep_case(N, C, h, w, hs, ws, S, V, mode, seed, with_key=True):
    """Seeded inputs with the calibration of test_hip_shapes.test_sweep_corr_vs_oracle."""
    from oracle import mvd_oracle as O
    rng = np.random.default_rng(seed)
    fk = rng.standard_normal((N, C, h, w)).astype(f32) if with_key else None
    fs = [rng.standard_normal((N, C, hs, ws)).astype(f32) for _ in range(V)]
    Kk = np.stack([np.array([[0.72, 0, 0.5], [0, 1.28, 0.5], [0, 0, 1]], f32)] * N)
    Ks = [Kk * np.array([[1.0 + 0.05 * v], [1.0 - 0.03 * v], [1.0]], f32) for v in range(V)]
    Ts = [np.stack([gc.synthetic_pose(rng, 0.08, 0.2) for _ in range(N)]) for _ in range(V)]
    n = 1 if mode == "shared" else N
    inv = O.compute_sampling_invdepths(np.full(n, 0.4, f32), np.linspace(100.0, 1000.0, n).astype(f32), S)
    if mode == "pixel":
        inv = (inv[:, :, None, None] * (1 + 0.05 * rng.uniform(-1, 1, (N, S, h, w)))).astype(f32)
    return dict(fk=fk, fs=fs, Kk=Kk, Ks=Ks, Ts=Ts, inv=inv, key_size=(h, w))


def k1_case(case):
    return sweep_case(*case)


def warp_case(case):
    N, C, hs, ws, (h, w), S, V, mode, seed = case
    return sweep_case(N, C, h, w, hs, ws, S, V, mode, seed, with_key=False)


@pytest.mark.parametrize("case", K1_CASES + WARP_CASES, ids=str)
def test_shape_sweep_inputs_are_off_the_decision_boundaries(case):
    """No sample of a case sits where one float32 rounding decides a mask entry: the sampling mask's threshold (inb against 0.9999,
    for the samples with a tap out of bounds; the others sum to 1), the sign of k_inf, and zs against the pole's depth.  Under this
    condition the GPU tests demand masks EQUAL to the restated ones.  Every view of every one-hot plane keeps a live sample, so
    that no one-hot case is vacuous."""
    c = k1_case(case) if len(case) == 10 else warp_case(case)
    (h, w), (hs, ws) = c["key_size"], c["fs"][0].shape[-2:]
    S = c["inv"].shape[1]
    for v, (Ks, T) in enumerate(zip(c["Ks"], c["Ts"])):
        g = warp_chain(c["Kk"], Ks, T, c["inv"], h, w, hs, ws)
        edge = ~g["all_in"]
        d_inb = np.abs(g["inb"][edge] - f32(0.9999)).min() if edge.any() else np.inf
        d_k = np.abs(g["k_inf"]).min()
        d_z = (np.abs(g["zs"] - g["z_pole"]) / np.abs(g["z_pole"])).min()
        print(f"{case} view {v}: |inb - 0.9999| >= {d_inb:.2e}, |k_inf| >= {d_k:.2e}, |zs - z_pole| / |z_pole| >= {d_z:.2e}")
        assert d_inb > 1e-6 and d_k > 1e-6 and d_z > 1e-5
        assert np.abs(g["inb"][g["all_in"]] - 1).max(initial=0) < 1e-5
        live = g["mask"] * (g["visible"] if len(case) == 10 else 1)
        for planes in one_hot_planes(S, warp_only=len(case) != 10):
            assert all(live[:, s].any() for s in planes), (v, planes)


# The g10 gradients are float32 autograd through the reference: sums of <= S x 4 = 32 products of magnitude <= ~3 per key element
# (more per source element where samples crowd), each rounded to 6e-8 relative, and positions restated operation by operation.
# A few 1e-6 absolute at most; measured 2.4e-7 on gradients of magnitude 1-2.
K1_GOLDEN = dict(atol=5e-6, rtol=1e-5)


@pytest.mark.parametrize("name,V", [("toy", 2), ("behind", 1)])
def test_restated_sweep_corr_gradients_match_reference(name, V):
    g = load_golden("g10_grads")
    key, srcs = leaf64(gc.rng_array(1101, (1, 64, 12, 18))), [leaf64(gc.rng_array(1102 + i, (1, 64, 12, 18))) for i in range(V)]
    K = g[f"k1_{name}_K"]
    corrs, masks = sweep_corr_restated(key, srcs, K, [K] * V, [g[f"k1_{name}_T{v}"] for v in range(V)],
                                       g[f"k1_{name}_invdepths"].reshape(1, -1), 1.0 / 8.0)
    for v in range(V):
        want = g[f"k1_{name}_corr{v}"]
        print(f"k1_{name}_corr{v}: max |diff| {np.abs(corrs[v].detach().numpy() - want).max():.3e}, max |want| {np.abs(want).max():.3e}")
        np.testing.assert_allclose(corrs[v].detach().numpy(), want, **K1_GOLDEN)
    got = grads_of(corrs, [gc.rng_array(1110 + v, tuple(c.shape)) for v, c in enumerate(corrs)], [key] + srcs)
    for a, k in zip(got, ["dkey"] + [f"dsrc{v}" for v in range(V)]):
        want = g[f"k1_{name}_{k}"]
        print(f"k1_{name}_{k}: max |diff| {np.abs(a - want).max():.3e}, max |want| {np.abs(want).max():.3e}")
        np.testing.assert_allclose(a, want, err_msg=k, **K1_GOLDEN)


def test_restated_sweep_corr_matches_oracle_backward():
    """a shape no golden has: two batch elements with their own planes, source maps of another size than the key's.  The oracle
    accumulates in float64 on float32 positions like the restatement; its corr_scale is 1/sqrt(C) rounded to float32 (6e-8)."""
    from oracle import mvd_oracle as O
    c = sweep_case(2, 64, 5, 6, 4, 7, 9, 2, "batched", 301)
    key, srcs = leaf64(c["fk"]), [leaf64(f) for f in c["fs"]]
    corrs, masks = sweep_corr_restated(key, srcs, c["Kk"], c["Ks"], c["Ts"], c["inv"], 1.0 / 8.0)
    ref_c, ref_m, _ = O.planesweep_correlation(c["fk"], c["Kk"], c["fs"], c["Ts"], c["Ks"], sampling_invdepths=c["inv"])
    for v in range(2):
        assert np.array_equal(masks[v], ref_m[v]) and 0 < masks[v].mean() < 1
        np.testing.assert_allclose(corrs[v].detach().numpy(), ref_c[v], atol=2e-5, rtol=1e-5)  # the oracle's forward sums in float32
    rng = np.random.default_rng(302)
    cots = [rng.standard_normal(tuple(x.shape)).astype(f32) for x in corrs]
    got = grads_of(corrs, cots, [key] + srcs)
    dkey, dsrcs = O.planesweep_correlation_backward(c["fk"], c["Kk"], c["fs"], c["Ts"], c["inv"], cots, c["Ks"])
    for a, b, k in zip(got, [dkey] + dsrcs, ("dkey", "dsrc0", "dsrc1")):
        print(f"{k}: max |diff| {np.abs(a - b).max():.3e}, max |want| {np.abs(b).max():.3e}")
        np.testing.assert_allclose(a, b, err_msg=k, **K1_GOLDEN)


def test_restated_per_pixel_invdepths_broadcast():
    """per-pixel inverse depths (N,S,h,w) that are constant on each plane against the (N,S) path: the same values, whole and plane by
    plane (this pins warp_chain's per-pixel indexing: batch element, plane and pixel each land on their own axis)"""
    c = sweep_case(2, 64, 4, 5, 3, 6, 5, 2, "batched", 303)
    N, S, (h, w) = 2, 5, c["key_size"]
    pp = np.ascontiguousarray(np.broadcast_to(c["inv"][:, :, None, None], (N, S, h, w)))
    rng = np.random.default_rng(304)
    cots = [rng.standard_normal((N, S, h, w)).astype(f32) for _ in range(2)]

    def run(inv, cot):
        key, srcs = leaf64(c["fk"]), [leaf64(f) for f in c["fs"]]
        corrs, masks = sweep_corr_restated(key, srcs, c["Kk"], c["Ks"], c["Ts"], inv, 0.125)
        return [x.detach().numpy() for x in corrs], masks, grads_of(corrs, cot, [key] + srcs, dtype=np.float64)

    corr_pp, mask_pp, grad_pp = run(pp, cots)
    corr_ns, mask_ns, grad_ns = run(c["inv"], cots)
    for a, b in zip(corr_pp + mask_pp + grad_pp, corr_ns + mask_ns + grad_ns):
        assert np.array_equal(a, b)
    total = [0, 0, 0]
    for s in range(S):
        corr_s, mask_s, grad_s = run(c["inv"][:, s:s + 1], [x[:, s:s + 1] for x in cots])
        for v in range(2):
            assert np.array_equal(mask_s[v][:, 0], mask_pp[v][:, s])
            np.testing.assert_allclose(corr_s[v][:, 0], corr_pp[v][:, s], atol=1e-12, rtol=1e-12)  # float64 sums in another order
        total = [t + x for t, x in zip(total, grad_s)]
    for a, b in zip(total, grad_pp):
        np.testing.assert_allclose(a, b, atol=1e-12, rtol=1e-12)
    # a per-pixel map that is NOT constant moves each pixel's samples on its own
    live = np.argwhere((mask_pp[0] == 1) & (np.arange(N).reshape(N, 1, 1, 1) == 1))
    at = tuple(live[len(live) // 2])  # a live sample of view 0 in the second batch element
    pp2 = pp.copy()
    pp2[at] *= f32(1.5)
    corr2 = run(pp2, cots)[0]
    changed = [np.argwhere(a != b) for a, b in zip(corr2, corr_pp)]
    assert all((ch == at).all() for ch in changed) and len(changed[0]) == 1


# ------------------------------------------------------------------------------------------------ (b) validation, no GPU
def _arr(n, value=0x1000):
    return (ctypes.c_void_p * n)(*([value] * n))


def _reduce_backward(lib, **kw):
    a = dict(key=0x1000, src=_arr(2), M=_arr(2), depth=0x1000, per_pixel=0, mode=0, groups=1, gout=_arr(2), B=1, C=16, D=4, h=8, w=8, V=2,
             gkey=0x1000, gsrc=_arr(2), ws=0x1000, wsb=None)
    a.update(kw)
    if a["wsb"] is None:
        a["wsb"] = lib.mvd_sweep_reduce_backward_workspace_bytes(a["B"], a["C"], a["h"], a["w"], a["V"])
    cast = lambda x: ctypes.cast(x, ctypes.POINTER(ctypes.c_void_p)) if x is not None else None
    return lib.mvd_sweep_reduce_backward_f32(a["key"], cast(a["src"]), cast(a["M"]), a["depth"], a["per_pixel"], 0.0, 1.0, 1.0, -0.5,
                                             a["mode"], a["groups"], cast(a["gout"]), a["B"], a["C"], a["D"], a["h"], a["w"], a["V"],
                                             a["gkey"], cast(a["gsrc"]), a["ws"], a["wsb"], None)


def test_sweep_reduce_backward_validates_before_any_gpu_call():
    from robustmvd_amd import _lib as L
    lib = L.load()
    err = lambda: lib.mvd_last_error().decode()
    assert lib.mvd_sweep_reduce_backward_workspace_bytes(1, 16, 8, 8, 2) == 5 * lib.mvd_sweep_reduce_workspace_bytes(1, 16, 8, 8, 0)
    assert lib.mvd_sweep_reduce_backward_workspace_bytes(0, 16, 8, 8, 2) == 0
    for kw in (dict(key=None), dict(src=None), dict(gout=None), dict(gkey=None), dict(gsrc=None), dict(depth=None)):
        assert _reduce_backward(lib, **kw) == 1 and "NULL argument" in err()
    assert _reduce_backward(lib, gsrc=_arr(2, 0)) == 1 and "NULL view 0" in err()
    assert _reduce_backward(lib, mode=L.REDUCE_GROUPCORR, groups=2, gout=(ctypes.c_void_p * 2)(0x1000, 0)) == 1 and "NULL view 1" in err()
    assert _reduce_backward(lib, mode=3) == 1 and "mode 3" in err()
    assert _reduce_backward(lib, C=6) == 1 and "multiple of 4" in err()
    assert _reduce_backward(lib, mode=L.REDUCE_GROUPCORR, groups=8) == 1 and "C/groups = 16/8" in err()   # 2 channels per group
    assert _reduce_backward(lib, mode=L.REDUCE_GROUPCORR, groups=3) == 1 and "C/groups" in err()
    assert _reduce_backward(lib, V=0) == 1 and _reduce_backward(lib, V=L.MVD_MAX_VIEWS + 1, src=_arr(33), M=_arr(33), gsrc=_arr(33)) == 1
    assert _reduce_backward(lib, h=1) == 1 and "bad dimensions" in err()
    need = lib.mvd_sweep_reduce_backward_workspace_bytes(1, 16, 8, 8, 2)
    assert _reduce_backward(lib, wsb=need - 1) == 2 and "workspace" in err()
    assert _reduce_backward(lib, ws=None) == 2


def _warp_backward(lib, **kw):
    a = dict(Kk=0x1000, Ks=_arr(2), T=_arr(2), inv=0x1000, mode=0, gw=_arr(2), N=1, C=16, h=8, w=8, hs=8, ws=8, S=4, V=2, gsrc=_arr(2))
    a.update(kw)
    cast = lambda x: ctypes.cast(x, ctypes.POINTER(ctypes.c_void_p)) if x is not None else None
    return lib.mvd_sweep_warp_backward_f32(a["Kk"], cast(a["Ks"]), cast(a["T"]), a["inv"], a["mode"], cast(a["gw"]), a["N"], a["C"], a["h"],
                                           a["w"], a["hs"], a["ws"], a["S"], a["V"], cast(a["gsrc"]), None)


def test_sweep_warp_backward_validates_before_any_gpu_call():
    from robustmvd_amd import _lib as L
    lib = L.load()
    err = lambda: lib.mvd_last_error().decode()
    for kw in (dict(Kk=None), dict(Ks=None), dict(T=None), dict(inv=None), dict(gw=None), dict(gsrc=None)):
        assert _warp_backward(lib, **kw) == 1 and "NULL argument" in err()
    assert _warp_backward(lib, gw=(ctypes.c_void_p * 2)(0x1000, 0)) == 1 and "NULL view 1" in err()
    assert _warp_backward(lib, mode=3) == 1 and "invdepth_mode 3" in err()
    assert _warp_backward(lib, C=0) == 1 and _warp_backward(lib, C=257) == 1 and "C=257" in err()
    assert _warp_backward(lib, V=0) == 1 and _warp_backward(lib, S=0) == 1 and "bad dimensions" in err()


def test_sweep_corr_autograd_refuses_unsupported_channels_before_any_gpu_call():
    """C = 320 is a forward-only channel count: asked for a gradient, sweep_corr_autograd raises when it is CALLED (CPU tensors
    reach the check, so nothing has touched a device), not from inside backward(); without a gradient to come it goes on to the
    forward (which refuses the CPU tensors)"""
    from robustmvd_amd import ops
    K, Tm, inv = torch.eye(3)[None], torch.eye(4)[None], torch.ones(1, 4)
    for C in (320, 512):
        key, src = torch.zeros(1, C, 4, 4, requires_grad=True), torch.zeros(1, C, 4, 4)
        for a, b in ((key, src), (src, key)):
            with pytest.raises(ValueError, match=f"C={C}.*64, 128, 192, 256"):
                ops.sweep_corr_autograd(a, [b], K, [K], [Tm], inv)
        with torch.no_grad(), pytest.raises(ValueError, match="cuda"):
            ops.sweep_corr_autograd(key, [src], K, [K], [Tm], inv)
        with pytest.raises(ValueError, match="cuda"):
            ops.sweep_corr_autograd(src, [src], K, [K], [Tm], inv)
    with pytest.raises(ValueError, match="cuda"):  # a supported count passes the check
        ops.sweep_corr_autograd(torch.zeros(1, 256, 4, 4, requires_grad=True), [torch.zeros(1, 256, 4, 4)], K, [K], [Tm], inv)


# ------------------------------------------------------------------------------------------------ (c) inference entries
def test_inference_entries_still_refuse_grad():
    """ops.inference_only is unchanged: the inference entries raise on an input that requires grad while autograd records (the
    check comes before any device work, so CPU tensors do), and accept it under no_grad (then fail later, on the device check)."""
    from robustmvd_amd import ops, sweep_modes as SM
    x = torch.zeros(1, 4, 4, 4, requires_grad=True)
    M = torch.zeros(1, 3, 4)
    with pytest.raises(RuntimeError, match="inference-only"):
        SM.sweep_reduce_inference(x, [x], [M], torch.ones(1, 2), 0)
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.sweep_warp([x], torch.zeros(1, 3, 3), [torch.zeros(1, 3, 3)], [torch.zeros(1, 4, 4)], torch.ones(1, 2), (4, 4))
    with torch.no_grad(), pytest.raises(ValueError, match="cuda"):
        SM.sweep_reduce_inference(x, [x], [M], torch.ones(1, 2), 0)
    # without a feature that requires grad the public entry is the inference one (a CPU tensor reaches its device check)
    with pytest.raises(ValueError, match="cuda"):
        SM.sweep_reduce(x.detach(), [x.detach()], [M], torch.ones(1, 2), 0)
    # the warp-only block keeps refusing grad unless it was built differentiable
    import robustmvd_amd as R
    with pytest.raises(ValueError, match="differentiable=True"):
        R.PlanesweepCorrelation(warp_only=True)(x, torch.zeros(1, 3, 3), [x], [torch.zeros(1, 4, 4)], sampling_invdepths=torch.ones(1, 2))
