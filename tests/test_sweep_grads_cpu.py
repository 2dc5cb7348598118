"""CPU side of the differentiable sweep consumers (mvd_sweep_reduce_backward_f32, mvd_sweep_warp_backward_f32):

(a) a float64 restatement of the three sweep reductions and of the warp-only sweep, local to this module, whose autograd
    gradients are pinned against the reference's own (tests/golden/g15_sweep_grads.npz).  The GPU tests
    (tests/test_hip_sweep_grads.py) use it as their checker on the shapes the reference was never run on;
(b) the argument validation of the two C entry points, which runs before any GPU call;
(c) the inference entries still refuse an input that requires grad (ops.inference_only).

The restatement computes the sampling positions in float32 with the kernels' formulas (a fused multiply-add is taken as the
float64 product and sum rounded to float32) and gathers by index in float64 under autograd."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
import gen_common as gc

f32 = np.float32


# ------------------------------------------------------------------------------------------------ the restatement
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


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
    (B,D,h,w) float32 weights (nw, ne, sw, se) -> (B,C,D,h,w) float64 samples, differentiable w.r.t. src."""
    P = torch.nn.functional.pad(src, (1, 2, 1, 2))
    out = []
    for b in range(src.shape[0]):
        y0, x0 = torch.from_numpy(cell_y[b].astype(np.int64)), torch.from_numpy(cell_x[b].astype(np.int64))
        w4 = [torch.from_numpy(wk[b].astype(np.float64)) for wk in wts]
        out.append(P[b][:, y0, x0] * w4[0] + P[b][:, y0, x0 + 1] * w4[1] + P[b][:, y0 + 1, x0] * w4[2] + P[b][:, y0 + 1, x0 + 1] * w4[3])
    return torch.stack(out)


def reduce_sample(src, M, depth, pix_offset, stretch):
    h, w = src.shape[-2:]
    ix, iy = reduce_positions(M, depth, h, w, pix_offset, stretch)
    xf, yf = np.floor(ix), np.floor(iy)
    wx, wy = ix - xf, iy - yf
    ux, uy = f32(1) - wx, f32(1) - wy
    return _gather4(src, yf.astype(np.int64) + 1, xf.astype(np.int64) + 1, (ux * uy, wx * uy, ux * wy, wx * wy))


def sweep_reduce_restated(key, srcs, Ms, depth, mode, groups=1, pix_offset=0.0, stretch=True):
    """key, srcs: float64 tensors (B,C,h,w); Ms, depth: float32 arrays.  mode "variance" | "keysq" | "groupcorr"."""
    sv = [reduce_sample(s, M, depth, pix_offset, stretch) for s, M in zip(srcs, Ms)]
    k = key.unsqueeze(2)
    if mode == "groupcorr":
        B, C, D, h, w = sv[0].shape
        return [(k * s).view(B, groups, C // groups, D, h, w).sum(2) for s in sv]
    N = len(srcs) + 1
    s2 = k * k + sum(s * s for s in sv)
    s1 = (k * k if mode == "keysq" else k) + sum(sv)
    return s2 / N - (s1 / N) ** 2


def warp_cells(K_key, K_src, T, invd, h, w, hs, ws):
    """sweep_epipolar.h's grid chain in float32, one rounding per operation: K_* (N,3,3) relative intrinsics, T (N,4,4),
    invd (1 or N, S) -> cell_y, cell_x (N,S,h,w), four tap weights (zero where out of bounds) and the 0/1 sampling mask."""
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
    ds = np.broadcast_to(invd, (N, invd.shape[1]))[:, :, None, None]
    with np.errstate(all="ignore"):
        den = k_inf + Em * ds
        us, vs = (u_inf + Ee * ds) / den, (v_inf + Ei * ds) / den

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
    return cell_y, cell_x, wts, mask


def sweep_warp_restated(srcs, K_key, K_srcs, Ts, invd, key_size, normalize=False):
    """PlanesweepCorrelation(warp_only=True): srcs float64 tensors (N,C,hs,ws) -> (warped[V] (N,S,C,h,w) float64, masks[V])."""
    h, w = key_size
    nrm = lambda x, dim: x / (torch.linalg.norm(x, dim=dim, keepdim=True) + 1e-9)
    warped, masks = [], []
    for s, Ks, T in zip(srcs, K_srcs, Ts):
        hs, ws = s.shape[-2:]
        if normalize == "before":
            s = nrm(s, 1)
        cy, cx, wts, mask = warp_cells(K_key, Ks, T, invd, h, w, hs, ws)
        x = _gather4(s, cy, cx, wts).transpose(1, 2)  # (N,S,C,h,w)
        if normalize is True or normalize == "after":
            x = nrm(x, 2)
        warped.append(x * torch.from_numpy(mask.astype(np.float64)).unsqueeze(2))
        masks.append(mask)
    return warped, masks


def grads_of(outs, cots, inputs):
    """autograd.grad of sum_i sum(outs[i] * cots[i]) w.r.t. inputs -> float32 arrays."""
    loss = sum((o * torch.from_numpy(np.asarray(c, np.float64))).sum() for o, c in zip(outs, cots))
    return [x.numpy().astype(f32) for x in torch.autograd.grad(loss, inputs)]


def leaf64(a):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)


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
