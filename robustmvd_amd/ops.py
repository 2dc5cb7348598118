"""Operator-level entry points of the HIP engine on torch (ROCm) tensors.  Each function validates its
arguments in Python (ValueError), allocates outputs/workspace with torch and launches one C-ABI function of
libmvd_hip.so on the tensor's device and torch's current stream, through call.

The first part holds the inference entry points: an input that requires grad while autograd is recording raises
(see inference_only).  The second part holds their differentiable forms (*_autograd), torch.autograd.Function wrappers
whose backward runs the engine's gradient kernels.
"""
import ctypes
import functools
import itertools

import torch

from . import _lib as L
from .mesh import check_triangles


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            yield from _tensors(o)
    elif isinstance(obj, dict):
        for o in obj.values():
            yield from _tensors(o)


def inference_only(fn):
    """The HIP kernels behind this entry point have no backward.  The reference's ops are differentiable
    (planesweep_corr.py:514-521, learned_fusion.py:24-54), so cutting the graph silently would train a model with
    wrong gradients: with autograd recording and an input that requires grad this raises instead.  Otherwise the
    call runs under torch.no_grad()."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        if torch.is_grad_enabled():
            if any(t.requires_grad for t in _tensors((args, kwargs))):
                raise RuntimeError(f"{fn.__qualname__}: an input requires grad, but this HIP path is inference-only (no "
                                   "backward is implemented); call it under torch.no_grad() or detach the inputs")
            # a bound nn.Module method (FeatureNet.forward_layout, CostRegNet.forward ...): `self` carries the parameters.
            # The reference's module is trainable; in training mode with autograd recording a silent no_grad forward would
            # hand back graph-less outputs
            owner = args[0] if args and isinstance(args[0], torch.nn.Module) else None
            if owner is not None and owner.training and any(p.requires_grad for p in owner.parameters()):
                raise RuntimeError(f"{fn.__qualname__}: the module is in training mode with trainable parameters and autograd is "
                                   "recording, but this HIP path is inference-only; call .eval() and run it under torch.no_grad()")
        with torch.no_grad():
            return fn(*args, **kwargs)
    return wrapper


def call(name, dev, *args):
    """Launches the C entry point `name` (any one that returns a status) on `dev` and torch's current stream of it.  args: the
    header's arguments in order, without the trailing stream.  Ints and floats go as they are and None as a NULL pointer; a
    tensor goes as its device address (L.ptr's value); a list or tuple of tensors goes as a void** array, which lives until
    the call has returned.  A non-zero status raises `name failed (status N): <mvd_last_error>`."""
    argv, keep = list(args), []
    for i, a in enumerate(args):
        t = type(a)
        # every launch of a frame passes here, most arguments are ints: asking isinstance(a, torch.Tensor) of each of them
        # first cost 0.08 ms of the 1.1 ms a robust_mvd frame takes to enqueue
        if t is int or t is float or a is None:
            continue
        if t is list or t is tuple:
            argv[i], arr = L.ptr_array(a)
            keep.append(arr)
        elif isinstance(a, torch.Tensor):
            argv[i] = a.data_ptr()
    with torch.cuda.device(dev):
        rc = getattr(L.load(), name)(*argv, L.raw_stream(dev))
    L.check(rc, name)


def views(ts, name, V=None):
    """The per-view arguments of an op as a list of 1..MVD_MAX_VIEWS entries (of V entries, where V is given)."""
    ts = list(ts)
    if len(ts) == 0 or len(ts) > L.MVD_MAX_VIEWS:
        raise ValueError(f"{name}: {len(ts)} views, supported 1..{L.MVD_MAX_VIEWS}")
    if V is not None and len(ts) != V:
        raise ValueError(f"{name}: {len(ts)} entries for {V} views")
    return ts


def workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _invdepth_mode(inv, N, h, w):
    """(1,S) shared, (N,S) per batch element, or (N,S,h,w) per key pixel (planesweep_corr.py:465-487)."""
    if inv.dim() == 2 and inv.shape[0] in (1, N):
        return L.INVDEPTH_BATCHED if (inv.shape[0] == N and N > 1) else L.INVDEPTH_SHARED
    if inv.dim() == 4 and tuple(inv.shape[0:1] + inv.shape[2:]) == (N, h, w):
        return L.INVDEPTH_PER_PIXEL
    raise ValueError(f"sampling_invdepths must be (1 or N, S) or (N, S, h, w), got {tuple(inv.shape)}")


def _k1_calibration(K_key, K_sources, T_src2key, invdepths, V, N, h, w, dev):
    """K1's calibration arguments, validated: relative intrinsics (N,3,3) of the key view and of the V source views, V
    source-to-key transforms (N,4,4) and the inverse depths -> (Kk, Ks, Ts, inv, the inverse depths' INVDEPTH_* mode)."""
    Kk = L.as_f32(K_key, "intrinsics_key", (N, 3, 3), dev)
    Ks = [L.as_f32(k, f"intrinsics_sources[{i}]", (N, 3, 3), dev) for i, k in enumerate(views(K_sources, "intrinsics_sources", V))]
    Ts = [L.as_f32(t, f"source_to_key_transforms[{i}]", (N, 4, 4), dev) for i, t in enumerate(views(T_src2key, "source_to_key_transforms", V))]
    inv = L.as_f32(invdepths, "sampling_invdepths", device=dev)
    return Kk, Ks, Ts, inv, _invdepth_mode(inv, N, h, w)


def _corr_scale(corr_scale, C):
    """The multiplier of K1's dot products: 1/sqrt(C) (normalize="dim") unless the caller gives one."""
    return float(corr_scale) if corr_scale is not None else 1.0 / float(C) ** 0.5


def _k3_depths(depth_values, B, C, dev):
    """K3's depth samples (B,D), validated together with the channel count C, which must be one the kernels are built for."""
    dv = L.as_f32(depth_values, "depth_values", device=dev)
    if dv.dim() != 2 or dv.shape[0] != B:
        raise ValueError(f"depth_values must be (B,D), got {tuple(dv.shape)}")
    if C not in (4, 8, 16, 32, 64):
        raise ValueError(f"feature channels C={C} unsupported (4, 8, 16, 32, 64)")
    return dv


def _k3_calibration(src_projs, key_proj_inv, depth_values, V, B, C, dev):
    """K3's calibration arguments, validated: V source projections and the inverse key projection (B,4,4), and _k3_depths
    -> (projs, kpi, dv)."""
    projs = [L.as_f32(p, f"src_projs[{i}]", (B, 4, 4), dev) for i, p in enumerate(views(src_projs, "src_projs", V))]
    kpi = L.as_f32(key_proj_inv, "key_proj_inv", (B, 4, 4), dev)
    return projs, kpi, _k3_depths(depth_values, B, C, dev)


@inference_only
def sweep_corr(feat_key, feat_sources, K_key, K_sources, T_src2key, invdepths, corr_scale=None):
    """K1. feat_key (N,C,h,w); feat_sources V x (N,C,hs,ws); K_* relative intrinsics (N,3,3);
    T_src2key V x (N,4,4); invdepths (1 or N, S) or per key pixel (N,S,h,w); corr_scale: multiplier of the dot products,
    default 1/sqrt(C) (normalize="dim").  Returns (corrs[V], masks[V]) each (N,S,h,w)."""
    fk = L.as_f32(feat_key, "feat_key")
    if fk.dim() != 4:
        raise ValueError("feat_key must be (N,C,h,w)")
    N, C, h, w = fk.shape
    dev = fk.device
    srcs = views(feat_sources, "feat_sources")
    V = len(srcs)
    hs, ws = srcs[0].shape[-2:]
    srcs = [L.as_f32(s, f"feat_sources[{i}]", (N, C, hs, ws), dev) for i, s in enumerate(srcs)]
    Kk, Ks, Ts, inv, mode = _k1_calibration(K_key, K_sources, T_src2key, invdepths, V, N, h, w, dev)
    S = inv.shape[1]
    scale = _corr_scale(corr_scale, C)
    if C % 64 != 0:
        raise ValueError(f"feature channels C={C} must be a multiple of 64")
    corrs = [torch.empty((N, S, h, w), dtype=torch.float32, device=dev) for _ in range(V)]
    masks = [torch.empty((N, S, h, w), dtype=torch.float32, device=dev) for _ in range(V)]
    wsb = L.load().mvd_sweep_corr_workspace_bytes(N, C, h, w, hs, ws, V)
    call("mvd_sweep_corr_ex_f32", dev, fk, srcs, Kk, Ks, Ts, inv, mode, scale, N, C, h, w, hs, ws, S, V, corrs, masks,
          workspace(wsb, dev), wsb)
    return corrs, masks


@inference_only
def sweep_warp(feat_sources, K_key, K_sources, T_src2key, invdepths, key_size, normalize_after=False):
    """WarpOnlyCorr's sweep (planesweep_corr.py:107-140).  feat_sources V x (N,C,hs,ws); key_size (h, w) of the key feature
    map; invdepths as in sweep_corr.  Returns (warped[V] (N,S,C,h,w), masks[V] (N,S,h,w))."""
    srcs = views(feat_sources, "feat_sources")
    V = len(srcs)
    s0 = L.as_f32(srcs[0], "feat_sources[0]")
    if s0.dim() != 4:
        raise ValueError("feat_sources must be (N,C,hs,ws)")
    N, C, hs, ws = s0.shape
    dev = s0.device
    h, w = int(key_size[0]), int(key_size[1])
    srcs = [L.as_f32(s, f"feat_sources[{i}]", (N, C, hs, ws), dev) for i, s in enumerate(srcs)]
    Kk, Ks, Ts, inv, mode = _k1_calibration(K_key, K_sources, T_src2key, invdepths, V, N, h, w, dev)
    S = inv.shape[1]
    outs = [torch.empty((N, S, C, h, w), dtype=torch.float32, device=dev) for _ in range(V)]
    masks = [torch.empty((N, S, h, w), dtype=torch.float32, device=dev) for _ in range(V)]
    call("mvd_sweep_warp_f32", dev, srcs, Kk, Ks, Ts, inv, mode, 1 if normalize_after else 0, N, C, h, w, hs, ws, S, V, outs, masks)
    return outs, masks


@inference_only
def fuse_views(corrs, masks, scores):
    """K2. corrs, masks V x (N,S,h,w); scores V x (N,1,h,w) -> fused, fused_mask (N,S,h,w)."""
    corrs = views(corrs, "corrs")
    V = len(corrs)
    c0 = L.as_f32(corrs[0], "corrs[0]")
    N, S, h, w = c0.shape
    dev = c0.device
    corrs = [L.as_f32(c, f"corrs[{i}]", (N, S, h, w), dev) for i, c in enumerate(corrs)]
    masks = [L.as_f32(m, f"masks[{i}]", (N, S, h, w), dev) for i, m in enumerate(views(masks, "masks", V))]
    scores = [L.as_f32(s, f"scores[{i}]", (N, 1, h, w), dev) for i, s in enumerate(views(scores, "scores", V))]
    fused = torch.empty_like(c0)
    fmask = torch.empty_like(c0)
    call("mvd_fuse_views_f32", dev, corrs, masks, scores, N, S, h, w, V, fused, fmask)
    return fused, fmask


@inference_only
def warp_variance(key_feat, src_feats, src_projs, key_proj_inv, depth_values, channels_last=False, exact_grid=False,
                  staged=False, return_absmax=False):
    """K3. key_feat (B,C,h,w); src_feats V x (B,C,h,w); src_projs V x (B,4,4); key_proj_inv (B,4,4);
    depth_values (B,D).  Returns the variance volume (B,C,D,h,w), or (B,D,h,w,C) if channels_last.
    return_absmax: also returns max |volume| as a one-element device tensor (a by-product of the store epilogue for
    C = 32 channel-last), which conv3d_bn_relu_split takes as its activation range.
    exact_grid: sampling positions follow the reference's operation chain rounding for rounding (MVD_GRID_EXACT).
    staged: the feature maps are the zero-bordered channel-last (B,h+3,w+3,C) copies K6 writes
    (conv2d_bn_relu(..., out_layout=LAYOUT_NHWC_BORDER)); the re-packing launches are skipped (MVD_FEAT_NHWC_BORDER)."""
    kf = L.as_f32(key_feat, "key_feat")
    if kf.dim() != 4:
        raise ValueError("key_feat must be (B,C,h,w)" + (" / (B,h+3,w+3,C) when staged" if staged else ""))
    if staged:
        B, h, w, C = kf.shape[0], kf.shape[1] - 3, kf.shape[2] - 3, kf.shape[3]
    else:
        B, C, h, w = kf.shape
    dev = kf.device
    srcs = [L.as_f32(s, f"src_feats[{i}]", tuple(kf.shape), dev) for i, s in enumerate(views(src_feats, "src_feats"))]
    V = len(srcs)
    projs, kpi, dv = _k3_calibration(src_projs, key_proj_inv, depth_values, V, B, C, dev)
    D = dv.shape[1]
    out = torch.empty((B, D, h, w, C) if channels_last else (B, C, D, h, w), dtype=torch.float32, device=dev)
    wsb = L.load().mvd_warp_variance_workspace_bytes(B, C, h, w, 0 if staged else V)
    flags = (L.LAYOUT_NDHWC if channels_last else L.LAYOUT_NCDHW) | (L.GRID_EXACT if exact_grid else 0) | \
        (L.FEAT_NHWC_BORDER if staged else 0)
    name, amax = "mvd_warp_variance_f32", []
    if return_absmax:  # the twin takes one more pointer, behind the volume
        name, amax = "mvd_warp_variance_absmax_f32", [torch.empty(1, dtype=torch.float32, device=dev)]
    call(name, dev, kf, srcs, projs, kpi, dv, B, C, D, h, w, V, out, *amax, flags, workspace(wsb, dev), wsb)
    return (out, amax[0]) if return_absmax else out


@inference_only
def absmax(x):
    """max |x| over a float32 device tensor as a one-element device tensor (NaNs ignored; a streaming read)."""
    x = L.as_f32(x, "x")
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    call("mvd_absmax_f32", x.device, x, x.numel(), out)
    return out


@inference_only
def to_f16(x):
    """fp32 -> fp16 (round to nearest even) through the library's converter; numel must be a multiple of 4."""
    x = L.as_f32(x, "x")
    y = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    call("mvd_convert_f32_to_f16", x.device, x, y, x.numel())
    return y


@inference_only
def warp_variance_f16(key_feat, src_feats, src_projs, key_proj_inv, depth_values):
    """K3, fp16-feature variant.  key_feat, src_feats: fp16 zero-bordered channel-last maps
    (B,h+3,w+3,32); calibration fp32.  Returns the fp16 channel-last variance volume (B,D,h,w,32)."""
    kf = L.as_f16(key_feat, "key_feat")
    if kf.dim() != 4 or kf.shape[3] != 32:
        raise ValueError("key_feat must be the fp16 zero-bordered channel-last map (B,h+3,w+3,32)")
    B, h, w = kf.shape[0], kf.shape[1] - 3, kf.shape[2] - 3
    dev = kf.device
    srcs = [L.as_f16(s, f"src_feats[{i}]", tuple(kf.shape), dev) for i, s in enumerate(views(src_feats, "src_feats"))]
    V = len(srcs)
    projs, kpi, dv = _k3_calibration(src_projs, key_proj_inv, depth_values, V, B, 32, dev)
    D = dv.shape[1]
    out = torch.empty((B, D, h, w, 32), dtype=torch.float16, device=dev)
    wsb = L.load().mvd_warp_variance_f16_workspace_bytes(B)
    call("mvd_warp_variance_f16", dev, kf, srcs, projs, kpi, dv, B, D, h, w, V, out, workspace(wsb, dev), wsb)
    return out


@inference_only
def homo_warp(src_feat, src_proj, ref_proj_inv, depth_values):
    """Drop-in for rmvd.models.blocks.utils.homo_warp (blocks/utils.py:222): -> (B,C,D,H,W)."""
    sf = L.as_f32(src_feat, "src_feat")
    if sf.dim() != 4:
        raise ValueError("src_feat must be (B,C,H,W)")
    B, C, h, w = sf.shape
    dev = sf.device
    sp = L.as_f32(src_proj, "src_proj", (B, 4, 4), dev)
    kpi = L.as_f32(ref_proj_inv, "ref_proj_inv", (B, 4, 4), dev)
    dv = _k3_depths(depth_values, B, C, dev)
    D = dv.shape[1]
    out = torch.empty((B, C, D, h, w), dtype=torch.float32, device=dev)
    wsb = L.load().mvd_warp_variance_workspace_bytes(B, C, h, w, 0)
    call("mvd_homo_warp_f32", dev, sf, sp, kpi, dv, B, C, D, h, w, out, workspace(wsb, dev), wsb)
    return out


def _conv3d_channels(weight, mode):
    """(Cin, Cout) of a 3x3x3 layer from its torch weight: Conv3d (Cout,Cin,3,3,3), or ConvTranspose3d (Cin,Cout,3,3,3) for mode
    DECONV3D_STRIDE2."""
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise ValueError(f"weight must be (*,*,3,3,3), got {tuple(weight.shape)}")
    return (weight.shape[0], weight.shape[1]) if mode == L.DECONV3D_STRIDE2 else (weight.shape[1], weight.shape[0])


def _conv3d_out_size(mode, Di, hi, wi):
    """(Do, ho, wo) of a 3x3x3 layer of `mode` on a (Di, hi, wi) volume."""
    if mode == L.CONV3D_STRIDE1:
        return Di, hi, wi
    if mode == L.CONV3D_STRIDE2:
        if Di % 2 or hi % 2 or wi % 2:
            raise ValueError(f"stride-2 conv needs even D,h,w, got {Di},{hi},{wi}")
        return Di // 2, hi // 2, wi // 2
    if mode == L.DECONV3D_STRIDE2:
        return Di * 2, hi * 2, wi * 2
    raise ValueError(f"mode {mode}")


@inference_only
def pack_conv3d_weights(weight, mode):
    """weight: Conv3d (Cout,Cin,3,3,3) or, for mode DECONV3D_STRIDE2, ConvTranspose3d (Cin,Cout,3,3,3)."""
    wt = L.as_f32(weight, "weight")
    Cin, Cout = _conv3d_channels(wt, mode)
    n = L.load().mvd_conv3d_packed_weight_floats(Cin, Cout)
    if n == 0:
        raise ValueError(f"conv3d: Cin={Cin}, Cout={Cout} unsupported (Cin in 8/16/32/64, Cout in 1/8/16/32/64; Cin 1 with Cout 4, 8 .. 64)")
    packed = torch.empty(n, dtype=torch.float32, device=wt.device)
    call("mvd_pack_conv3d_weights_f32", wt.device, wt, Cin, Cout, mode, packed)
    return packed, Cin, Cout


@inference_only
def conv3d_bn_relu(x, packed, Cin, Cout, scale, shift, mode, relu=True, skip=None, return_absmax=False):
    """K4. x (B,D,h,w,Cin) channel-last -> (B,Do,ho,wo,Cout).  return_absmax: also max |y| over the finite outputs (device,
    one float; what conv3d_bn_relu_split scales a following layer's activations by): a by-product of the store epilogue of
    the stride-2 layers, a pass over y otherwise."""
    x = L.as_f32(x, "x")
    if x.dim() != 5 or x.shape[-1] != Cin:
        raise ValueError(f"x must be (B,D,h,w,{Cin}) channel-last, got {tuple(x.shape)}")
    B, Di, hi, wi, _ = x.shape
    dev = x.device
    oshape = (B, *_conv3d_out_size(mode, Di, hi, wi), Cout)
    scale = L.as_f32(scale, "scale", (Cout,), dev)
    shift = L.as_f32(shift, "shift", (Cout,), dev)
    if skip is not None:
        skip = L.as_f32(skip, "skip", oshape, dev)
    y = torch.empty(oshape, dtype=torch.float32, device=dev)
    name, amax = "mvd_conv3d_bn_relu_f32", []
    if return_absmax:  # the twin takes one more pointer, behind y
        name, amax = "mvd_conv3d_bn_relu_absmax_f32", [torch.empty(1, dtype=torch.float32, device=dev)]
    call(name, dev, x, packed, scale, shift, skip, y, *amax, B, Di, hi, wi, Cin, Cout, mode, int(bool(relu)))
    return (y, amax[0]) if return_absmax else y


@inference_only
def pack_conv3d_weights_f16(weight):
    """weight: Conv3d (8,32,3,3,3) fp32 -> fp16 MFMA-fragment-ordered buffer for conv3d_bn_relu_f16in."""
    wt = L.as_f32(weight, "weight")
    if tuple(wt.shape) != (8, 32, 3, 3, 3):
        raise ValueError(f"conv3d f16: only the 32 -> 8 first layer is built, got weight {tuple(wt.shape)}")
    packed = torch.empty(L.load().mvd_conv3d_f16_packed_weight_bytes(32, 8), dtype=torch.uint8, device=wt.device)
    call("mvd_pack_conv3d_weights_f16", wt.device, wt, 32, 8, packed)
    return packed


@inference_only
def conv3d_bn_relu_f16in(x, packed, scale, shift, relu=True):
    """K4 first layer on fp16 MFMA: x (B,D,h,w,32) fp16 channel-last -> (B,D,h,w,8) fp32."""
    x = L.as_f16(x, "x")
    if x.dim() != 5 or x.shape[-1] != 32:
        raise ValueError(f"x must be (B,D,h,w,32) fp16 channel-last, got {tuple(x.shape)}")
    B, D, h, w, _ = x.shape
    dev = x.device
    scale = L.as_f32(scale, "scale", (8,), dev)
    shift = L.as_f32(shift, "shift", (8,), dev)
    y = torch.empty((B, D, h, w, 8), dtype=torch.float32, device=dev)
    call("mvd_conv3d_bn_relu_f16in", dev, x, packed, scale, shift, y, B, D, h, w, 32, 8, int(bool(relu)))
    return y


def _split3d_inputs(x, cin, cout, out_size, scale, shift, skip, x_absmax):
    """What the 3-D split-operand wrappers check and coerce alike: x (B,D,h,w,cin) channel-last fp32, scale and shift of cout floats,
    skip None or shaped like the output (B, *out_size(D,h,w), cout), x_absmax one float.  -> x, scale, shift, skip, x_absmax, output shape."""
    x = L.as_f32(x, "x")
    if x.dim() != 5 or x.shape[-1] != cin:
        raise ValueError(f"x must be (B,D,h,w,{cin}) channel-last, got {tuple(x.shape)}")
    dev = x.device
    oshape = (x.shape[0], *out_size(*x.shape[1:4]), cout)
    scale = L.as_f32(scale, "scale", (cout,), dev)
    shift = L.as_f32(shift, "shift", (cout,), dev)
    if skip is not None:
        skip = L.as_f32(skip, "skip", oshape, dev)
    return x, scale, shift, skip, L.as_f32(x_absmax, "x_absmax", (1,), dev), oshape


def _absmax_slot(return_absmax, out_absmax, dev):
    """The one-float max |y| slot of a layer call that raises it by atomic maximum: None unless asked for; the caller's out_absmax
    (zeroed by the caller), or a fresh zeroed one."""
    if not return_absmax:
        return None
    if out_absmax is not None:
        return L.as_f32(out_absmax, "out_absmax", (1,), dev)
    return torch.zeros(1, dtype=torch.float32, device=dev)


@inference_only
def pack_conv3d_weights_split(weight):
    """weight: Conv3d (Cout,Cin,3,3,3) fp32, Cin 16 or 32, Cout in 8, 16, ... 64 -> per block of 8 output channels the
    [w_hi | w_lo] fp16 fragments for conv3d_bn_relu_split, followed by the channels' power-of-two scales."""
    wt = L.as_f32(weight, "weight")
    cout, cin = (wt.shape[0], wt.shape[1]) if wt.dim() == 5 else (0, 0)
    if wt.dim() != 5 or tuple(wt.shape[2:]) != (3, 3, 3) or cin not in (16, 32) or cout % 8 or not 8 <= cout <= 64:
        raise ValueError(f"conv3d split: 16 or 32 input channels and 8..64 output channels (a multiple of 8) are built, got weight {tuple(wt.shape)}")
    packed = torch.empty(L.load().mvd_conv3d_split_packed_weight_bytes(cin, cout), dtype=torch.uint8, device=wt.device)
    call("mvd_pack_conv3d_weights_split", wt.device, wt, cin, cout, packed)
    return packed


@inference_only
def conv3d_bn_relu_split(x, packed, scale, shift, relu=True, x_absmax=None, return_absmax=False):
    """K4's stride-1 layers with 16 or 32 input channels (conv0: 32 -> 8, conv2: 16 -> 16, conv4: 32 -> 32), split-operand
    form: x (B,D,h,w,Cin) fp32 -> (B,D,h,w,Cout) fp32 (Cout = len(scale)) on fp16 MFMA with two-term operand
    splitting and power-of-two range scaling (fp32-grade results for inputs of any
    magnitude).  x_absmax: one-element device tensor with max |x| (warp_variance(..., return_absmax=True)); computed here
    with a streaming pass over x when omitted.  return_absmax: also max |y| (one-element device tensor), a by-product of the
    store epilogue."""
    x = L.as_f32(x, "x")
    if x.dim() != 5 or x.shape[-1] not in (16, 32):
        raise ValueError(f"x must be (B,D,h,w,16 or 32) channel-last, got {tuple(x.shape)}")
    B, D, h, w, cin = x.shape
    dev = x.device
    scale = L.as_f32(scale, "scale", device=dev)
    cout = scale.numel()
    if packed.numel() != L.load().mvd_conv3d_split_packed_weight_bytes(cin, cout):
        raise ValueError(f"packed weights of {packed.numel()} bytes do not belong to a {cin} -> {cout} layer")
    shift = L.as_f32(shift, "shift", (cout,), dev)
    y = torch.empty((B, D, h, w, cout), dtype=torch.float32, device=dev)
    if x_absmax is None:
        x_absmax = absmax(x)
    x_absmax = L.as_f32(x_absmax, "x_absmax", (1,), dev)
    name, yam = "mvd_conv3d_bn_relu_f32_split", []
    if return_absmax:  # the twin takes one more pointer, behind y
        name, yam = "mvd_conv3d_bn_relu_absmax_f32_split", [torch.empty(1, dtype=torch.float32, device=dev)]
    call(name, dev, x, x_absmax, packed, scale, shift, y, *yam, B, D, h, w, cin, cout, int(bool(relu)))
    return (y, yam[0]) if return_absmax else y


@inference_only
def pack_conv3d_weights_igemm(weight, mode):
    """weight: Conv3d (Cout,Cin,3,3,3), or ConvTranspose3d (Cin,Cout,3,3,3) for mode DECONV3D_STRIDE2 -> packed split-operand
    fragments for conv3d_bn_relu_igemm."""
    wt = L.as_f32(weight, "weight")
    cin, cout = _conv3d_channels(wt, mode)
    n = L.load().mvd_conv3d_igemm_packed_weight_bytes(cin, cout, mode)
    if n == 0:
        raise ValueError(f"conv3d igemm: {cin} -> {cout} channels, mode {mode} is not built (Cin a multiple of 8 (16 transposed), Cout of 4)")
    packed = torch.empty(n, dtype=torch.uint8, device=wt.device)
    call("mvd_pack_conv3d_weights_igemm", wt.device, wt, cin, cout, mode, packed)
    return packed


@inference_only
def conv3d_bn_relu_igemm(x, x_absmax, packed, Cin, Cout, scale, shift, mode, relu=True, skip=None, return_absmax=False, out_absmax=None):
    """K4's stride-2 / transposed / wide stride-1 layers on the split-operand implicit-GEMM kernel.
    x (B,D,h,w,Cin) channel-last fp32, x_absmax one-element device tensor with max |x| -> (B,Do,ho,wo,Cout); skip (like the output)
    is added after the activation.  return_absmax: also max |y| (out_absmax: a zeroed one-element device tensor to raise instead of a
    fresh one: several layers' slots can come from one zeroed buffer)."""
    lib = L.load()
    x, scale, shift, skip, xam, oshape = _split3d_inputs(x, Cin, Cout, lambda d, h, w: _conv3d_out_size(mode, d, h, w), scale, shift, skip,
                                                         x_absmax)
    B, Di, hi, wi, _ = x.shape
    dev = x.device
    if packed.numel() != lib.mvd_conv3d_igemm_packed_weight_bytes(Cin, Cout, mode):
        raise ValueError(f"packed weights of {packed.numel()} bytes do not belong to a {Cin} -> {Cout} layer of mode {mode}")
    y = torch.empty(oshape, dtype=torch.float32, device=dev)
    yam = _absmax_slot(return_absmax, out_absmax, dev)
    wsb = lib.mvd_conv3d_igemm_workspace_bytes(B, Di, hi, wi, Cin, Cout, mode)
    call("mvd_conv3d_bn_relu_igemm_f32", dev, x, xam, packed, scale, shift, skip, y, yam, B, Di, hi, wi, Cin, Cout, mode,
          int(bool(relu)), workspace(wsb, dev) if wsb else None, wsb)
    return (y, yam) if return_absmax else y


@inference_only
def pack_deconv3d_weights_split(weight):
    """weight: ConvTranspose3d (Cin,Cout,3,3,3) fp32; Cin 32 or 64 with Cout 16, 32, 48 or 64, or 16 -> 8 -> the hi / lo fp16 fragments
    for deconv3d_bn_relu_split, followed by the channels' power-of-two scales."""
    wt = L.as_f32(weight, "weight")
    cin, cout = _conv3d_channels(wt, L.DECONV3D_STRIDE2)
    n = L.load().mvd_deconv3d_split_packed_weight_bytes(cin, cout)
    if n == 0:
        raise ValueError(f"deconv3d split: {cin} -> {cout} channels is not built (32 or 64 -> 16, 32, 48 or 64; 16 -> 8)")
    packed = torch.empty(n, dtype=torch.uint8, device=wt.device)
    call("mvd_pack_deconv3d_weights_split", wt.device, wt, cin, cout, packed)
    return packed


@inference_only
def deconv3d_bn_relu_split(x, x_absmax, packed, Cin, Cout, scale, shift, relu=True, skip=None, return_absmax=False, out_absmax=None):
    """K4's transposed layers (conv7: 64 -> 32, conv9: 32 -> 16, conv11: 16 -> 8), split-operand form: x (B,D,h,w,Cin) channel-last
    fp32, x_absmax one-element device tensor with max |x| -> (B,2D,2h,2w,Cout); skip (like the output) is added after the
    activation.  return_absmax: also max |y| over the finite outputs, a by-product of the store epilogue (out_absmax: a zeroed
    one-element device tensor to raise instead of a fresh one)."""
    x, scale, shift, skip, xam, oshape = _split3d_inputs(x, Cin, Cout, lambda d, h, w: (2 * d, 2 * h, 2 * w), scale, shift, skip, x_absmax)
    B, Di, hi, wi, _ = x.shape
    dev = x.device
    n = L.load().mvd_deconv3d_split_packed_weight_bytes(Cin, Cout)
    if n == 0 or packed.numel() != n:
        raise ValueError(f"packed weights of {packed.numel()} bytes do not belong to a transposed {Cin} -> {Cout} layer")
    y = torch.empty(oshape, dtype=torch.float32, device=dev)
    yam = _absmax_slot(return_absmax, out_absmax, dev)
    call("mvd_deconv3d_bn_relu_f32_split", dev, x, xam, packed, scale, shift, skip, y, yam, B, Di, hi, wi, Cin, Cout, int(bool(relu)))
    return (y, yam) if return_absmax else y


@inference_only
def pack_conv2d_weights(weight):
    """weight: Conv2d (Cout,Cin,k,k), k in (3, 5) -> (packed, Cin, Cout, k)."""
    wt = L.as_f32(weight, "weight")
    if wt.dim() != 4 or wt.shape[2] != wt.shape[3]:
        raise ValueError(f"weight must be (Cout,Cin,k,k), got {tuple(wt.shape)}")
    Cout, Cin, k = wt.shape[0], wt.shape[1], wt.shape[2]
    n = L.load().mvd_conv2d_packed_weight_floats(Cin, Cout, k)
    if n == 0:
        raise ValueError(f"conv2d: Cin={Cin}, Cout={Cout}, k={k} unsupported (Cin in 3/8/16/32, Cout in 8/16/32, k in 3/5)")
    packed = torch.empty(n, dtype=torch.float32, device=wt.device)
    call("mvd_pack_conv2d_weights_f32", wt.device, wt, Cin, Cout, k, packed)
    return packed, Cin, Cout, k


@inference_only
def conv2d_head(image, w0, scale0, shift0, w1, scale1, shift1, return_absmax=False):
    """FeatureNet's conv0 -> conv1 in one launch.  image (B,3,H,W); w0 (3,3,3,8), w1 (3,3,8,8): the Conv2d
    weights as [ky][kx][cin][cout]; folded BN scale / shift (8) per layer.  Returns (B,H,W,8) channel-last; with return_absmax also
    max |y| as a one-element device tensor (per-tile maxima from the kernel, reduced by a pass over that small array)."""
    x = L.as_f32(image, "image")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"image must be (B,3,H,W), got {tuple(x.shape)}")
    B, _, H, W = x.shape
    dev = x.device
    w0 = L.as_f32(w0, "w0", (3, 3, 3, 8), dev)
    w1 = L.as_f32(w1, "w1", (3, 3, 8, 8), dev)
    vs = [L.as_f32(v, n, (8,), dev) for v, n in ((scale0, "scale0"), (shift0, "shift0"), (scale1, "scale1"), (shift1, "shift1"))]
    y = torch.empty((B, H, W, 8), dtype=torch.float32, device=dev)
    tiles = torch.empty(L.load().mvd_conv2d_head_tile_count(B, H, W), dtype=torch.float32, device=dev) if return_absmax else None
    call("mvd_conv2d_head_f32", dev, x, w0, vs[0], vs[1], w1, vs[2], vs[3], y, tiles, B, H, W)
    return (y, absmax(tiles)) if return_absmax else y


@inference_only
def pack_conv2d_head_weights_split(weight1):
    """conv1's Conv2d weight (8,8,3,3) fp32 -> the [w_hi | w_lo] fp16 fragments of conv2d_head_split, followed by the channels'
    power-of-two scales.  Once per model."""
    wt = L.as_f32(weight1, "weight1")
    if tuple(wt.shape) != (8, 8, 3, 3):
        raise ValueError(f"conv2d_head split: conv1's weight is (8,8,3,3), got {tuple(wt.shape)}")
    packed = torch.empty(L.load().mvd_conv2d_head_split_packed_bytes(), dtype=torch.uint8, device=wt.device)
    call("mvd_pack_conv2d_head_split_weights", wt.device, wt, packed)
    return packed


@inference_only
def conv2d_head_split(image, w0, scale0, shift0, w1_packed, scale1, shift1, return_absmax=False):
    """conv2d_head with conv1 on the fp16 matrix instruction (split operands, fp32 accumulation; fp32-grade).  w1_packed:
    pack_conv2d_head_weights_split of conv1's weight; everything else as conv2d_head."""
    x = L.as_f32(image, "image")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"image must be (B,3,H,W), got {tuple(x.shape)}")
    B, _, H, W = x.shape
    dev = x.device
    w0 = L.as_f32(w0, "w0", (3, 3, 3, 8), dev)
    n = L.load().mvd_conv2d_head_split_packed_bytes()
    if w1_packed.dtype != torch.uint8 or w1_packed.numel() != n or w1_packed.device != dev or not w1_packed.is_contiguous():
        raise ValueError(f"w1_packed: pack_conv2d_head_weights_split's {n} bytes on {dev} expected")
    vs = [L.as_f32(v, n_, (8,), dev) for v, n_ in ((scale0, "scale0"), (shift0, "shift0"), (scale1, "scale1"), (shift1, "shift1"))]
    y = torch.empty((B, H, W, 8), dtype=torch.float32, device=dev)
    tiles = torch.empty(L.load().mvd_conv2d_head_tile_count(B, H, W), dtype=torch.float32, device=dev) if return_absmax else None
    call("mvd_conv2d_head_split_f32", dev, x, w0, vs[0], vs[1], w1_packed, vs[2], vs[3], y, tiles, B, H, W)
    return (y, absmax(tiles)) if return_absmax else y


def conv2d_bn_relu(x, packed, Cin, Cout, ksize, stride, scale, shift, relu=True, out_layout=L.LAYOUT_NHWC, out=None, out_absmax=None):
    """K6. x: (B,3,H,W) image when Cin == 3, else channel-last (B,h,w,Cin).  Returns (B,ho,wo,Cout) for LAYOUT_NHWC,
    (B,Cout,ho,wo) for LAYOUT_NCHW, or the zero-bordered (B,ho+3,wo+3,Cout) staging map for LAYOUT_NHWC_BORDER
    (`out` may pass a buffer whose border is already zero; only the interior is written).  out_absmax: a zeroed one-element
    device tensor that is raised to max |y|, for a split-operand layer behind this one."""
    x = L.as_f32(x, "x")
    if Cin == 3:
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"x must be (B,3,H,W), got {tuple(x.shape)}")
        B, _, hi, wi = x.shape
        in_layout = L.LAYOUT_NCHW
    else:
        if x.dim() != 4 or x.shape[-1] != Cin:
            raise ValueError(f"x must be (B,h,w,{Cin}) channel-last, got {tuple(x.shape)}")
        B, hi, wi, _ = x.shape
        in_layout = L.LAYOUT_NHWC
    if (ksize, stride) not in ((3, 1), (5, 2)):
        raise ValueError(f"conv2d: kernel {ksize} stride {stride} unsupported (3/1 or 5/2)")
    dev = x.device
    ho, wo = (hi - 1) // stride + 1, (wi - 1) // stride + 1
    oshape = {L.LAYOUT_NHWC: (B, ho, wo, Cout), L.LAYOUT_NCHW: (B, Cout, ho, wo),
              L.LAYOUT_NHWC_BORDER: (B, ho + 3, wo + 3, Cout)}.get(out_layout)
    if oshape is None:
        raise ValueError(f"out_layout {out_layout}")
    scale = L.as_f32(scale, "scale", (Cout,), dev)
    shift = L.as_f32(shift, "shift", (Cout,), dev)
    if out is not None:
        y = L.as_f32(out, "out", oshape, dev)
        if y.data_ptr() != out.data_ptr():
            raise ValueError("out must be a contiguous fp32 tensor")
    elif out_layout == L.LAYOUT_NHWC_BORDER:
        y = torch.zeros(oshape, dtype=torch.float32, device=dev)
    else:
        y = torch.empty(oshape, dtype=torch.float32, device=dev)
    name, yam = "mvd_conv2d_bn_relu_f32", []
    if out_absmax is not None:  # the twin takes one more pointer, behind y
        name, yam = "mvd_conv2d_bn_relu_absmax_f32", [L.as_f32(out_absmax, "out_absmax", (1,), dev)]
    call(name, dev, x, in_layout, packed, scale, shift, y, *yam, out_layout, B, hi, wi, Cin, Cout, ksize, stride, int(bool(relu)))
    return y


@inference_only
def softmax_regress(cost, depth_values, with_confidence=True):
    """K5. cost (B,D,h,w); depth_values (B,D) -> depth (B,h,w), confidence (B,h,w) or None."""
    c = L.as_f32(cost, "cost")
    if c.dim() != 4:
        raise ValueError("cost must be (B,D,h,w)")
    B, D, h, w = c.shape
    dv = L.as_f32(depth_values, "depth_values", (B, D), c.device)
    depth = torch.empty((B, h, w), dtype=torch.float32, device=c.device)
    conf = torch.empty((B, h, w), dtype=torch.float32, device=c.device) if with_confidence else None
    call("mvd_softmax_regress_f32", c.device, c, dv, B, D, h, w, depth, conf)
    return depth, conf


@inference_only
def softmax_regress_pp(cost, depth_hypos, with_confidence=True):
    """K5 with per-pixel hypotheses (CVP-MVSNet's refinement levels). cost (B,D,h,w); depth_hypos (B,D,h,w) -> depth (B,h,w),
    confidence (B,h,w) or None; softmax_regress's conventions."""
    c = L.as_f32(cost, "cost")
    if c.dim() != 4:
        raise ValueError("cost must be (B,D,h,w)")
    B, D, h, w = c.shape
    dh = L.as_f32(depth_hypos, "depth_hypos", (B, D, h, w), c.device)
    depth = torch.empty((B, h, w), dtype=torch.float32, device=c.device)
    conf = torch.empty((B, h, w), dtype=torch.float32, device=c.device) if with_confidence else None
    call("mvd_softmax_regress_pp_f32", c.device, c, dh, B, D, h, w, depth, conf)
    return depth, conf


@inference_only
def sweep_reduce_nhwc(key_feat, src_feats, Ms, depth, mode, pix_offset=0.0, stretch=True):
    """The variance modes of sweep_modes.sweep_reduce on the engine's own layouts, without repacking: key_feat (B,h,w,C) channel-last;
    src_feats V x (B,h+3,w+3,C) channel-last, zero-bordered with the map at (1,1) (what conv2d_split writes with
    out=buf[:, 1:h+1, 1:w+1, :]); Ms V x (B,3,4) [R|t]; depth (B,D) or (B,D,h,w); mode REDUCE_VARIANCE or REDUCE_VARIANCE_KEYSQ.
    Returns the volume (B,D,h,w,C) channel-last, bit-identical to sweep_reduce's (B,C,D,h,w) permuted."""
    if mode not in (L.REDUCE_VARIANCE, L.REDUCE_VARIANCE_KEYSQ):
        raise ValueError(f"sweep_reduce_nhwc: mode {mode} (the variance modes only)")
    kf = L.as_f32(key_feat, "key_feat")
    if kf.dim() != 4 or kf.shape[3] % 4 or kf.shape[3] > 64:
        raise ValueError(f"key_feat must be (B,h,w,C) channel-last with C a multiple of 4 up to 64, got {tuple(kf.shape)}")
    B, h, w, C = kf.shape
    dev = kf.device
    srcs = [L.as_f32(s, f"src_feats[{i}]", (B, h + 3, w + 3, C), dev) for i, s in enumerate(views(src_feats, "src_feats"))]
    V = len(srcs)
    Ms = [L.as_f32(m, f"Ms[{i}]", (B, 3, 4), dev) for i, m in enumerate(views(Ms, "Ms", V))]
    dv = L.as_f32(depth, "depth", device=dev)
    if dv.dim() == 2 and dv.shape[0] == B:
        per_pixel, D = 0, dv.shape[1]
    elif dv.dim() == 4 and dv.shape[0] == B and tuple(dv.shape[2:]) == (h, w):
        per_pixel, D = 1, dv.shape[1]
    else:
        raise ValueError(f"depth must be (B,D) or (B,D,h,w), got {tuple(dv.shape)}")
    sx, sy = (w / (w - 1), h / (h - 1)) if stretch else (1.0, 1.0)
    out = torch.empty((B, D, h, w, C), dtype=torch.float32, device=dev)
    call("mvd_sweep_reduce_nhwc_f32", dev, kf, srcs, Ms, dv, per_pixel, float(pix_offset), float(sx), float(sy), -0.5, mode,
         B, C, D, h, w, V, out)
    return out


@inference_only
def sweep_groupcorr_nhwc(key_feat, src_feats, Ms, depth, groups, pix_offset=0.0, stretch=True, grid_clamp=0.0, out=None):
    """sweep_modes.sweep_reduce's REDUCE_GROUPCORR on the engine's own layouts, without repacking (Vis-MVSNet's pair-wise cost
    volumes): key_feat (B,h,w,C) channel-last; src_feats V x (B,h+3,w+3,C) channel-last, zero-bordered with the map at (1,1);
    Ms V x (B,3,4) [R|t]; depth (B,D) or (B,D,h,w); C / groups a multiple of 4, C up to 64.  Returns V volumes (B,D,h,w,groups)
    channel-last, consecutive slices of ONE (V B,D,h,w,groups) buffer (`out`, where given), each bit-identical to sweep_reduce's
    (B,groups,D,h,w) permuted.  grid_clamp=1.1 adds the clamp of the reference's interpolate (blocks/utils.py:168: the normalised grid
    to +-1.1 before grid_sample), which changes the values on maps narrower than 10 pixels only (include/mvd.h)."""
    kf = L.as_f32(key_feat, "key_feat")
    if kf.dim() != 4 or kf.shape[3] % 4 or kf.shape[3] > 64:
        raise ValueError(f"key_feat must be (B,h,w,C) channel-last with C a multiple of 4 up to 64, got {tuple(kf.shape)}")
    B, h, w, C = kf.shape
    groups = int(groups)
    if groups < 1 or C % groups or (C // groups) % 4:
        raise ValueError(f"group correlation needs C/groups a multiple of 4, got {C}/{groups}")
    dev = kf.device
    srcs = [L.as_f32(s, f"src_feats[{i}]", (B, h + 3, w + 3, C), dev) for i, s in enumerate(views(src_feats, "src_feats"))]
    V = len(srcs)
    Ms = [L.as_f32(m, f"Ms[{i}]", (B, 3, 4), dev) for i, m in enumerate(views(Ms, "Ms", V))]
    dv = L.as_f32(depth, "depth", device=dev)
    if dv.dim() == 2 and dv.shape[0] == B:
        per_pixel, D = 0, dv.shape[1]
    elif dv.dim() == 4 and dv.shape[0] == B and tuple(dv.shape[2:]) == (h, w):
        per_pixel, D = 1, dv.shape[1]
    else:
        raise ValueError(f"depth must be (B,D) or (B,D,h,w), got {tuple(dv.shape)}")
    sx, sy = (w / (w - 1), h / (h - 1)) if stretch else (1.0, 1.0)
    if out is None:
        out = torch.empty((V * B, D, h, w, groups), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (V * B, D, h, w, groups) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 ({V * B},{D},{h},{w},{groups}) tensor on {dev}")
    outs = [out[v * B:(v + 1) * B] for v in range(V)]
    call("mvd_sweep_groupcorr_nhwc_f32", dev, kf, srcs, Ms, dv, per_pixel, float(pix_offset), float(sx), float(sy), -0.5, float(grid_clamp),
         groups, B, C, D, h, w, V, outs)
    return outs


@inference_only
def soft_argmin(score, depth_start, depth_interval, with_entropy=False, window=None):
    """Vis-MVSNet's soft argmin (blocks/utils.py:51-68) in one kernel.  score (B,D,h,w); depth_start (B) or (B,h,w) (any shape with
    B or B h w elements, e.g. the reference's n111 / n1hw); depth_interval (B) (or n111).
    Returns (depth, entropy, prob_map), each (B,h,w): depth = (sum_i i p_i) * interval + start with p = softmax_D(score);
    entropy = sum_i -p_i log(clamp(p_i, 1e-9, 1)) or None; prob_map = sum_i p_i [|i - index| <= window] or None (window=None)."""
    c = L.as_f32(score, "score")
    if c.dim() != 4:
        raise ValueError("score must be (B,D,h,w)")
    B, D, h, w = c.shape
    dev = c.device
    start = L.as_f32(depth_start, "depth_start", device=dev)
    if start.numel() == B:
        per_pixel, start = 0, start.reshape(B)
    elif start.numel() == B * h * w:
        per_pixel, start = 1, start.reshape(B, h, w)
    else:
        raise ValueError(f"depth_start must have {B} or {B}x{h}x{w} elements, got {tuple(start.shape)}")
    interval = L.as_f32(depth_interval, "depth_interval", device=dev)
    if interval.numel() != B:
        raise ValueError(f"depth_interval must have {B} elements, got {tuple(interval.shape)}")
    new = lambda: torch.empty((B, h, w), dtype=torch.float32, device=dev)
    depth, ent, prob = new(), new() if with_entropy else None, new() if window is not None else None
    call("mvd_soft_argmin_f32", dev, c, start, per_pixel, interval.reshape(B), float(window or 0.0), B, D, h, w, depth, ent, prob)
    return depth, ent, prob


@inference_only
def vis_fuse(xs, us, out=None):
    """Vis-MVSNet's "soft" fusion (vis_mvsnet_singlestage.py:263-266,302-303): xs V x (B,D,h,w,C) channel-last, C a multiple of 4;
    us V x (B,h,w) (or (B,1,h,w)) -> (sum_v x_v exp(-u_v)) / (sum_v exp(-u_v)), (B,D,h,w,C)."""
    xs = [L.as_f32(x, f"xs[{i}]") for i, x in enumerate(views(xs, "xs"))]
    if xs[0].dim() != 5 or xs[0].shape[4] % 4 or any(x.shape != xs[0].shape or x.device != xs[0].device for x in xs):
        raise ValueError(f"xs must be equal (B,D,h,w,C) channel-last volumes with C a multiple of 4, got {[tuple(x.shape) for x in xs]}")
    B, D, h, w, C = xs[0].shape
    dev = xs[0].device
    us = [L.as_f32(u, f"us[{i}]", device=dev) for i, u in enumerate(views(us, "us", len(xs)))]
    if any(u.numel() != B * h * w for u in us):
        raise ValueError(f"us must be (B,h,w) = ({B},{h},{w}) maps, got {[tuple(u.shape) for u in us]}")
    if out is None:
        out = torch.empty_like(xs[0])
    elif out.dtype != torch.float32 or out.device != dev or out.shape != xs[0].shape or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 {tuple(xs[0].shape)} tensor on {dev}")
    call("mvd_vis_fuse_f32", dev, xs, us, B, D, h, w, C, len(xs), out)
    return out


@inference_only
def geo_consistency(key_depth, src_depths, matrices, uncertainty=None, min_consistent_views=None, max_reproj_error=1.0,
                    max_rel_depth_diff=0.01, max_uncertainty=None):
    """The geometric consistency of one key depth map (H,W) against V <= 32 source maps of the same size (include/mvd.h:
    mvd_geo_consistency_f32; the reference has no counterpart).  matrices (V,24): per source A (9), b (3), A' (9), b' (3), as
    depth_fusion.compose_matrices forms them.  min_consistent_views defaults to min(3, V); the uncertainty filter applies when both
    `uncertainty` (H,W) and `max_uncertainty` are given.
    Returns (view_bits uint32, fused float32, mask uint8, num_consistent uint8), each (H,W)."""
    d = L.as_f32(key_depth, "key_depth")
    if d.dim() != 2 or d.shape[0] < 2 or d.shape[1] < 2:
        raise ValueError(f"key_depth must be (H,W) with H, W >= 2, got {tuple(d.shape)}")
    H, W = d.shape
    dev = d.device
    srcs = [L.as_f32(s, f"src_depths[{i}]", (H, W), dev) for i, s in enumerate(views(src_depths, "src_depths"))]
    V = len(srcs)
    mats = L.as_f32(matrices, "matrices", (V, 24), dev)
    unc = None
    if uncertainty is not None and max_uncertainty is not None:
        unc = L.as_f32(uncertainty, "uncertainty", (H, W), dev)
    min_views = min(3, V) if min_consistent_views is None else int(min_consistent_views)
    bits = torch.empty((H, W), dtype=torch.uint32, device=dev)
    fused = torch.empty((H, W), dtype=torch.float32, device=dev)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    count = torch.empty((H, W), dtype=torch.uint8, device=dev)
    call("mvd_geo_consistency_f32", dev, d, srcs, mats, unc, V, H, W, float(max_reproj_error), float(max_rel_depth_diff), min_views,
         float(max_uncertainty) if unc is not None else 0.0, bits, fused, mask, count)
    return bits, fused, mask, count


@inference_only
def depth_normals(depth, backproject):
    """World-frame normals (3,H,W) of one depth map (H,W) (include/mvd.h: mvd_depth_normals_f32; depth_fusion.normals_numpy is the
    definition).  backproject: the 12 floats of depth_fusion.compose_backprojection on the device.  (0,0,0) marks an invalid normal."""
    d = L.as_f32(depth, "depth")
    if d.dim() != 2:
        raise ValueError(f"depth must be (H,W), got {tuple(d.shape)}")
    H, W = d.shape
    bp = L.as_f32(backproject, "backproject", device=d.device)
    if bp.numel() != 12:
        raise ValueError(f"backproject must hold 12 floats, got {tuple(bp.shape)}")
    normals = torch.empty((3, H, W), dtype=torch.float32, device=d.device)
    call("mvd_depth_normals_f32", d.device, d, bp, H, W, normals)
    return normals


@inference_only
def geo_merge(key_depth, src_depths, matrices, key_claimed, src_claimed, uncertainty=None, min_consistent_views=None,
              max_reproj_error=1.0, max_rel_depth_diff=0.01, max_uncertainty=None, key_image=None, src_images=None, key_normal=None,
              src_normals=None):
    """geo_consistency for a scene fused view by view (include/mvd.h: mvd_geo_merge_f32; depth_fusion.merge_numpy is the definition).
    key_claimed (H,W) uint8 is read: a pixel an earlier view has claimed is not emitted.  src_claimed: V x (H,W) uint8, UPDATED IN
    PLACE: every emitted pixel sets the byte of the source pixel nearest to its projection in each consistent source.  key_image and
    src_images (planar (3,H,W)), key_normal and src_normals (depth_normals' maps) are each given together or not at all.
    Returns (view_bits, fused, mask, num_consistent, merged_rgb, merged_normal): the first four as geo_consistency's with the claimed
    pixels taken out of the mask; merged_rgb and merged_normal (3,H,W), or None without their inputs, are 0 where mask is 0."""
    d = L.as_f32(key_depth, "key_depth")
    if d.dim() != 2 or d.shape[0] < 2 or d.shape[1] < 2:
        raise ValueError(f"key_depth must be (H,W) with H, W >= 2, got {tuple(d.shape)}")
    H, W = d.shape
    dev = d.device
    srcs = [L.as_f32(s, f"src_depths[{i}]", (H, W), dev) for i, s in enumerate(views(src_depths, "src_depths"))]
    V = len(srcs)
    mats = L.as_f32(matrices, "matrices", (V, 24), dev)
    unc = None
    if uncertainty is not None and max_uncertainty is not None:
        unc = L.as_f32(uncertainty, "uncertainty", (H, W), dev)
    min_views = min(3, V) if min_consistent_views is None else int(min_consistent_views)
    # the claimed maps are written in place: they are taken as they are, never converted or made contiguous into a copy
    claims = [key_claimed] + views(src_claimed, "src_claimed", V)
    for i, c in enumerate(claims):
        name = "key_claimed" if i == 0 else f"src_claimed[{i - 1}]"
        L.as_dtype(torch.uint8, False, c, name, (H, W), dev)
        if not c.is_contiguous():
            raise ValueError(f"{name}: must be contiguous")
    if any(c.data_ptr() == key_claimed.data_ptr() for c in claims[1:]):
        raise ValueError("key_claimed is among src_claimed: a view cannot be its own source in merge mode")

    def attribute(key, srcs_, name):
        if (key is None) != (srcs_ is None):
            raise ValueError(f"key_{name} and src_{name}s go together")
        if key is None:
            return None, None, None
        return (L.as_f32(key, f"key_{name}", (3, H, W), dev),
                [L.as_f32(s, f"src_{name}s[{i}]", (3, H, W), dev) for i, s in enumerate(views(srcs_, f"src_{name}s", V))],
                torch.empty((3, H, W), dtype=torch.float32, device=dev))

    k_img, s_img, rgb = attribute(key_image, src_images, "image")
    k_nrm, s_nrm, nrm = attribute(key_normal, src_normals, "normal")
    bits = torch.empty((H, W), dtype=torch.uint32, device=dev)
    fused = torch.empty((H, W), dtype=torch.float32, device=dev)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    count = torch.empty((H, W), dtype=torch.uint8, device=dev)
    call("mvd_geo_merge_f32", dev, d, srcs, mats, unc, V, H, W, float(max_reproj_error), float(max_rel_depth_diff), min_views,
         float(max_uncertainty) if unc is not None else 0.0, key_claimed, claims[1:], k_img, s_img, k_nrm, s_nrm, bits, fused, mask,
         count, rgb, nrm)
    return bits, fused, mask, count, rgb, nrm


@inference_only
def compact_points(mask, depth, backproject, image=None, count=None, out=None, normals=None):
    """The set pixels of mask (H,W) uint8 in row-major order as world points (include/mvd.h: mvd_compact_points_f32): xyz =
    depth * B (x,y,1) + c with backproject = (B (9), c (3)) on the device; image: planar (3,H,W), gathered into rgb.
    Returns (xyz (H*W,3), rgb (H*W,3) or None, count): the first count[0] rows are the points; count is a device int64 tensor of
    one element (the caller's own, where given), left on the device so that the caller decides when to read it.  out: the
    (xyz, rgb) of an earlier call on maps of this size, written again instead of two new buffers.
    normals: planar (3,H,W), gathered like the image (mvd_compact_points_attr_f32); the result is then (xyz, rgb, count, normals
    (H*W,3)), and `out` may carry that buffer as a third element."""
    m = L.as_dtype(torch.uint8, False, mask, "mask")
    if m.dim() != 2:
        raise ValueError(f"mask must be (H,W), got {tuple(m.shape)}")
    H, W = m.shape
    dev = m.device
    d = L.as_f32(depth, "depth", (H, W), dev)
    bp = L.as_f32(backproject, "backproject", device=dev)
    if bp.numel() != 12:
        raise ValueError(f"backproject must hold 12 floats, got {tuple(bp.shape)}")
    img = L.as_f32(image, "image", (3, H, W), dev) if image is not None else None
    if count is None:
        count = torch.empty(1, dtype=torch.int64, device=dev)
    elif count.dtype != torch.int64 or count.device != dev or count.numel() != 1:
        raise ValueError("count must be one int64 on the mask's device")
    nrm = L.as_f32(normals, "normals", (3, H, W), dev) if normals is not None else None
    if out is None:
        xyz = torch.empty((H * W, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((H * W, 3), dtype=torch.float32, device=dev) if img is not None else None
        nrm_out = torch.empty((H * W, 3), dtype=torch.float32, device=dev) if nrm is not None else None
    else:
        xyz, rgb, nrm_out = out if len(out) == 3 else (*out, None)
        for t, want in ((xyz, True), (rgb, img is not None), (nrm_out, nrm is not None)):
            if (t is not None) != want or (want and (t.dtype != torch.float32 or t.device != dev or t.shape != (H * W, 3)
                                                     or not t.is_contiguous())):
                raise ValueError(f"out must be (xyz, rgb[, normals]) contiguous float32 ({H * W},3) tensors on {dev}, rgb None without "
                                 "an image, normals there exactly when normals are gathered")
    nbytes = L.load().mvd_compact_points_workspace_bytes(H, W)
    ws = workspace(nbytes, dev)
    if nrm is None:
        call("mvd_compact_points_f32", dev, m, d, img, bp, H, W, xyz, rgb, count, ws, int(nbytes))
        return xyz, rgb, count
    call("mvd_compact_points_attr_f32", dev, m, d, img, nrm, bp, H, W, xyz, rgb, nrm_out, count, ws, int(nbytes))
    return xyz, rgb, count, nrm_out


def _tsdf_state(tsdf, weight, color, writable):
    """The state of a TSDF volume as the kernels take it: float32, contiguous, on one GPU; where it is written, as it is (never a
    converted or contiguous copy).  -> (tsdf, weight, color or None, (nx, ny, nz))."""
    convert = not writable
    f = L.as_dtype(torch.float32, convert, tsdf, "tsdf")
    if f.dim() != 3:
        raise ValueError(f"tsdf must be (nz,ny,nx), got {tuple(f.shape)}")
    if f.numel() == 0 or f.numel() >= 2 ** 31:
        raise ValueError(f"tsdf {tuple(f.shape)}: nx ny nz must be in 1 .. 2^31 - 1")
    w = L.as_dtype(torch.float32, convert, weight, "weight", tuple(f.shape), f.device)
    c = None if color is None else L.as_dtype(torch.float32, convert, color, "color", (3,) + tuple(f.shape), f.device)
    if writable:
        for name, t in (("tsdf", tsdf), ("weight", weight), ("color", color)):
            if t is not None and not t.is_contiguous():
                raise ValueError(f"{name}: must be contiguous (it is updated in place)")
    nz, ny, nx = f.shape
    return f, w, c, (nx, ny, nz)


@inference_only
def tsdf_integrate(tsdf, weight, color, depths, matrices, trunc, max_weight=None, weights=None, images=None):
    """Integrates V <= 32 depth maps of one size into a TSDF volume IN PLACE, in list order and in one launch (include/mvd.h:
    mvd_tsdf_integrate_f32; tsdf.integrate_numpy is the definition).  tsdf, weight (nz,ny,nx) and color (3,nz,ny,nx) or None:
    contiguous float32.  depths: V x (H,W); matrices (V,12): tsdf.compose_matrix's rows; weights: V x (H,W) per-pixel weights (any
    dtype, taken as float32) or None; images: V x (3,H,W), read only when the volume has colour.  max_weight None: no cap."""
    f, w, c, (nx, ny, nz) = _tsdf_state(tsdf, weight, color, writable=True)
    dev = f.device
    depths = views(depths, "depths")
    V = len(depths)
    d0 = L.as_f32(depths[0], "depths[0]", device=dev)
    if d0.dim() != 2 or d0.numel() == 0:
        raise ValueError(f"depths[0] must be (H,W) with H, W >= 1, got {tuple(d0.shape)}")
    H, W = d0.shape
    ds = [d0] + [L.as_f32(d, f"depths[{i + 1}]", (H, W), dev) for i, d in enumerate(depths[1:])]
    mats = L.as_f32(matrices, "matrices", (V, 12), dev)
    ws = None if weights is None else [L.as_f32(m, f"weights[{i}]", (H, W), dev) for i, m in enumerate(views(weights, "weights", V))]
    ims = None
    if images is not None and c is not None:
        ims = [L.as_f32(im, f"images[{i}]", (3, H, W), dev) for i, im in enumerate(views(images, "images", V))]
    if not float(trunc) > 0:
        raise ValueError(f"trunc must be positive, got {trunc}")
    if max_weight is not None and not float(max_weight) > 0:
        raise ValueError(f"max_weight must be positive, got {max_weight}")
    call("mvd_tsdf_integrate_f32", dev, f, w, c, nx, ny, nz, ds, ws, ims, mats, V, H, W, float(trunc),
         0.0 if max_weight is None else float(max_weight))


@inference_only
def tsdf_extract(tsdf, weight, color=None, origin=(0.0, 0.0, 0.0), voxel=1.0, min_weight=1.0):
    """The surface of a TSDF volume as a triangle mesh (include/mvd.h: mvd_tsdf_extract_f32; tsdf.extract_numpy is the definition).
    Returns (vertices (M,3) float32, triangles (T,3) int32, colors (M,3) float32 or None) at their exact sizes: the volume is
    classified and counted, M and T are read (the call's one synchronisation, 16 bytes), and the second call writes the mesh from
    the classification the workspace still holds."""
    f, w, c, (nx, ny, nz) = _tsdf_state(tsdf, weight, color, writable=False)
    dev = f.device
    o = [float(a) for a in origin]
    if len(o) != 3:
        raise ValueError(f"origin must hold 3 values, got {len(o)}")
    nbytes = L.load().mvd_tsdf_extract_workspace_bytes(nx, ny, nz)
    ws = workspace(nbytes, dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    head = (f, w, c, nx, ny, nz, o[0], o[1], o[2], float(voxel), float(min_weight))
    call("mvd_tsdf_extract_f32", dev, *head, 0, None, None, None, 0, 0, counts, ws, int(nbytes))
    M, T = (int(n) for n in counts.tolist())
    if M >= 2 ** 31 or T >= 2 ** 31:
        raise ValueError(f"the mesh has {M} vertices and {T} triangles: both must be below 2^31")
    vertices = torch.empty((M, 3), dtype=torch.float32, device=dev)
    triangles = torch.empty((T, 3), dtype=torch.int32, device=dev)
    colors = torch.empty((M, 3), dtype=torch.float32, device=dev) if c is not None else None
    if M:
        call("mvd_tsdf_extract_f32", dev, *head, 1, vertices, colors, triangles, M, T, counts, ws, int(nbytes))
    return vertices, triangles, colors


@inference_only
def mesh_render(vertices, triangles, matrices, size, colors=None, normals=False, bary=False, cull=None, near=0.0, max_small=None,
                load_first=False, check_indices=True, stages=0, workspace_=None, out=None):
    """Renders a triangle mesh into V <= 32 views of one size in one call (include/mvd.h: mvd_mesh_render_f32; render.render_numpy is
    the definition).  vertices (M,3) float32, triangles (T,3) int32, colors None or (M,3) float32, matrices (V,12):
    render.compose_projection's rows; size (H,W); cull None, "back" or "front".  -> dict: depth (V,H,W) float32 (0: empty), triangle
    (V,H,W) int32 (-1: empty), and bary / colors / normals (V,3,H,W) float32 or None.
    max_small: the largest pixel box one lane rasterises by itself (None: L.MESH_RENDER_MAX_SMALL); load_first: a plain load of the key
    before the atomic (measured slower).  Neither changes a bit of the result.  check_indices: one reduction and synchronisation that refuses a vertex index
    outside 0 .. M - 1 (the kernels skip such a triangle).  stages, workspace_, out: for measurements (tools/bench_render.py), the
    MVD_RENDER_KEEP_* / NO_RESOLVE bits with the workspace and the result of an earlier call on the same arguments."""
    from . import render as R
    v = _device_vertices(vertices, convert=True)
    dev, M = v.device, int(v.shape[0])
    t = _device_triangles(triangles, M, dev, convert=True, index_range=check_indices)
    T = int(t.shape[0])
    c = None if colors is None else L.as_f32(colors, "colors", device=dev)
    R.check_colors(c, M)
    mats = L.as_f32(matrices, "matrices", device=dev)
    if mats.dim() != 2 or mats.shape[1] != 12 or not 1 <= mats.shape[0] <= L.MVD_MAX_VIEWS:
        raise ValueError(f"matrices must be (V,12) with V in 1..{L.MVD_MAX_VIEWS}, got {tuple(mats.shape)}")
    V = int(mats.shape[0])
    _, H, W = R.check_views([None] * V, [None] * V, size)
    if V * T >= 2 ** 32:
        raise ValueError(f"V T = {V * T} must be below 2^32: render fewer views per call")
    code = R.check_cull(cull)
    max_small = L.MESH_RENDER_MAX_SMALL if max_small is None else int(max_small)
    if not 0 <= max_small < 2 ** 31:
        raise ValueError(f"max_small must be in 0 .. 2^31 - 1, got {max_small}")
    if out is None:
        maps = lambda on: torch.empty((V, 3, H, W), dtype=torch.float32, device=dev) if on else None
        out = {"depth": torch.empty((V, H, W), dtype=torch.float32, device=dev),
               "triangle": torch.empty((V, H, W), dtype=torch.int32, device=dev),
               "bary": maps(bary), "colors": maps(c is not None), "normals": maps(normals)}
    nbytes = L.load().mvd_mesh_render_workspace_bytes(M, T, V, H, W)
    ws = workspace(nbytes, dev) if workspace_ is None else workspace_
    if ws.numel() < nbytes:
        raise ValueError(f"workspace_ holds {ws.numel()} bytes, needed {nbytes}")
    flags = (L.RENDER_LOAD_FIRST if load_first else 0) | int(stages)
    call("mvd_mesh_render_f32", dev, v if M else None, M, t if T else None, T, c, mats, V, H, W, float(near), code, max_small, flags,
         out["depth"], out["triangle"], out["bary"], out["colors"], out["normals"], ws, int(nbytes))
    return out


def _device_vertices(vertices, device=None, convert=False):
    """A mesh's vertices (M,3) as the kernels take them: float32, contiguous, on a GPU; another dtype is converted or refused."""
    v = L.as_dtype(torch.float32, convert, vertices, "vertices", device=device)
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"vertices must be (M,3), got {tuple(v.shape)}")
    return v


def _device_triangles(triangles, M, device=None, convert=False, index_range=False):
    """A mesh's triangles (T,3) as the kernels take them: int32, contiguous, on a GPU, M and T below 2^31; another dtype is converted
    or refused.  index_range: mesh.check_triangles' reduction and read, which only mesh_render asks for."""
    t = L.as_dtype(torch.int32, convert, triangles, "triangles", device=device)
    check_triangles(t, M, dtypes=False, index_range=index_range)
    return t


@inference_only
def mesh_hook_round(triangles, M, label, referenced, changed, first=False, stages=0):
    """One round of the component labelling IN PLACE (include/mvd.h: mvd_mesh_hook_round): a hook launch over the triangles and a
    shortcut launch over the vertices.  triangles (T,3) int32, label (M) int32, referenced (M) uint8, changed: one int32 word on the
    device, zeroed by the call and 1 after it when a label changed.  first: starts a labelling (label[v] = v, referenced = 0).
    stages: for measurements (tools/bench_mesh_clean.py), L.MESH_ROUND_NO_HOOK or L.MESH_ROUND_NO_SHORTCUT: one launch of the two."""
    t = _device_triangles(triangles, M)
    dev = t.device
    M = int(M)
    lab = L.as_dtype(torch.int32, False, label, "label", (M,), dev)
    ref = L.as_dtype(torch.uint8, False, referenced, "referenced", (M,), dev)
    ch = L.as_dtype(torch.int32, False, changed, "changed", device=dev)
    if ch.numel() != 1 or not (label.is_contiguous() and referenced.is_contiguous()):
        raise ValueError("changed must hold one word; label and referenced must be contiguous (they are updated in place)")
    T = int(t.shape[0])
    call("mvd_mesh_hook_round", dev, t if T else None, T, M, (L.MESH_ROUND_FIRST if first else 0) | int(stages), lab if M else None,
         ref if M else None, ch)


@inference_only
def mesh_component_rank(label, referenced):
    """-> (vertex_component (M) int32: the component of every vertex, ids in ascending order of the components' lowest vertex, -1
    for an unreferenced vertex; num_components: one int64 left on the device) from a converged labelling (mvd_mesh_component_rank)."""
    lab = L.as_dtype(torch.int32, False, label, "label")
    dev, M = lab.device, int(lab.numel())
    ref = L.as_dtype(torch.uint8, False, referenced, "referenced", (M,), dev)
    vcomp = torch.empty(M, dtype=torch.int32, device=dev)
    num = torch.empty(1, dtype=torch.int64, device=dev)
    nbytes = L.load().mvd_mesh_component_rank_workspace_bytes(M)
    ws = workspace(nbytes, dev)
    call("mvd_mesh_component_rank", dev, lab if M else None, ref if M else None, M, vcomp if M else None, num, ws, int(nbytes))
    return vcomp, num


@inference_only
def mesh_component_table(vertex_component, triangles, C):
    """-> (triangle_component (T) int32: the component of each triangle's first vertex; num_vertices (C) int32)
    (mvd_mesh_component_table).  C: mesh_component_rank's count, read by the caller."""
    vc = L.as_dtype(torch.int32, False, vertex_component, "vertex_component")
    dev, M = vc.device, int(vc.numel())
    t = _device_triangles(triangles, M, dev)
    T, C = int(t.shape[0]), int(C)
    tcomp = torch.empty(T, dtype=torch.int32, device=dev)
    nv = torch.empty(C, dtype=torch.int32, device=dev)
    call("mvd_mesh_component_table", dev, vc if M else None, t if T else None, T, M, C, tcomp if T else None, nv if C else None)
    return tcomp, nv


@inference_only
def mesh_component_sums(vertices, triangles, sorted_component, perm, C):
    """-> (num_triangles (C) int32, area (C) float64): the fixed-order sums over the triangles sorted stably by component
    (mvd_mesh_component_sums_f64).  sorted_component (T) int32 and perm (T) int64: torch.sort(triangle_component, stable=True)."""
    v = L.as_f32(vertices, "vertices")
    dev, M = v.device, int(v.shape[0])
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"vertices must be (M,3), got {tuple(v.shape)}")
    t = _device_triangles(triangles, M, dev)
    T, C = int(t.shape[0]), int(C)
    key = L.as_dtype(torch.int32, False, sorted_component, "sorted_component", (T,), dev)
    pm = L.as_dtype(torch.int64, False, perm, "perm", (T,), dev)
    nt = torch.empty(C, dtype=torch.int32, device=dev)
    area = torch.empty(C, dtype=torch.float64, device=dev)
    if C:
        nbytes = L.load().mvd_mesh_component_sums_workspace_bytes(T, C)
        ws = workspace(nbytes, dev)
        call("mvd_mesh_component_sums_f64", dev, v, M, t, T, key, pm, C, nt, area, ws, int(nbytes))
    return nt, area


@inference_only
def mesh_filter(triangles, M, triangle_component=None, keep_component=None, remove_unreferenced=True):
    """The kept triangles and vertices of a mesh (include/mvd.h: mvd_mesh_filter; mesh_clean.clean_numpy is the definition).
    keep_component (C) uint8 / bool with triangle_component (T) int32, or None for every triangle.  Returns (out_triangles (T',3)
    int32 re-indexed, kept_triangles (T') int32, vertex_remap (M) int32, M') at their exact sizes: the call counts, M' and T' are read
    (the call's one synchronisation, 16 bytes), and the second call writes from the counts the workspace still holds."""
    t = _device_triangles(triangles, M)
    dev, T, M = t.device, int(t.shape[0]), int(M)
    keep, tcomp, C = None, None, 0
    if keep_component is not None:
        keep = L.as_dtype(torch.uint8, True, keep_component, "keep_component", device=dev)
        C = int(keep.numel())
        if triangle_component is None:
            raise ValueError("keep_component needs triangle_component")
        tcomp = L.as_dtype(torch.int32, False, triangle_component, "triangle_component", (T,), dev)
        if C == 0:  # told by a pointer: one byte nobody reads
            keep = torch.zeros(1, dtype=torch.uint8, device=dev)
    nbytes = L.load().mvd_mesh_filter_workspace_bytes(M, T)
    ws = workspace(nbytes, dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    head = (t if T else None, T, M, tcomp if T else None, keep, C, int(bool(remove_unreferenced)))
    call("mvd_mesh_filter", dev, *head, 0, None, None, None, 0, counts, ws, int(nbytes))
    Mk, Tk = (int(n) for n in counts.tolist())
    out = torch.empty((Tk, 3), dtype=torch.int32, device=dev)
    kept = torch.empty(Tk, dtype=torch.int32, device=dev)
    remap = torch.empty(M, dtype=torch.int32, device=dev)
    # the pointers tell the second use: one word each where the arrays are empty
    spare = torch.empty(4, dtype=torch.int32, device=dev)
    call("mvd_mesh_filter", dev, *head, 1, out if Tk else spare, kept if Tk else spare, remap if M else spare, Tk, counts, ws, int(nbytes))
    return out, kept, remap, Mk


@inference_only
def mesh_gather_rows(src, vertex_remap, rows):
    """-> (rows,k) float32: dst[vertex_remap[v]] = src[v] for every kept vertex, bit for bit (mvd_mesh_gather_rows_f32)."""
    remap = L.as_dtype(torch.int32, False, vertex_remap, "vertex_remap")
    dev, M = remap.device, int(remap.numel())
    s = L.as_dtype(torch.float32, False, src, "src", device=dev)
    if s.dim() != 2 or s.shape[0] != M or not 1 <= s.shape[1] <= 65536:
        raise ValueError(f"src must be ({M},k) with k in 1 .. 65536, got {tuple(s.shape)}")
    rows, k = int(rows), int(s.shape[1])
    if not 0 <= rows <= M:
        raise ValueError(f"{rows} rows out of {M}")
    if M * k >= 2 ** 31:
        raise ValueError(f"src holds {M * k} values: M k must be below 2^31")
    dst = torch.empty((rows, k), dtype=torch.float32, device=dev)
    if rows:
        call("mvd_mesh_gather_rows_f32", dev, s, remap, M, k, rows, dst)
    return dst


@inference_only
def mesh_vertex_normals(vertices, triangles, sorted_vertex, perm):
    """-> normals (M,3) float32, area-weighted (include/mvd.h: mvd_mesh_vertex_normals_f32; mesh_clean.vertex_normals_numpy is the
    definition).  sorted_vertex (3T) int32 and perm (3T) int64: torch.sort(triangles.reshape(-1), stable=True)."""
    v = L.as_f32(vertices, "vertices")
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"vertices must be (M,3), got {tuple(v.shape)}")
    dev, M = v.device, int(v.shape[0])
    t = _device_triangles(triangles, M, dev)
    T = int(t.shape[0])
    if 3 * T >= 2 ** 31:
        raise ValueError(f"{T} triangles: 3 T must be below 2^31")
    key = L.as_dtype(torch.int32, False, sorted_vertex, "sorted_vertex", (3 * T,), dev)
    pm = L.as_dtype(torch.int64, False, perm, "perm", (3 * T,), dev)
    normals = torch.empty((M, 3), dtype=torch.float32, device=dev)
    if M:
        call("mvd_mesh_vertex_normals_f32", dev, v, M, t if T else None, T, key if T else None, pm if T else None, normals)
    return normals


class MeshClusters:
    """The clusters of a mesh's vertices (mesh_cluster_ids): vertex_cluster (M) int32, cluster_start (K+1) int32 into perm,
    cluster_key (K) int64, perm (M) int64 (the vertices sorted stably by key), origin (3 floats), cell (the float32 edge as a float)."""
    __slots__ = ("vertex_cluster", "cluster_start", "cluster_key", "perm", "origin", "cell")

    def __init__(self, vertex_cluster, cluster_start, cluster_key, perm, origin, cell):
        self.vertex_cluster, self.cluster_start, self.cluster_key, self.perm = vertex_cluster, cluster_start, cluster_key, perm
        self.origin, self.cell = origin, cell

    @property
    def num_clusters(self):
        return int(self.cluster_key.shape[0])

    @property
    def counts(self):
        return self.cluster_start[1:] - self.cluster_start[:-1]


@inference_only
def mesh_cluster_ids(vertices, cell, origin=None):
    """The vertices of a mesh sorted into the cells of edge `cell` (taken as float32) and numbered (include/mvd.h:
    mvd_mesh_cluster_ids; mesh_simplify.cluster_numpy is the definition) -> MeshClusters.  origin defaults to the per-axis minimum
    over the finite vertices.  Host reads: the extent (6 floats) and K."""
    v = _device_vertices(vertices)
    dev, M = v.device, int(v.shape[0])
    cell = float(torch.tensor(float(cell), dtype=torch.float32))
    if not 0.0 < cell < float("inf"):
        raise ValueError(f"cell must be finite and > 0, got {cell}")
    inv = 1.0 / cell
    extent = cloud_extent(v)
    o = _cloud_origin(origin) if origin is not None else ([0.0, 0.0, 0.0] if extent is None else extent[0].tolist())
    _check_cloud_indices(extent, o, inv, "voxel_downsample", cell)
    keys, perm = cloud_sorted(v, o, inv)
    vc = torch.empty(M, dtype=torch.int32, device=dev)
    start = torch.empty(M + 1, dtype=torch.int32, device=dev)
    ckey = torch.empty(M, dtype=torch.int64, device=dev)
    num = torch.empty(1, dtype=torch.int64, device=dev)
    nbytes = L.load().mvd_mesh_cluster_ids_workspace_bytes(M)
    ws = workspace(nbytes, dev)
    call("mvd_mesh_cluster_ids", dev, keys if M else None, perm if M else None, M, vc if M else None, start, ckey if M else None, num, ws,
         int(nbytes))
    K = int(num.item())
    return MeshClusters(vc, start[:K + 1].clone(), ckey[:K].clone(), perm, o, cell)


@inference_only
def mesh_cluster_means(rows, clusters):
    """-> (K,k) float64: every cluster's mean of a per-vertex (M,k) float32 array, summed in ascending vertex index in the fixed
    segment order (mvd_mesh_cluster_means_f64)."""
    dev, M, K = clusters.perm.device, int(clusters.perm.numel()), clusters.num_clusters
    r = L.as_dtype(torch.float32, False, rows, "rows", device=dev)
    if r.dim() != 2 or r.shape[0] != M or not 1 <= r.shape[1] <= 65536:
        raise ValueError(f"rows must be ({M},k) with k in 1 .. 65536, got {tuple(r.shape)}")
    k = int(r.shape[1])
    if M * k >= 2 ** 31:
        raise ValueError(f"rows holds {M * k} values: M k must be below 2^31")
    means = torch.empty((K, k), dtype=torch.float64, device=dev)
    if K:
        call("mvd_mesh_cluster_means_f64", dev, r, clusters.perm, clusters.cluster_start, K, M, k, means)
    return means


@inference_only
def mesh_cluster_triples(triangles, clusters):
    """-> (triples (T,3) int32: the rotated cluster triple or (-1,-1,-1); alive (T) uint8; corner_key (T,3) int32: each corner's
    cluster, K for a triangle with an invalid vertex) (mvd_mesh_cluster_triples)."""
    vc = clusters.vertex_cluster
    dev, M, K = vc.device, int(vc.numel()), clusters.num_clusters
    t = _device_triangles(triangles, M, dev)
    T = int(t.shape[0])
    if 3 * T >= 2 ** 31:
        raise ValueError(f"{T} triangles: 3 T must be below 2^31")
    triples = torch.empty((T, 3), dtype=torch.int32, device=dev)
    alive = torch.empty(T, dtype=torch.uint8, device=dev)
    corner = torch.empty((T, 3), dtype=torch.int32, device=dev)
    if T:
        call("mvd_mesh_cluster_triples", dev, t, T, M, vc, K, triples, alive, corner)
    return triples, alive, corner


@inference_only
def mesh_cluster_quadrics(vertices, triangles, sorted_cluster, perm, clusters):
    """-> (K,10) float64: every cluster's quadric sums over its corners in ascending (triangle, corner) in the fixed segment order
    (mvd_mesh_cluster_quadrics_f64).  sorted_cluster (3T) int32 and perm (3T) int64: torch.sort(corner_key.reshape(-1), stable=True)."""
    dev, K = clusters.vertex_cluster.device, clusters.num_clusters
    v = _device_vertices(vertices, dev)
    M = int(v.shape[0])
    t = _device_triangles(triangles, M, dev)
    T = int(t.shape[0])
    if 3 * T >= 2 ** 31:
        raise ValueError(f"{T} triangles: 3 T must be below 2^31")
    key = L.as_dtype(torch.int32, False, sorted_cluster, "sorted_cluster", (3 * T,), dev)
    pm = L.as_dtype(torch.int64, False, perm, "perm", (3 * T,), dev)
    quadrics = torch.empty((K, 10), dtype=torch.float64, device=dev)
    if K:
        nbytes = L.load().mvd_mesh_cluster_quadrics_workspace_bytes(K)
        ws = workspace(nbytes, dev)
        o = clusters.origin
        call("mvd_mesh_cluster_quadrics_f64", dev, v, M, t if T else None, T, key if T else None, pm if T else None, clusters.cluster_key, K,
             o[0], o[1], o[2], clusters.cell, quadrics, ws, int(nbytes))
    return quadrics


@inference_only
def mesh_cluster_place(vertices, clusters, means, quadrics=None, regularisation=1e-3):
    """-> (vertices (K,3) float32, placed (K) uint8): per cluster the quadric's regularised minimum (1), the mean (0: quadrics=None,
    or the minimum is refused) or its single vertex (2) (mvd_mesh_cluster_place_f32; mesh_simplify.place_numpy is the definition)."""
    dev, K = clusters.vertex_cluster.device, clusters.num_clusters
    v = _device_vertices(vertices, dev)
    M = int(v.shape[0])
    mean = L.as_dtype(torch.float64, False, means, "means", (K, 3), dev)
    q = None if quadrics is None else L.as_dtype(torch.float64, False, quadrics, "quadrics", (K, 10), dev)
    reg = float(regularisation)
    if not 0.0 < reg < float("inf"):
        raise ValueError(f"regularisation must be finite and > 0, got {regularisation}")
    out = torch.empty((K, 3), dtype=torch.float32, device=dev)
    placed = torch.empty(K, dtype=torch.uint8, device=dev)
    if K:
        o = clusters.origin
        call("mvd_mesh_cluster_place_f32", dev, q, mean, clusters.cluster_start, clusters.cluster_key, clusters.perm, v, K, M, o[0], o[1], o[2],
             clusters.cell, reg, out, placed)
    return out, placed


@inference_only
def mesh_cluster_mark_first(triples, alive, perm):
    """-> keep (T) uint8: the alive triangles that come first among those of their triple (mvd_mesh_cluster_mark_first).  perm (T)
    int64 orders the alive triples lexicographically, equal ones by triangle index."""
    tr = L.as_dtype(torch.int32, False, triples, "triples")
    dev, T = tr.device, int(tr.shape[0])
    if tr.dim() != 2 or tr.shape[1] != 3:
        raise ValueError(f"triples must be (T,3), got {tuple(tr.shape)}")
    al = L.as_dtype(torch.uint8, False, alive, "alive", (T,), dev)
    pm = L.as_dtype(torch.int64, False, perm, "perm", (T,), dev)
    keep = torch.empty(T, dtype=torch.uint8, device=dev)
    if T:
        call("mvd_mesh_cluster_mark_first", dev, tr, al, pm, T, keep)
    return keep


CLOUD_INDEX_LIMIT = (1 << 21) - 1 # a cell or voxel index is in [0, 2^21 - 1): the all-ones key is the invalid points' own
CLOUD_CELL_MARGIN = 1.0 + 2.0 ** -10  # cell edge = max_dist * margin (csrc/cloud_eval.hip: why 27 cells are enough)


def cloud_points(points, name, device=None):
    p = L.as_f32(points, name, device=device)
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"{name} must be (n,3), got {tuple(p.shape)}")
    if p.shape[0] >= 2 ** 31:
        raise ValueError(f"{name}: {p.shape[0]} points, supported below 2^31")
    return p


def cloud_extent(p):
    """Per-axis min and max over the valid points of p (n,3) as float64 numpy, or None when there is none: one read of 6 floats."""
    if p.shape[0] == 0:
        return None
    ok = torch.isfinite(p).all(dim=1, keepdim=True)
    inf = torch.tensor(float("inf"), device=p.device)
    both = torch.stack([torch.where(ok, p, inf).amin(dim=0), torch.where(ok, p, -inf).amax(dim=0)]).double().cpu().numpy()
    return None if both[0, 0] == float("inf") else both


def _cloud_origin(origin, name="origin"):
    o = [float(v) for v in (origin.tolist() if hasattr(origin, "tolist") else origin)]
    if len(o) != 3 or not all(abs(v) < float("inf") for v in o):
        raise ValueError(f"{name} must be 3 finite numbers, got {o}")
    return o


def _check_cloud_indices(extent, origin, inv, what, edge):
    """The host's check that every index floor((x - o) * inv) of a cloud fits the key: a ValueError that names extent and edge."""
    if extent is None:
        return
    lo = [(extent[0, a] - origin[a]) * inv for a in range(3)]
    hi = [(extent[1, a] - origin[a]) * inv for a in range(3)]
    if min(lo) < 0 or max(hi) >= CLOUD_INDEX_LIMIT:
        raise ValueError(f"{what}: the points span {extent[0].tolist()} .. {extent[1].tolist()} from origin {list(origin)}, which at an edge of "
                         f"{edge:g} gives indices {min(lo):.0f} .. {max(hi):.0f}; each must be in [0, {CLOUD_INDEX_LIMIT})")


def cloud_sorted(p, origin, inv):
    """Keys of p's cells, sorted stably, and the permutation -> (keys, perm).  The sort is torch's: plumbing between two kernels."""
    n = p.shape[0]
    keys = torch.empty(n, dtype=torch.int64, device=p.device)
    call("mvd_cloud_cell_keys_f32", p.device, p, n, origin[0], origin[1], origin[2], inv, keys)
    return torch.sort(keys, stable=True)


class CloudGrid:
    """A cloud sorted into the cells of a uniform grid (cloud_grid): points (n,3) as given, keys (n) int64 ascending, records (n,4)
    = x, y, z and the original index's bits in key order, origin (3 floats), cell and inv = 1.0 / cell."""
    __slots__ = ("points", "keys", "records", "origin", "cell", "inv")

    def __init__(self, points, keys, records, origin, cell):
        self.points, self.keys, self.records, self.origin, self.cell, self.inv = points, keys, records, origin, cell, 1.0 / cell


@inference_only
def cloud_grid(points, origin, cell, check=True):
    """points (n,3) sorted into the cells of edge `cell` from `origin` (include/mvd.h: mvd_cloud_cell_keys_f32,
    mvd_cloud_grid_build_f32) -> CloudGrid.  check: every valid point's cell indices must be in [0, 2^21 - 1), else ValueError
    (a target grid needs it; check=False clamps instead, for a cloud that is only queried)."""
    p = cloud_points(points, "points")
    origin, cell = _cloud_origin(origin), float(cell)
    if not 0.0 < cell < float("inf"):
        raise ValueError(f"cell must be finite and > 0, got {cell}")
    inv = 1.0 / cell
    if check:
        _check_cloud_indices(cloud_extent(p), origin, inv, "cloud_grid", cell)
    keys, perm = cloud_sorted(p, origin, inv)
    records = torch.empty((p.shape[0], 4), dtype=torch.float32, device=p.device)
    call("mvd_cloud_grid_build_f32", p.device, p, perm, p.shape[0], records)
    return CloudGrid(p, keys, records, origin, cell)


def _cloud_nearest(query_records, grid, max_dist):
    """mvd_cloud_nearest_f32 behind cloud_nearest and cloud_nearest_records.  query_records(device) -> the (n,4) records of the
    queries, asked for once the grid and max_dist have passed their checks -> (dist (n) float32, index (n) int32)."""
    if not isinstance(grid, CloudGrid):
        raise ValueError(f"grid: expected a CloudGrid (ops.cloud_grid), got {type(grid).__name__}")
    dev = grid.points.device
    max_dist = float(torch.tensor(max_dist, dtype=torch.float32))  # the float32 the kernel compares with
    if not 0.0 < max_dist < float("inf"):
        raise ValueError(f"max_dist must be finite and > 0, got {max_dist}")
    if grid.cell < max_dist * CLOUD_CELL_MARGIN * (1 - 1e-12):
        raise ValueError(f"the grid's cell {grid.cell:g} is below max_dist * (1 + 2^-10) = {max_dist * CLOUD_CELL_MARGIN:g}")
    rec = query_records(dev)
    n, m = rec.shape[0], grid.points.shape[0]
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    index = torch.empty(n, dtype=torch.int32, device=dev)
    call("mvd_cloud_nearest_f32", dev, rec, n, grid.records, grid.keys, m, grid.origin[0], grid.origin[1], grid.origin[2], grid.inv,
         max_dist, dist, index)
    return dist, index


def _result_block(result, words, dev, owner):
    """The device block a sum kernel fills: the caller's `result`, checked, or a new one of `words` int64."""
    if result is None:
        return torch.empty(words, dtype=torch.int64, device=dev)
    if result.dtype != torch.int64 or result.device != dev or result.numel() != words or not result.is_contiguous():
        raise ValueError(f"result must be {words} contiguous int64 on {owner} device")
    return result


@inference_only
def cloud_nearest(query, grid, max_dist):
    """The truncated nearest neighbour of every query in the grid's cloud (include/mvd.h: mvd_cloud_nearest_f32).  query: (n,3)
    points, sorted here by the grid's cells, or a CloudGrid of the same origin and cell (PointCloudEvaluation sorts each cloud once
    for both directions).  grid.cell must be at least max_dist * (1 + 2^-10).
    Returns (dist (n) float32, index (n) int32) in the query's original order; index -1 = nothing nearer than max_dist."""
    def records(dev):
        if isinstance(query, CloudGrid):
            if query.origin != grid.origin or query.cell != grid.cell or query.points.device != dev:
                raise ValueError("query and target grids differ in origin, cell or device")
            return query.records
        return cloud_grid(cloud_points(query, "query", dev), grid.origin, grid.cell, check=False).records

    return _cloud_nearest(records, grid, max_dist)


@inference_only
def cloud_scores(dist, index, thresholds, points=None, result=None):
    """One direction's sums over the valid queries (include/mvd.h: mvd_cloud_scores_f32).  dist (n) float32 and index (n) int32 from
    cloud_nearest; thresholds: T <= 8 numbers or a device tensor; points: the queries (n,3), so that the invalid ones among the
    truncated are left out (None: every query counts).  Returns a device int64 tensor of 10 words, left on the device: the bits of
    the float64 sum of dist, the count of valid queries, and eight counts of dist < thresholds[t] (read it with cloud_scores_read)."""
    d = L.as_dtype(torch.float32, False, dist, "dist")
    if d.dim() != 1:
        raise ValueError(f"dist must be (n,), got {tuple(d.shape)}")
    n, dev = d.shape[0], d.device
    idx = L.as_dtype(torch.int32, False, index, "index", (n,), dev)
    th = thresholds if isinstance(thresholds, torch.Tensor) else torch.tensor([float(t) for t in thresholds], dtype=torch.float32)
    if th.dim() != 1 or not 1 <= th.shape[0] <= L.MVD_CLOUD_MAX_THRESHOLDS:
        raise ValueError(f"{th.numel()} thresholds, supported 1..{L.MVD_CLOUD_MAX_THRESHOLDS}")
    th = L.as_f32(th.to(dev), "thresholds")
    pts = cloud_points(points, "points", dev) if points is not None else None
    if pts is not None and pts.shape[0] != n:
        raise ValueError(f"{pts.shape[0]} points for {n} distances")
    result = _result_block(result, 10, dev, "dist's")
    nbytes = L.load().mvd_cloud_scores_workspace_bytes(n)
    ws = workspace(nbytes, dev)
    call("mvd_cloud_scores_f32", dev, d, idx, pts, n, th, th.shape[0], result, ws, int(nbytes))
    return result


def cloud_scores_read(result, T):
    """cloud_scores' block on the host -> (sum float, valid int, counts (T,) int64 numpy): the one read of a direction."""
    r = result.cpu()
    return float(r[:1].view(torch.float64)[0]), int(r[1]), r[2:2 + T].numpy().copy()


CLOUD_PAIR_SUMS_PER_WG = L.MVD_CLOUD_PAIR_SUMS_PER_WORKGROUP  # the points one workgroup of cloud_pair_sums adds
CLOUD_PAIR_SUMS_WORDS = 32  # cloud_pair_sums' block: 256 bytes


def _transform12(transform):
    """A (4,4) or (3,4) transform [M | t] (cloud_register.py) -> the 12 finite doubles the C entries take, as a ctypes array."""
    from .cloud_register import affine_parts
    M, t = affine_parts(transform)
    return (ctypes.c_double * 12)(*[float(v) for a in range(3) for v in (M[a, 0], M[a, 1], M[a, 2], t[a])])


@inference_only
def cloud_transform(points, transform, normals=None):
    """points (n,3) through x -> M x + t in float64, rounded once (include/mvd.h: mvd_cloud_transform_f32; bit for bit
    cloud_register.transform_numpy) -> (n,3) float32, or (points, normals) with the normals (n,3) through M and re-normalised."""
    p = cloud_points(points, "points")
    n, dev = p.shape[0], p.device
    T = _transform12(transform)
    nrm = L.as_f32(normals, "normals", (n, 3), dev) if normals is not None else None
    out = torch.empty_like(p)
    out_n = torch.empty_like(p) if nrm is not None else None
    call("mvd_cloud_transform_f32", dev, p, nrm, n, T, out, out_n)
    return out if nrm is None else (out, out_n)


@inference_only
def cloud_transform_records(points, perm, transform):
    """cloud_grid's records of the MOVED points (include/mvd.h: mvd_cloud_transform_records_f32): sorted position i holds
    T(points[perm[i]]) and perm[i].  perm (n) int64: the permutation of a stable sort of the cell keys -> records (n,4) float32."""
    p = cloud_points(points, "points")
    n, dev = p.shape[0], p.device
    perm = L.as_dtype(torch.int64, False, perm, "perm", (n,), dev)
    records = torch.empty((n, 4), dtype=torch.float32, device=dev)
    call("mvd_cloud_transform_records_f32", dev, p, perm, n, _transform12(transform), records)
    return records


@inference_only
def cloud_nearest_records(records, grid, max_dist):
    """cloud_nearest for query records (n,4) that are already there (cloud_transform_records): -> (dist (n) float32, index (n) int32)
    in the order of the records' original indices."""
    def checked(dev):
        rec = L.as_dtype(torch.float32, False, records, "records", device=dev)
        if rec.dim() != 2 or rec.shape[1] != 4:
            raise ValueError(f"records must be (n,4), got {tuple(rec.shape)}")
        return rec

    return _cloud_nearest(checked, grid, max_dist)


@inference_only
def cloud_pair_sums(source, transform, index, target, pivot, target_normals=None, result=None):
    """The sums of one ICP iteration (include/mvd.h: mvd_cloud_pair_sums_f32; cloud_register.pair_sums_numpy).  source (n,3), index
    (n) int32 from cloud_nearest of the moved source, target (m,3), pivot: 3 numbers, target_normals (m,3): plane mode.  Returns a
    device int64 tensor of 32 words, left on the device: the count of pairs, then the bits of the float64 sums (read it with
    cloud_pair_sums_read)."""
    s = cloud_points(source, "source")
    n, dev = s.shape[0], s.device
    idx = L.as_dtype(torch.int32, False, index, "index", (n,), dev)
    p = cloud_points(target, "target", dev)
    m = p.shape[0]
    nrm = L.as_f32(target_normals, "target_normals", (m, 3), dev) if target_normals is not None else None
    if nrm is not None and m == 0:
        nrm = torch.zeros((1, 3), dtype=torch.float32, device=dev)  # plane mode is told by a pointer: one row nobody reads
    c = _cloud_origin(pivot, "pivot")
    result = _result_block(result, CLOUD_PAIR_SUMS_WORDS, dev, "the source's")
    nbytes = L.load().mvd_cloud_pair_sums_workspace_bytes(n)
    ws = workspace(nbytes, dev)
    call("mvd_cloud_pair_sums_f32", dev, s, n, _transform12(transform), idx, p if m else None, nrm, m, c[0], c[1], c[2], result, ws,
         int(nbytes))
    return result


def cloud_pair_sums_read(result, plane):
    """cloud_pair_sums' block on the host -> (N int, sums (18,) or (28,) float64 numpy): the one read of an iteration."""
    r = result.cpu()
    k = 28 if plane else 18
    return int(r[0]), r[1:1 + k].view(torch.float64).numpy().copy()


@inference_only
def voxel_downsample(points, voxel, colors=None, origin=None):
    """One point per occupied voxel of edge `voxel` (include/mvd.h: mvd_voxel_reduce_f32): the float64 mean of the voxel's valid
    points (and colours), in ascending order of the key floor((x - o) / voxel) per axis; origin defaults to the per-axis minimum
    over the valid points.  Returns (xyz (k,3) float32, rgb (k,3) or None, counts (k,) int32)."""
    p = cloud_points(points, "points")
    n, dev = p.shape[0], p.device
    voxel = float(torch.tensor(float(voxel), dtype=torch.float32))  # the definition takes the voxel as float32: inv = 1 / float64(float32)
    if not 0.0 < voxel < float("inf"):
        raise ValueError(f"voxel must be finite and > 0, got {voxel}")
    col = None
    if colors is not None:
        col = L.as_f32(colors, "colors", (n, 3), dev)
    inv = 1.0 / voxel
    extent = cloud_extent(p)
    o = _cloud_origin(origin) if origin is not None else ([0.0, 0.0, 0.0] if extent is None else extent[0].tolist())
    _check_cloud_indices(extent, o, inv, "voxel_downsample", voxel)
    keys, perm = cloud_sorted(p, o, inv)
    xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev) if col is not None else None
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    num = torch.empty(1, dtype=torch.int64, device=dev)
    nbytes = L.load().mvd_voxel_reduce_workspace_bytes(n)
    ws = workspace(nbytes, dev)
    call("mvd_voxel_reduce_f32", dev, keys, perm, p, col, n, xyz, rgb, counts, num, ws, int(nbytes))
    k = int(num.item())
    return xyz[:k].clone(), None if rgb is None else rgb[:k].clone(), counts[:k].clone()


CLOUD_KNN_MAX = L.CLOUD_KNN_MAX  # the largest k of cloud_knn


def _neighbour_query(query, grid, radius, name):
    """The shared front of cloud_radius_moments and cloud_knn -> (query records, exclude_self, radius as the float32 the kernel
    squares).  query: None or the grid itself (every point of the grid's cloud asks, and is not its own neighbour), another
    CloudGrid of the same origin and cell, or (n,3) points."""
    if not isinstance(grid, CloudGrid):
        raise ValueError(f"grid: expected a CloudGrid (ops.cloud_grid), got {type(grid).__name__}")
    dev = grid.points.device
    radius = float(torch.tensor(float(radius), dtype=torch.float32))
    if not 0.0 < radius < float("inf"):
        raise ValueError(f"{name} must be finite and > 0, got {radius}")
    if grid.cell < radius * CLOUD_CELL_MARGIN * (1 - 1e-12):
        raise ValueError(f"the grid's cell {grid.cell:g} is below {name} * (1 + 2^-10) = {radius * CLOUD_CELL_MARGIN:g}")
    if query is None or query is grid:
        return grid.records, 1, radius
    if isinstance(query, CloudGrid):
        if query.origin != grid.origin or query.cell != grid.cell or query.points.device != dev:
            raise ValueError("query and target grids differ in origin, cell or device")
        return query.records, 0, radius
    return cloud_grid(cloud_points(query, "query", dev), grid.origin, grid.cell, check=False).records, 0, radius


@inference_only
def cloud_radius_moments(query, grid, radius):
    """Per query the targets of the grid's cloud with d2 < radius^2 (include/mvd.h: mvd_cloud_radius_moments_f32) -> (count (n) int32,
    sum_dist (n) float64, moments (n,9) float64) in the query's original order.  query None or the grid itself: the cloud against
    itself, a point not its own neighbour."""
    rec, self_query, radius = _neighbour_query(query, grid, radius, "radius")
    dev, n, m = grid.points.device, rec.shape[0], grid.points.shape[0]
    count = torch.empty(n, dtype=torch.int32, device=dev)
    sum_dist = torch.empty(n, dtype=torch.float64, device=dev)
    moments = torch.empty((n, 9), dtype=torch.float64, device=dev)
    call("mvd_cloud_radius_moments_f32", dev, rec, n, grid.records, grid.keys, m, grid.origin[0], grid.origin[1], grid.origin[2], grid.inv,
         radius, self_query, count, sum_dist, moments)
    return count, sum_dist, moments


@inference_only
def cloud_knn(query, grid, k, max_dist):
    """Per query the up-to-k nearest targets of the grid's cloud within max_dist (include/mvd.h: mvd_cloud_knn_f32) -> (index (n,k)
    int32, dist (n,k) float32, count (n) int32) in the query's original order.  query None or the grid itself: the cloud against
    itself, a point not its own neighbour."""
    k = int(k)
    if not 1 <= k <= CLOUD_KNN_MAX:
        raise ValueError(f"k = {k}, supported 1..{CLOUD_KNN_MAX}")
    rec, self_query, max_dist = _neighbour_query(query, grid, max_dist, "max_dist")
    dev, n, m = grid.points.device, rec.shape[0], grid.points.shape[0]
    if n * k >= 2 ** 31:
        raise ValueError(f"{n} queries of {k} neighbours: n k must be below 2^31")
    index = torch.empty((n, k), dtype=torch.int32, device=dev)
    dist = torch.empty((n, k), dtype=torch.float32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    call("mvd_cloud_knn_f32", dev, rec, n, grid.records, grid.keys, m, grid.origin[0], grid.origin[1], grid.origin[2], grid.inv, max_dist, k,
         self_query, index, dist, count)
    return index, dist, count


@inference_only
def cloud_list_moments(points, targets, index, dist):
    """cloud_radius_moments' outputs over the lists of cloud_knn (include/mvd.h: mvd_cloud_list_moments_f32): points (n,3), targets
    (m,3), index and dist (n,k) -> (count (n) int32, sum_dist (n) float64, moments (n,9) float64)."""
    idx = L.as_dtype(torch.int32, False, index, "index")
    if idx.dim() != 2 or not 1 <= idx.shape[1] <= CLOUD_KNN_MAX:
        raise ValueError(f"index must be (n,k) with k in 1..{CLOUD_KNN_MAX}, got {tuple(idx.shape)}")
    dev, (n, k) = idx.device, idx.shape
    d = L.as_dtype(torch.float32, False, dist, "dist", (n, k), dev)
    p = L.as_dtype(torch.float32, False, cloud_points(points, "points", dev), "points", (n, 3))
    t = cloud_points(targets, "targets", dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    sum_dist = torch.empty(n, dtype=torch.float64, device=dev)
    moments = torch.empty((n, 9), dtype=torch.float64, device=dev)
    call("mvd_cloud_list_moments_f32", dev, p, n, t if t.shape[0] else None, t.shape[0], idx, d, k, count, sum_dist, moments)
    return count, sum_dist, moments


@inference_only
def cloud_normals(points, count, moments, min_neighbours=5, toward=None, like=None):
    """Normals and surface variation from the moments (include/mvd.h: mvd_cloud_normals_f64) -> (normals (n,3) float32, curvature (n)
    float32).  toward: a viewpoint of 3 numbers or (n,3) per-point viewpoints on the device; like: (n,3) reference normals; at most
    one of them."""
    p = cloud_points(points, "points")
    n, dev = p.shape[0], p.device
    cnt = L.as_dtype(torch.int32, False, count, "count", (n,), dev)
    mom = L.as_dtype(torch.float64, False, moments, "moments", (n, 9), dev)
    min_neighbours = int(min_neighbours)
    if min_neighbours < 2:
        raise ValueError(f"min_neighbours = {min_neighbours}, at least 2")
    if toward is not None and like is not None:
        raise ValueError("toward and like: at most one of them")
    orient, w, per_point = 0, [0.0, 0.0, 0.0], None
    if like is not None:
        orient, per_point = 3, L.as_f32(like, "like", (n, 3), dev)
    elif isinstance(toward, torch.Tensor) and toward.dim() == 2:
        orient, per_point = 2, L.as_f32(toward, "toward", (n, 3), dev)
    elif toward is not None:
        orient, w = 1, _cloud_origin(toward, "toward")
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    curvature = torch.empty(n, dtype=torch.float32, device=dev)
    call("mvd_cloud_normals_f64", dev, p, n, cnt, mom, min_neighbours, orient, w[0], w[1], w[2], per_point, normals, curvature)
    return normals, curvature


@inference_only
def cloud_keep_density(points, count, min_neighbours):
    """keep (n) uint8: the point is valid and has at least min_neighbours neighbours (include/mvd.h: mvd_cloud_keep_density)."""
    p = cloud_points(points, "points")
    n, dev = p.shape[0], p.device
    cnt = L.as_dtype(torch.int32, False, count, "count", (n,), dev)
    min_neighbours = int(min_neighbours)
    if min_neighbours < 0:
        raise ValueError(f"min_neighbours = {min_neighbours}, at least 0")
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    call("mvd_cloud_keep_density", dev, p, cnt, n, min_neighbours, keep)
    return keep


@inference_only
def cloud_knn_mean_sums(dist, count, result=None):
    """The statistical rule's first half (include/mvd.h: mvd_cloud_knn_mean_sums_f32): dist (n,k), count (n) of cloud_knn -> (mean (n)
    float64, NaN without a full list; a device int64 tensor of 4 words: the bits of the float64 sum of the means and of their
    squares, and their number; read it with cloud_knn_mean_sums_read)."""
    d = L.as_dtype(torch.float32, False, dist, "dist")
    if d.dim() != 2 or not 1 <= d.shape[1] <= CLOUD_KNN_MAX:
        raise ValueError(f"dist must be (n,k) with k in 1..{CLOUD_KNN_MAX}, got {tuple(d.shape)}")
    dev, (n, k) = d.device, d.shape
    cnt = L.as_dtype(torch.int32, False, count, "count", (n,), dev)
    mean = torch.empty(n, dtype=torch.float64, device=dev)
    result = _result_block(result, 4, dev, "dist's")
    nbytes = L.load().mvd_cloud_knn_mean_sums_workspace_bytes(n)
    ws = workspace(nbytes, dev)
    call("mvd_cloud_knn_mean_sums_f32", dev, d, cnt, n, k, mean, result, ws, int(nbytes))
    return mean, result


def cloud_knn_mean_sums_read(result):
    """cloud_knn_mean_sums' block on the host -> (sum of the means, sum of their squares, their number): the one read of the rule."""
    r = result.cpu()
    s = r[:2].view(torch.float64)
    return float(s[0]), float(s[1]), int(r[2])


@inference_only
def cloud_keep_threshold(mean, threshold):
    """keep (n) uint8: mean <= threshold, 0 for a NaN mean (include/mvd.h: mvd_cloud_keep_threshold)."""
    mu = L.as_dtype(torch.float64, False, mean, "mean")
    if mu.dim() != 1:
        raise ValueError(f"mean must be (n,), got {tuple(mu.shape)}")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold is NaN")
    keep = torch.empty(mu.shape[0], dtype=torch.uint8, device=mu.device)
    call("mvd_cloud_keep_threshold", mu.device, mu, mu.shape[0], threshold, keep)
    return keep


@inference_only
def cloud_select(keep):
    """The kept points of keep (n) uint8 (include/mvd.h: mvd_cloud_select) -> (kept (K) int32: their indices ascending, remap (n) int32:
    the new index or -1, K); the count is the one read.  Rows follow through mesh_gather_rows(src, remap, K)."""
    kp = L.as_dtype(torch.uint8, False, keep, "keep")
    if kp.dim() != 1:
        raise ValueError(f"keep must be (n,), got {tuple(kp.shape)}")
    n, dev = kp.shape[0], kp.device
    if n >= 2 ** 31:
        raise ValueError(f"keep: {n} points, supported below 2^31")
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    remap = torch.empty(n, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    nbytes = L.load().mvd_cloud_select_workspace_bytes(n)
    ws = workspace(nbytes, dev)
    call("mvd_cloud_select", dev, kp, n, kept, remap, total, ws, int(nbytes))
    K = int(total.item())
    return kept[:K].clone(), remap, K


MESH_MAX_PAIRS = 1 << 28    # mesh_grid's default bound on the (cell, triangle) pairs: 2^28 pairs are 15 GB of keys, permutation and records
MESH_MAX_SAMPLES = 1 << 28  # mesh_sample's default bound on the samples
_MESH_HARD_LIMIT = 2 ** 31 - 1


def _mesh_bound(value, name):
    value = int(value)
    if not 1 <= value <= _MESH_HARD_LIMIT:
        raise ValueError(f"{name} must be in 1 .. 2^31 - 1, got {value}")
    return value


def _mesh_ends(counts):
    """The inclusive prefix sums of per-triangle int64 counts (torch.cumsum: plumbing), and their total and the largest count in ONE
    read -> (ends, total, largest)."""
    if counts.numel() == 0:
        return counts, 0, 0
    ends = torch.cumsum(counts, dim=0)
    total, largest = torch.stack([ends[-1], counts.max()]).tolist()
    return ends, int(total), int(largest)


class MeshGrid:
    """A mesh's triangles entered into the cells of a uniform grid (mesh_grid): vertices (M,3) and triangles (T,3) as given, keys (P)
    int64 ascending: the cell of each (cell, triangle) pair, records (P,12): the pairs' triangles in key order (three vertices, the
    triangle's index as the bits of the tenth float, two zeros), origin (3 floats), cell and inv = 1.0 / cell."""
    __slots__ = ("vertices", "triangles", "keys", "records", "origin", "cell", "inv")

    def __init__(self, vertices, triangles, keys, records, origin, cell):
        self.vertices, self.triangles, self.keys, self.records, self.origin, self.cell = vertices, triangles, keys, records, origin, cell
        self.inv = 1.0 / cell

    @property
    def pair_triangles(self):
        """(P) int32: the triangle of each pair, in key order"""
        return self.records[:, 9].contiguous().view(torch.int32)


@inference_only
def mesh_grid(vertices, triangles, origin, cell, max_pairs=MESH_MAX_PAIRS):
    """The triangles of a mesh entered into every cell (edge `cell`, from `origin`) of their axis-aligned boxes (include/mvd.h:
    mvd_mesh_cell_counts_f32, mvd_mesh_pairs_f32, mvd_mesh_records_f32; mesh_eval.mesh_grid_pairs_numpy is the definition) ->
    MeshGrid.  Every finite vertex's cell indices must be in [0, 2^21 - 1), else ValueError.  The number of pairs P is read once; more
    than max_pairs (at most 2^31 - 1) raises ValueError: a larger cell gives fewer pairs (and more candidates per query)."""
    v = _device_vertices(vertices, convert=True)
    t = _device_triangles(triangles, v.shape[0], v.device)
    dev, M, T = v.device, int(v.shape[0]), int(t.shape[0])
    origin, cell, max_pairs = _cloud_origin(origin), float(cell), _mesh_bound(max_pairs, "max_pairs")
    if not 0.0 < cell < float("inf"):
        raise ValueError(f"cell must be finite and > 0, got {cell}")
    inv = 1.0 / cell
    _check_cloud_indices(cloud_extent(v), origin, inv, "mesh_grid", cell)
    counts = torch.empty(T, dtype=torch.int64, device=dev)
    if T:
        call("mvd_mesh_cell_counts_f32", dev, v if M else None, M, t, T, origin[0], origin[1], origin[2], inv, counts)
    ends, P, largest = _mesh_ends(counts)
    if P > max_pairs:
        raise ValueError(f"mesh_grid: {P} (cell, triangle) pairs at a cell of {cell:g}, above max_pairs = {max_pairs}; the largest "
                         f"triangle's box alone covers {largest} cells.  Pass a larger cell= (it may exceed max_dist * (1 + 2^-10): fewer "
                         "pairs, more candidates per query) or raise max_pairs")
    keys = torch.empty(P, dtype=torch.int64, device=dev)
    pair_tri = torch.empty(P, dtype=torch.int32, device=dev)
    records = torch.empty((P, 12), dtype=torch.float32, device=dev)
    if P:
        call("mvd_mesh_pairs_f32", dev, v, M, t, T, ends, P, origin[0], origin[1], origin[2], inv, keys, pair_tri)
        keys, perm = torch.sort(keys, stable=True)  # torch's sort: plumbing between two kernels, as cloud_sorted's
        call("mvd_mesh_records_f32", dev, v, M, t, T, pair_tri, perm, P, records)
    return MeshGrid(v, t, keys, records, origin, cell)


@inference_only
def mesh_nearest(query, grid, max_dist):
    """The truncated nearest triangle of every query in the grid's mesh (include/mvd.h: mvd_mesh_nearest_f32).  query: (n,3) points,
    sorted here by the grid's cells, or a CloudGrid of the same origin and cell (MeshEvaluation sorts a cloud once for both
    directions).  grid.cell must be at least max_dist * (1 + 2^-10).
    Returns (dist (n) float32, index (n) int32: the triangle) in the query's original order; index -1 = nothing nearer than max_dist."""
    if not isinstance(grid, MeshGrid):
        raise ValueError(f"grid: expected a MeshGrid (ops.mesh_grid), got {type(grid).__name__}")
    dev = grid.vertices.device
    max_dist = float(torch.tensor(max_dist, dtype=torch.float32))  # the float32 the kernel compares with
    if not 0.0 < max_dist < float("inf"):
        raise ValueError(f"max_dist must be finite and > 0, got {max_dist}")
    if grid.cell < max_dist * CLOUD_CELL_MARGIN * (1 - 1e-12):
        raise ValueError(f"the grid's cell {grid.cell:g} is below max_dist * (1 + 2^-10) = {max_dist * CLOUD_CELL_MARGIN:g}")
    if isinstance(query, CloudGrid):
        if query.origin != grid.origin or query.cell != grid.cell or query.points.device != dev:
            raise ValueError("query and mesh grids differ in origin, cell or device")
        rec = query.records
    else:
        rec = cloud_grid(cloud_points(query, "query", dev), grid.origin, grid.cell, check=False).records
    n, P = rec.shape[0], grid.keys.shape[0]
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    index = torch.empty(n, dtype=torch.int32, device=dev)
    call("mvd_mesh_nearest_f32", dev, rec if n else None, n, grid.records if P else None, grid.keys if P else None, P, grid.origin[0],
         grid.origin[1], grid.origin[2], grid.inv, max_dist, dist if n else None, index if n else None)
    return dist, index


@inference_only
def mesh_sample(vertices, triangles, spacing, attributes=None, max_samples=MESH_MAX_SAMPLES):
    """Deterministic covering samples of a mesh's surface (include/mvd.h: mvd_mesh_sample_counts_f32, mvd_mesh_sample_f32;
    mesh_eval.sample_mesh_numpy is the definition, bit for bit): a triangle whose longest edge is L gets k = max(1, ceil(L / spacing))
    and the centroids of its k^2 congruent sub-triangles, so that every surface point is within 2 spacing / 3 of a sample.
    attributes (M,c) float32 are interpolated with the points.  The number of samples S is read once; more than max_samples (at most
    2^31 - 1) raises ValueError.  Returns (points (S,3) float32, triangle (S) int32, attributes (S,c) or None), in triangle order."""
    v = _device_vertices(vertices, convert=True)
    t = _device_triangles(triangles, v.shape[0], v.device)
    dev, M, T = v.device, int(v.shape[0]), int(t.shape[0])
    spacing, max_samples = float(torch.tensor(float(spacing), dtype=torch.float32)), _mesh_bound(max_samples, "max_samples")
    if not 0.0 < spacing < float("inf"):
        raise ValueError(f"spacing must be finite and > 0, got {spacing}")
    inv_s2 = 1.0 / (spacing * spacing)
    if not 0.0 < inv_s2 < float("inf"):
        raise ValueError(f"spacing {spacing:g}: 1 / spacing^2 is not a finite positive double")
    attr, C = None, 0
    if attributes is not None:
        attr = L.as_f32(attributes, "attributes", device=dev)
        if attr.dim() != 2 or attr.shape[0] != M or not 1 <= attr.shape[1] <= 65536:
            raise ValueError(f"attributes must be ({M},c) with c in 1 .. 65536, got {tuple(attr.shape)}")
        C = int(attr.shape[1])
    counts = torch.empty(T, dtype=torch.int64, device=dev)
    if T:
        call("mvd_mesh_sample_counts_f32", dev, v if M else None, M, t, T, inv_s2, counts)
    ends, S, largest = _mesh_ends(counts)
    if S > max_samples:
        raise ValueError(f"mesh_sample: {S} samples at a spacing of {spacing:g}, above max_samples = {max_samples}; the largest triangle "
                         f"alone gets {largest}.  Pass a larger spacing or raise max_samples")
    points = torch.empty((S, 3), dtype=torch.float32, device=dev)
    tri = torch.empty(S, dtype=torch.int32, device=dev)
    out = torch.empty((S, C), dtype=torch.float32, device=dev) if attr is not None else None
    if S:
        call("mvd_mesh_sample_f32", dev, v, M, t, T, attr, C, ends, S, inv_s2, points, tri, out)
    return points, tri, out


class SplitConv2dWeights:
    """Packed split-operand weights of one 2-D layer (pack_conv2d_weights_split) with what conv2d_split needs to call it."""
    __slots__ = ("packed", "bias", "cin", "cin_pad", "cout", "kh", "kw", "stride", "mode")

    def __init__(self, packed, bias, cin, cin_pad, cout, kh, kw, stride, mode):
        self.packed, self.bias, self.cin, self.cin_pad, self.cout = packed, bias, cin, cin_pad, cout
        self.kh, self.kw, self.stride, self.mode = kh, kw, stride, mode


@inference_only
def pack_conv2d_weights_split(weight, bias=None, stride=1, mode=L.CONV2D, cin_pad=None):
    """weight: Conv2d (Cout,Cin,k,k) (mode CONV2D / CONV2D_IMAGE) or ConvTranspose2d (Cin,Cout,4,4) (mode DECONV2D), fp32 ->
    SplitConv2dWeights for conv2d_split.  cin_pad: the channel count of the (zero-padded) input slice the layer will read, a
    multiple of 8 (default: Cin rounded up to 8)."""
    wt = L.as_f32(weight, "weight")
    if wt.dim() != 4:
        raise ValueError(f"weight must be 4-D, got {tuple(wt.shape)}")
    if mode == L.DECONV2D:
        cin, cout = wt.shape[0], wt.shape[1]
    else:
        cout, cin = wt.shape[0], wt.shape[1]
    kh, kw = wt.shape[2], wt.shape[3]
    cin_pad = (cin + 7) // 8 * 8 if cin_pad is None else int(cin_pad)
    nbytes = L.load().mvd_conv2d_split_packed_weight_bytes(cin_pad, cout, kh, kw, stride, mode) if cin_pad >= cin else 0
    if nbytes == 0:
        raise ValueError(f"conv2d split: a {kh}x{kw} stride-{stride} layer (mode {mode}) with {cin} (padded {cin_pad}) -> {cout} channels is not built")
    packed = torch.empty(nbytes, dtype=torch.uint8, device=wt.device)
    call("mvd_pack_conv2d_weights_split", wt.device, wt, cin, cin_pad, cout, kh, kw, stride, mode, packed)
    b = None if bias is None else L.as_f32(bias.detach(), "bias", (cout,), wt.device).clone()
    return SplitConv2dWeights(packed, b, cin, cin_pad, cout, kh, kw, stride, mode)


def _nhwc_slice(t, name, channels=None, free_rows=False):
    """(B,H,W,C) fp32 device view with unit channel stride -> (B,H,W,C, pixel stride, row stride, image stride) in floats.  Without
    free_rows the view must be a channel slice of a dense NHWC buffer (rows and images follow each other)."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
        raise ValueError(f"{name} must be a float32 device tensor (B,H,W,C)")
    B, H, W, C = t.shape
    ps = t.stride(2) if W > 1 else max(C, 1)
    rs = t.stride(1) if H > 1 else W * ps
    ims = t.stride(0) if B > 1 else H * rs
    if (C > 1 and t.stride(3) != 1) or ps < C or rs < W * ps or ims < H * rs:
        raise ValueError(f"{name}: a channel slice of a channel-last buffer is needed, got shape {tuple(t.shape)} strides {t.stride()}")
    if not free_rows and (rs != W * ps or ims != H * rs):
        raise ValueError(f"{name}: a channel slice of a DENSE channel-last buffer is needed, got shape {tuple(t.shape)} strides {t.stride()}")
    if channels is not None and C != channels:
        raise ValueError(f"{name}: {C} channels, the layer takes {channels}")
    return B, H, W, C, ps, rs, ims


@inference_only
def conv2d_split(x, x_absmax, wts, act=1, slope=0.2, out=None, out_absmax=None, use_workspace=True, planar_out=False):
    """One layer of Path A's 2-D CNN on the split-operand kernel.  x: (B,Hi,Wi,Cin_pad) NHWC fp32, possibly
    a channel slice of a wider buffer (mode CONV2D_IMAGE: the planar (B,3,Hi,Wi) image); x_absmax: one-element device tensor with
    max |x|; wts: SplitConv2dWeights.  out: NHWC destination view (B,Ho,Wo,Cout), e.g. a slice of a concat buffer or the interior
    of a zero-bordered map (allocated if None); planar_out: allocate and return (B,Cout,Ho,Wo) instead.  out_absmax: one-element
    device tensor that receives max |out| by atomic maximum (zero it first), or None.  act 0 none / 1 LeakyReLU(slope) / 2 ReLU."""
    if wts.mode == L.CONV2D_IMAGE:
        xi = L.as_f32(x, "x")
        if xi.dim() != 4 or xi.shape[1] != 3:
            raise ValueError(f"x must be the planar image (B,3,H,W), got {tuple(xi.shape)}")
        B, _, Hi, Wi = xi.shape
        x, xs = xi, 0
    else:
        B, Hi, Wi, _, xs, _, _ = _nhwc_slice(x, "x", wts.cin_pad)
    if wts.mode == L.DECONV2D:
        Ho, Wo = 2 * Hi, 2 * Wi
    else:
        Ho = (Hi + 2 * (wts.kh // 2) - wts.kh) // wts.stride + 1
        Wo = (Wi + 2 * (wts.kw // 2) - wts.kw) // wts.stride + 1
    dev = x.device
    if planar_out:
        if out is not None:
            raise ValueError("planar_out allocates its own output")
        out = torch.empty((B, wts.cout, Ho, Wo), dtype=torch.float32, device=dev)
        ys, rs, ims, cs = 1, Wo, wts.cout * Ho * Wo, Ho * Wo
    else:
        if out is None:
            out = torch.empty((B, Ho, Wo, wts.cout), dtype=torch.float32, device=dev)
        ob, oh, ow, _, ys, rs, ims = _nhwc_slice(out, "out", wts.cout, free_rows=True)
        cs = 1
        if (ob, oh, ow) != (B, Ho, Wo):
            raise ValueError(f"out is {tuple(out.shape)}, the layer writes ({B},{Ho},{Wo},{wts.cout})")
    xam = L.as_f32(x_absmax, "x_absmax", (1,), dev)
    yam = None if out_absmax is None else L.as_f32(out_absmax, "out_absmax", (1,), dev)
    wsb = L.load().mvd_conv2d_split_workspace_bytes(B, Hi, Wi, wts.cin_pad, wts.cout, wts.kh, wts.kw, wts.stride, wts.mode) if use_workspace else 0
    call("mvd_conv2d_split_f32", dev, x, xam, wts.packed, wts.bias, out, yam, B, Hi, Wi, wts.cin_pad, xs, wts.cout, ys, rs, ims, cs,
          wts.kh, wts.kw, wts.stride, wts.mode, int(act), float(slope), workspace(wsb, dev) if wsb else None, wsb)
    return out


@inference_only
def upsample2x_into(x, out, out_absmax=None):
    """F.interpolate(x, size=(2h,2w), mode="bilinear", align_corners=False) of a planar (B,C,h,w) map written into the channel-last
    slice out (B,2h,2w,C) (the decoder's up-sampled prediction inside the next level's concat buffer)."""
    x = L.as_f32(x, "x")
    B, C, h, w = x.shape
    ob, oh, ow, _, ys, _, _ = _nhwc_slice(out, "out", C)
    if (ob, oh, ow) != (B, 2 * h, 2 * w):
        raise ValueError(f"out is {tuple(out.shape)}, expected ({B},{2 * h},{2 * w},{C})")
    yam = None if out_absmax is None else L.as_f32(out_absmax, "out_absmax", (1,), x.device)
    call("mvd_upsample2x_nhwc_f32", x.device, x, out, yam, B, C, h, w, ys)
    return out


@inference_only
def sweep_corr_nhwc(feat_key, feat_sources, K_key, K_sources, T_src2key, invdepths, corrs, masks, corr_scale=None, corr_absmax=None):
    """K1 on its working layouts: feat_key (N,h,w,C) channel-last; feat_sources V x zero-bordered
    channel-last (N,hs+3,ws+3,C); corrs, masks: V x pixel-major destinations (N,h,w,S) (channel slices allowed), filled in place.
    corr_absmax: one-element device tensor raised to max |corr| over all views (zero it first), or None."""
    fk = L.as_f32(feat_key, "feat_key")
    N, h, w, C = fk.shape
    dev = fk.device
    srcs = views(feat_sources, "feat_sources")
    V = len(srcs)
    hs, ws = srcs[0].shape[1] - 3, srcs[0].shape[2] - 3
    srcs = [L.as_f32(s, f"feat_sources[{i}]", (N, hs + 3, ws + 3, C), dev) for i, s in enumerate(srcs)]
    Kk, Ks, Ts, inv, mode = _k1_calibration(K_key, K_sources, T_src2key, invdepths, V, N, h, w, dev)
    S = inv.shape[1]
    if C % 64 != 0:
        raise ValueError(f"feature channels C={C} must be a multiple of 64")
    ps = None
    for name, ts in (("corrs", corrs), ("masks", masks)):
        if len(ts) != V:
            raise ValueError(f"{name}: {len(ts)} entries for {V} views")
        for t in ts:
            b_, h_, w_, _, p_, _, _ = _nhwc_slice(t, name, S)
            if (b_, h_, w_) != (N, h, w) or (ps is not None and p_ != ps):
                raise ValueError(f"{name}: (N,h,w,S) = ({N},{h},{w},{S}) maps with one common pixel stride are needed")
            ps = p_
    cam = None if corr_absmax is None else L.as_f32(corr_absmax, "corr_absmax", (1,), dev)
    call("mvd_sweep_corr_nhwc_f32", dev, fk, srcs, Kk, Ks, Ts, inv, mode, _corr_scale(corr_scale, C), N, C, h, w, hs, ws, S, V,
          list(corrs), list(masks), ps, cam)
    return corrs, masks


@inference_only
def fuse_views_nhwc(corrs, masks, scores, out, out_absmax=None):
    """K2 on pixel-major volumes: corrs, masks V x (N,h,w,S); scores V x (N,h,w,1) or (N,1,h,w); out: (N,h,w,S) destination view
    (a channel slice of the cost-volume encoder's input buffer).  Returns out."""
    V = len(corrs)
    N, h, w, S, ps, _, _ = _nhwc_slice(corrs[0], "corrs[0]")
    dev = corrs[0].device
    for name, ts in (("corrs", corrs), ("masks", masks)):
        for t in ts:
            if _nhwc_slice(t, name, S)[:5] != (N, h, w, S, ps):
                raise ValueError(f"{name}: equal (N,h,w,S) maps are needed")
    scores = [L.as_f32(s_.reshape(N, h * w), f"scores[{i}]", (N, h * w), dev) for i, s_ in enumerate(views(scores, "scores", V))]
    ob, oh, ow, _, ops_, _, _ = _nhwc_slice(out, "out", S)
    if (ob, oh, ow) != (N, h, w):
        raise ValueError(f"out is {tuple(out.shape)}, expected ({N},{h},{w},{S})")
    yam = None if out_absmax is None else L.as_f32(out_absmax, "out_absmax", (1,), dev)
    call("mvd_fuse_views_nhwc_f32", dev, list(corrs), list(masks), scores, N, S, h, w, V, ps, out, None, ops_, yam)
    return out


@inference_only
def bias_leaky_relu_(x, bias, slope=0.2):
    """In place: x (N,C,H,W) contiguous <- leaky_relu(x + bias[c], slope).  Returns x."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() >= 2):
        raise ValueError("bias_leaky_relu_: x must be a contiguous fp32 device tensor (N,C,...)")
    N, C = x.shape[0], x.shape[1]
    b = L.as_f32(bias, "bias", (C,), x.device)
    call("mvd_bias_leaky_relu_f32", x.device, x, b, N, C, x.numel() // (N * C), float(slope))
    return x


@inference_only
def resize_order1(images, ht, wd):
    """images (..., H, W) fp32 device tensor -> (..., ht, wd): skimage.transform.resize(order=1) for upscaling
    (rmvd/data/transforms.py:64-66), on the device."""
    x = L.as_f32(images, "images")
    if x.dim() < 2:
        raise ValueError("images must be (..., H, W)")
    hi, wi = x.shape[-2:]
    if ht < hi or wd < wi:
        raise ValueError(f"resize_order1: only upscaling is built ({hi}x{wi} -> {ht}x{wd})")
    planes = x.numel() // (hi * wi)
    y = torch.empty(tuple(x.shape[:-2]) + (ht, wd), dtype=torch.float32, device=x.device)
    call("mvd_resize_order1_f32", x.device, x, y, planes, hi, wi, ht, wd)
    return y


@inference_only
def dispnet_head(x):
    """x (N,2,h,w) raw output of a pred_k convolution -> (pred (N,2,h,w) = [relu(x0), sigmoid(0.2 x1) * 20 - 10],
    entropy (N,1,h,w) = log(2 exp(pred1) + 1e-4) + 1) in one launch (dispnet_decoder.py:17-22,126-138)."""
    x = L.as_f32(x, "x")
    if x.dim() != 4 or x.shape[1] != 2:
        raise ValueError(f"x must be (N,2,h,w), got {tuple(x.shape)}")
    N, _, h, w = x.shape
    pred = torch.empty_like(x)
    ent = torch.empty((N, 1, h, w), dtype=torch.float32, device=x.device)
    call("mvd_dispnet_head_f32", x.device, x, pred, ent, N, h * w)
    return pred, ent


@inference_only
def zero_border_nhwc(buf):
    """buf (B, h + 3, w + 3, C) contiguous fp32, K3's zero-bordered staging map: zeroes row 0, rows h + 1 and h + 2, column 0 and
    columns w + 1 and w + 2 in place and leaves the interior to its producer.  Returns buf."""
    if not (isinstance(buf, torch.Tensor) and buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous() and buf.dim() == 4):
        raise ValueError("zero_border_nhwc: buf must be a contiguous (B, h + 3, w + 3, C) fp32 device tensor")
    B, hp, wp, C = buf.shape
    if hp < 4 or wp < 4 or C % 4:
        raise ValueError(f"zero_border_nhwc: shape {tuple(buf.shape)} (h, w >= 1, C a multiple of 4)")
    call("mvd_zero_border_nhwc_f32", buf.device, buf, B, hp - 3, wp - 3, C)
    return buf


@inference_only
def to_channels_last_3d(x):
    """(B,C,D,h,w) -> (B,D,h,w,C) through the library's tiled transpose."""
    x = L.as_f32(x, "x")
    B, C, D, h, w = x.shape
    y = torch.empty((B, D, h, w, C), dtype=torch.float32, device=x.device)
    call("mvd_nchw_to_nhwc_f32", x.device, x, y, B, C, D * h * w)
    return y


@inference_only
def from_channels_last_3d(y):
    """(B,D,h,w,C) -> (B,C,D,h,w)."""
    y = L.as_f32(y, "y")
    B, D, h, w, C = y.shape
    x = torch.empty((B, C, D, h, w), dtype=torch.float32, device=y.device)
    call("mvd_nhwc_to_nchw_f32", y.device, y, x, B, C, D * h * w)
    return x


# ------------------------------------------------------------------------------------------------
# Differentiable forms: torch.autograd.Function wrappers whose backward runs the engine's VJP
# kernels (include/mvd.h "Backward of the sweep operators").  Gradients flow to the FEATURE MAPS (and, for the fusion, to
# the score maps); calibration, depth samples and masks are constants, exactly as in the reference
# (planesweep_corr.py:436,464,489 compute the grids under no_grad).
# ------------------------------------------------------------------------------------------------
def _bordered_channels_last(x):
    """(N,C,h,w) -> zero-bordered channel-last (N,h+3,w+3,C) with the map at (1,1): the layout the kernels gather from."""
    n, c, h, w = x.shape
    out = torch.zeros((n, h + 3, w + 3, c), dtype=torch.float32, device=x.device)
    out[:, 1:h + 1, 1:w + 1] = x.permute(0, 2, 3, 1)
    return out


def _interior_nchw(g, h, w):
    return g[:, 1:h + 1, 1:w + 1].permute(0, 3, 1, 2).contiguous()


class _WarpVariance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, key_proj_inv, depth_values, n_views, backward, fallback_count, key_feat, *rest):
        srcs, projs = list(rest[:n_views]), list(rest[n_views:])
        ctx.save_for_backward(key_proj_inv, depth_values, key_feat, *srcs, *projs)
        ctx.n_views, ctx.mode, ctx.fallback_count = n_views, backward, fallback_count
        return warp_variance(key_feat.detach(), [s.detach() for s in srcs], projs, key_proj_inv, depth_values)

    @staticmethod
    def backward(ctx, gvar):
        V = ctx.n_views
        kpi, dv, key = ctx.saved_tensors[:3]
        srcs, projs = list(ctx.saved_tensors[3:3 + V]), list(ctx.saved_tensors[3 + V:])
        B, C, h, w = key.shape
        dev = key.device
        with torch.no_grad():
            kb = _bordered_channels_last(key.float())
            sb = [_bordered_channels_last(s.float()) for s in srcs]
            g = gvar.float().permute(0, 2, 3, 4, 1).contiguous()  # (B,D,h,w,C)
            gk = torch.empty_like(kb)
            gs = [torch.empty_like(kb) for _ in range(V)]
            projs, kpi, dv = _k3_calibration(projs, kpi, dv, V, B, C, dev)
            if ctx.mode == "gather":
                wsb = L.load().mvd_warp_variance_backward_gather_workspace_bytes(B, C, dv.shape[1], h, w, V)
                call("mvd_warp_variance_backward_gather_f32", dev, kb, sb, projs, kpi, dv, g, B, C, dv.shape[1], h, w, V, gk, gs,
                      ctx.fallback_count, workspace(wsb, dev), wsb)
            else:
                wsb = L.load().mvd_warp_variance_backward_workspace_bytes(B)
                call("mvd_warp_variance_backward_f32", dev, kb, sb, projs, kpi, dv, g, B, C, dv.shape[1], h, w, V, gk, gs,
                      workspace(wsb, dev), wsb)
            out = [None] * 5 + [_interior_nchw(gk, h, w)] + [_interior_nchw(x, h, w) for x in gs] + [None] * V
        return tuple(out)


K3_BACKWARDS = ("atomic", "gather")


def warp_variance_autograd(key_feat, src_feats, src_projs, key_proj_inv, depth_values, backward="atomic", fallback_count=None):
    """Differentiable K3: like warp_variance (reference layout (B,C,D,h,w)), with gradients to key_feat and src_feats.
    backward: "atomic" (default) scatters the source gradients with float atomics, so their last bits vary from run to run;
    "gather" collects them per source pixel in a fixed order (mvd_warp_variance_backward_gather_f32): two calls on the same inputs
    give the same bits.  A view whose mapping minifies beyond the gather's window (more than L.K3_GATHER_RADIUS key pixels from a
    source pixel's centre) is detected on the device and takes the atomic path; fallback_count, an int32 device tensor of one
    element, is then raised by the number of such (batch element, view) (no host synchronisation: read it when you choose)."""
    if backward not in K3_BACKWARDS:
        raise ValueError(f"backward must be 'atomic' or 'gather', got {backward!r}")
    if fallback_count is not None:
        if backward != "gather":
            raise ValueError("fallback_count belongs to backward='gather'")
        if not (isinstance(fallback_count, torch.Tensor) and fallback_count.is_cuda and fallback_count.dtype == torch.int32
                and fallback_count.numel() == 1):
            raise ValueError("fallback_count must be a one-element int32 device tensor")
    srcs = views(src_feats, "src_feats")
    return _WarpVariance.apply(key_proj_inv, depth_values, len(srcs), backward, fallback_count, key_feat, *srcs,
                               *views(src_projs, "src_projs", len(srcs)))


class _SweepCorr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K_key, invdepths, n_views, corr_scale, feat_key, *rest):
        V = n_views
        srcs, Ks, Ts = list(rest[:V]), list(rest[V:2 * V]), list(rest[2 * V:])
        corrs, masks = sweep_corr(feat_key.detach(), [s.detach() for s in srcs], K_key, Ks, Ts, invdepths, corr_scale)
        ctx.save_for_backward(K_key, invdepths, feat_key, *srcs, *Ks, *Ts)
        ctx.n_views = V
        ctx.corr_scale = corr_scale
        ctx.mark_non_differentiable(*masks)
        return tuple(corrs) + tuple(masks)

    @staticmethod
    def backward(ctx, *grads):
        V = ctx.n_views
        Kk, inv, fk = ctx.saved_tensors[:3]
        srcs = list(ctx.saved_tensors[3:3 + V])
        Ks, Ts = list(ctx.saved_tensors[3 + V:3 + 2 * V]), list(ctx.saved_tensors[3 + 2 * V:])
        N, C, h, w = fk.shape
        hs, ws = srcs[0].shape[-2:]
        S = inv.shape[1]
        dev = fk.device
        with torch.no_grad():
            key = fk.float().permute(0, 2, 3, 1).contiguous()
            sb = [_bordered_channels_last(s.float()) for s in srcs]
            gc = [(g if g is not None else torch.zeros((N, S, h, w), device=dev)).float().contiguous() for g in grads[:V]]
            gk = torch.empty_like(key)
            gs = [torch.empty_like(sb[0]) for _ in range(V)]
            Kk, Ks, Ts, inv, mode = _k1_calibration(Kk, Ks, Ts, inv, V, N, h, w, dev)
            call("mvd_sweep_corr_backward_f32", dev, key, sb, Kk, Ks, Ts, inv, mode, _corr_scale(ctx.corr_scale, C), gc,
                  N, C, h, w, hs, ws, S, V, gk, gs)
            out = [None, None, None, None, gk.permute(0, 3, 1, 2).contiguous()] + [_interior_nchw(x, hs, ws) for x in gs] + [None] * (2 * V)
        return tuple(out)


K1_BACKWARD_CHANNELS = (64, 128, 192, 256)  # sweep_corr_backward_kernel<C / 64> (csrc/backward.hip)


def sweep_corr_autograd(feat_key, feat_sources, K_key, K_sources, T_src2key, invdepths, corr_scale=None):
    """Differentiable K1: returns (corrs[V], masks[V]); gradients to feat_key and feat_sources.  The VJP kernel is built for
    K1_BACKWARD_CHANNELS only: another channel count that the forward accepts (a multiple of 64 above 256) is refused here, before
    any kernel runs, when a gradient will be asked for; without one it is computed as by sweep_corr."""
    srcs = views(feat_sources, "feat_sources")
    V = len(srcs)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in [feat_key] + srcs):
        C = feat_key.shape[1] if isinstance(feat_key, torch.Tensor) and feat_key.dim() == 4 else None
        if C is not None and C % 64 == 0 and C not in K1_BACKWARD_CHANNELS:
            raise ValueError(f"sweep_corr_autograd: feature channels C={C} have no backward kernel (supported with gradients: "
                             f"{', '.join(map(str, K1_BACKWARD_CHANNELS))}); run it under torch.no_grad() or on detached features")
    outs = _SweepCorr.apply(K_key, invdepths, V, corr_scale, feat_key, *srcs, *views(K_sources, "intrinsics_sources", V),
                            *views(T_src2key, "source_to_key_transforms", V))
    return list(outs[:V]), list(outs[V:])


class _SweepWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K_key, invdepths, key_size, n_views, *rest):
        V = n_views
        srcs, Ks, Ts = list(rest[:V]), list(rest[V:2 * V]), list(rest[2 * V:])
        outs, masks = sweep_warp([s.detach() for s in srcs], K_key, Ks, Ts, invdepths, key_size, False)
        ctx.save_for_backward(K_key, invdepths, *Ks, *Ts)  # the op is linear in the features: the VJP needs their shape only
        ctx.n_views, ctx.key_size, ctx.src_shape = V, (int(key_size[0]), int(key_size[1])), tuple(srcs[0].shape)
        ctx.mark_non_differentiable(*masks)
        return tuple(outs) + tuple(masks)

    @staticmethod
    def backward(ctx, *grads):
        V = ctx.n_views
        Kk, inv = ctx.saved_tensors[:2]
        Ks, Ts = list(ctx.saved_tensors[2:2 + V]), list(ctx.saved_tensors[2 + V:])
        N, C, hs, ws = ctx.src_shape
        h, w = ctx.key_size
        dev = Kk.device
        with torch.no_grad():
            Kk, Ks, Ts, inv, mode = _k1_calibration(Kk, Ks, Ts, inv, V, N, h, w, dev)
            S = inv.shape[1]
            gw = [L.as_f32(g, f"grad_warped[{i}]", (N, S, C, h, w), dev) for i, g in enumerate(grads[:V])]
            gs = [torch.empty((N, hs + 3, ws + 3, C), dtype=torch.float32, device=dev) for _ in range(V)]
            call("mvd_sweep_warp_backward_f32", dev, Kk, Ks, Ts, inv, mode, gw, N, C, h, w, hs, ws, S, V, gs)
            gsrc = [_interior_nchw(g, hs, ws) if need else None for g, need in zip(gs, ctx.needs_input_grad[4:4 + V])]
        return (None,) * 4 + tuple(gsrc) + (None,) * (2 * V)


class _ForwardValue(torch.autograd.Function):
    """y with the value of `value` (same shape): the gradient goes to y unchanged."""
    @staticmethod
    def forward(ctx, y, value):
        return value.view_as(y)

    @staticmethod
    def backward(ctx, g):
        return g, None


def sweep_warp_autograd(feat_sources, K_key, K_sources, T_src2key, invdepths, key_size, normalize_after=False):
    """Differentiable sweep_warp: returns (warped[V] (N,S,C,h,w), masks[V] (N,S,h,w)) with the same bits; gradients to
    feat_sources (mvd_sweep_warp_backward_f32), calibration, inverse depths and masks are constants.  The VJP kernel is the
    un-normalised warp's.  normalize_after: x / (|x|_2 + 1e-9) along C is applied to the un-normalised warp in torch and
    differentiated by autograd (a masked sample is 0 before and after it); the VALUE handed back is the fused inference kernel's
    own, so that training and inference see one forward."""
    srcs = views(feat_sources, "feat_sources")
    V = len(srcs)
    Ks, Ts = views(K_sources, "intrinsics_sources", V), views(T_src2key, "source_to_key_transforms", V)
    outs = _SweepWarp.apply(K_key, invdepths, tuple(key_size), V, *srcs, *Ks, *Ts)
    warped, masks = list(outs[:V]), list(outs[V:])
    if normalize_after:
        exact, _ = sweep_warp([s.detach() for s in srcs], K_key, Ks, Ts, invdepths, key_size, True)
        warped = [_ForwardValue.apply(u / (torch.linalg.norm(u, dim=2, keepdim=True) + 1e-9), e) for u, e in zip(warped, exact)]
    return warped, masks


class _SweepReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, mode, groups, pix_offset, stretch, n_views, key_feat, *rest):
        from . import sweep_modes
        V = n_views
        srcs, Ms = list(rest[:V]), list(rest[V:])
        ctx.save_for_backward(depth, key_feat, *srcs, *Ms)
        ctx.cfg = (mode, groups, pix_offset, stretch, V)
        out = sweep_modes.sweep_reduce_inference(key_feat.detach(), [s.detach() for s in srcs], Ms, depth, mode, groups, pix_offset, stretch)
        return tuple(out) if mode == L.REDUCE_GROUPCORR else out

    @staticmethod
    def backward(ctx, *grads):
        from . import sweep_modes
        mode, groups, pix_offset, stretch, V = ctx.cfg
        depth, key = ctx.saved_tensors[:2]
        srcs, Ms = list(ctx.saved_tensors[2:2 + V]), list(ctx.saved_tensors[2 + V:])
        with torch.no_grad():
            kf, srcs, Ms, dv, per_pixel, (B, C, D, h, w, _), (sx, sy) = sweep_modes._reduce_args(key, srcs, Ms, depth, mode, groups, stretch)
            dev = kf.device
            oshape = (B, groups, D, h, w) if mode == L.REDUCE_GROUPCORR else (B, C, D, h, w)
            gout = [L.as_f32(g, f"grad_out[{i}]", oshape, dev) for i, g in enumerate(grads)]
            gk = torch.empty_like(kf)
            gs = [torch.empty_like(kf) for _ in range(V)]
            wsb = L.load().mvd_sweep_reduce_backward_workspace_bytes(B, C, h, w, V)
            call("mvd_sweep_reduce_backward_f32", dev, kf, srcs, Ms, dv, per_pixel, float(pix_offset), float(sx), float(sy), -0.5, mode,
                 groups, gout, B, C, D, h, w, V, gk, gs, workspace(wsb, dev), wsb)
        need = ctx.needs_input_grad
        return (None,) * 6 + (gk if need[6] else None,) + tuple(g if n else None for g, n in zip(gs, need[7:7 + V])) + (None,) * V


def sweep_reduce_autograd(key_feat, src_feats, Ms, depth, mode, groups=1, pix_offset=0.0, stretch=True):
    """Differentiable sweep_modes.sweep_reduce (same arguments, same forward bits): gradients to key_feat and src_feats through
    mvd_sweep_reduce_backward_f32; Ms and depth are constants.  Group correlation returns a list of V volumes."""
    srcs = views(src_feats, "src_feats")
    out = _SweepReduce.apply(depth, mode, groups, pix_offset, stretch, len(srcs), key_feat, *srcs, *views(Ms, "Ms", len(srcs)))
    return list(out) if mode == L.REDUCE_GROUPCORR else out


class _FuseViews(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n_views, *rest):
        V = n_views
        corrs, masks, scores = list(rest[:V]), list(rest[V:2 * V]), list(rest[2 * V:])
        fused, fmask = fuse_views([c.detach() for c in corrs], [m.detach() for m in masks], [s.detach() for s in scores])
        ctx.save_for_backward(*corrs, *masks, *scores)
        ctx.n_views = V
        ctx.mark_non_differentiable(fmask)
        return fused, fmask

    @staticmethod
    def backward(ctx, gfused, _gmask):
        V = ctx.n_views
        t = ctx.saved_tensors
        corrs, masks, scores = list(t[:V]), list(t[V:2 * V]), list(t[2 * V:])
        N, S, h, w = corrs[0].shape
        dev = corrs[0].device
        with torch.no_grad():
            cs = [L.as_f32(c, f"corrs[{i}]", (N, S, h, w), dev) for i, c in enumerate(corrs)]
            ms = [L.as_f32(m, f"masks[{i}]", (N, S, h, w), dev) for i, m in enumerate(masks)]
            ss = [L.as_f32(s, f"scores[{i}]", (N, 1, h, w), dev) for i, s in enumerate(scores)]
            g = gfused.float().contiguous()
            gcs = [torch.empty_like(cs[0]) for _ in range(V)]
            gss = [torch.empty_like(ss[0]) for _ in range(V)]
            call("mvd_fuse_views_backward_f32", dev, cs, ms, ss, g, N, S, h, w, V, gcs, gss)
        return (None,) + tuple(gcs) + (None,) * V + tuple(gss)


def fuse_views_autograd(corrs, masks, scores):
    """Differentiable K2: gradients to corrs and scores."""
    corrs = views(corrs, "corrs")
    V = len(corrs)
    return _FuseViews.apply(V, *corrs, *views(masks, "masks", V), *views(scores, "scores", V))


class _SoftmaxRegress(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, depth_values):
        c = L.as_f32(cost.detach(), "cost")
        if c.dim() != 4:
            raise ValueError("cost must be (B,D,h,w)")
        B, D, h, w = c.shape
        dv = L.as_f32(depth_values.detach(), "depth_values", (B, D), c.device)
        depth = torch.empty((B, h, w), dtype=torch.float32, device=c.device)
        conf = torch.empty((B, h, w), dtype=torch.float32, device=c.device)
        stats = torch.empty((B, 2, h, w), dtype=torch.float32, device=c.device)
        call("mvd_softmax_regress_stats_f32", c.device, c, dv, B, D, h, w, depth, conf, stats)
        ctx.save_for_backward(c, dv, depth, stats)
        ctx.mark_non_differentiable(conf)
        return depth, conf

    @staticmethod
    def backward(ctx, g_depth, _g_conf):
        c, dv, depth, stats = ctx.saved_tensors
        B, D, h, w = c.shape
        with torch.no_grad():
            g = g_depth.float().contiguous() if g_depth is not None else None
            g_cost = torch.empty_like(c)
            call("mvd_softmax_regress_backward_f32", c.device, c, dv, depth, stats, g, B, D, h, w, g_cost)
        return g_cost, None


def softmax_regress_autograd(cost, depth_values):
    """Differentiable K5: cost (B,D,h,w), depth_values (B,D) -> depth (B,h,w), confidence (B,h,w), depth bit-identical to
    softmax_regress's.  The gradient flows to the cost volume only (mvd_softmax_regress_backward_f32); the confidence is
    non-differentiable (the reference computes it under no_grad, mvsnet.py:143-160) and the depth samples are constants."""
    return _SoftmaxRegress.apply(cost, depth_values)


def conv3d_adjoint(weight, mode):
    """The layer whose FORWARD is the gradient of a CostRegNet layer w.r.t. its input: (weight, mode) -> (weight', mode').
    stride-1 conv W (Cout,Cin,3,3,3): a stride-1 conv with the taps flipped and the channel axes swapped, (Cin <- Cout);
    stride-2 conv W (Cout,Cin,...): a transposed conv whose weight (in = Cout, out = Cin) is W as it stands;
    transposed conv W (Cin,Cout,...): a stride-2 conv whose weight (out = Cin, in = Cout) is W as it stands.
    Plain tensor work on any device (include/mvd.h, "K4 for training")."""
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise ValueError(f"weight must be (*,*,3,3,3), got {tuple(weight.shape)}")
    if mode == L.CONV3D_STRIDE1:
        return weight.flip(2, 3, 4).transpose(0, 1).contiguous(), L.CONV3D_STRIDE1
    if mode == L.CONV3D_STRIDE2:
        return weight, L.DECONV3D_STRIDE2
    if mode == L.DECONV3D_STRIDE2:
        return weight, L.CONV3D_STRIDE2
    raise ValueError(f"mode {mode}")


_IDENTITY_EPILOGUE = {}


def _conv3d_plain(x, weight, mode):
    """One engine layer without epilogue (scale 1, shift 0, no ReLU, no skip); the weights are packed on every call."""
    packed, Cin, Cout = pack_conv3d_weights(weight, mode)
    key = (x.device, Cout)
    if key not in _IDENTITY_EPILOGUE:
        _IDENTITY_EPILOGUE[key] = (torch.ones(Cout, dtype=torch.float32, device=x.device),
                                   torch.zeros(Cout, dtype=torch.float32, device=x.device))
    scale, shift = _IDENTITY_EPILOGUE[key]
    return conv3d_bn_relu(x, packed, Cin, Cout, scale, shift, mode, relu=False)


# The layer kernels add every product of an output voxel into ONE fp32 accumulator, so their rounding error grows like the
# square root of the chain length.  27 taps x 8 channels is what the full-resolution layers have; longer reductions (the
# low-resolution layers with 16 .. 64 channels, a few per cent of the voxels) are cut into chains of at most that length.
_MAX_CHAIN = 27 * 8


def _conv3d_blocked(x, weight, mode):
    """_conv3d_plain with blocked accumulation: the reduction over (taps, Cin) is split along kd, then kh, then kw until no
    accumulator chain is longer than _MAX_CHAIN products; each part is the same layer with the other taps' weights zeroed
    (adding an exact zero product leaves the accumulator unchanged) and the parts are added in a fixed order.  Deterministic."""
    Cin, _ = _conv3d_channels(weight, mode)
    per_dim = 2 if mode == L.DECONV3D_STRIDE2 else 3  # taps that reach one output voxel, per dimension
    chain, level = per_dim ** 3 * Cin, 0
    while chain > _MAX_CHAIN and level < 3:
        chain //= per_dim
        level += 1
    if level == 0:
        return _conv3d_plain(x, weight, mode)
    out = None
    for idx in itertools.product(range(3), repeat=level):
        sel = (slice(None), slice(None)) + idx
        part = torch.zeros_like(weight)
        part[sel] = weight[sel]
        y = _conv3d_plain(x, part, mode)
        out = y if out is None else out.add_(y)
    return out


@inference_only
def conv3d_weight_grad(x, gy, mode):
    """x (B,Di,hi,wi,Cin) and gy (B,Do,ho,wo,Cout) channel-last -> the gradient of the layer's
    3x3x3 weight in its torch layout, (Cout,Cin,3,3,3) or (Cin,Cout,3,3,3) for DECONV3D_STRIDE2.  Deterministic."""
    x = L.as_f32(x, "x")
    if x.dim() != 5:
        raise ValueError(f"x must be (B,D,h,w,Cin) channel-last, got {tuple(x.shape)}")
    B, Di, hi, wi, Cin = x.shape
    osz = _conv3d_out_size(mode, Di, hi, wi)
    gy = L.as_f32(gy, "gy", device=x.device)
    if gy.dim() != 5 or tuple(gy.shape[:4]) != (B, *osz):
        raise ValueError(f"gy must be ({B},{osz[0]},{osz[1]},{osz[2]},Cout) channel-last, got {tuple(gy.shape)}")
    Cout = gy.shape[4]
    nbytes = L.load().mvd_conv3d_weight_grad_workspace_bytes(B, Di, hi, wi, Cin, Cout, mode)
    if nbytes == 0:
        raise ValueError(f"conv3d_weight_grad: Cin={Cin}, Cout={Cout} unsupported (1..64)")
    ws = workspace(nbytes, x.device)
    gw = torch.empty((Cin, Cout, 3, 3, 3) if mode == L.DECONV3D_STRIDE2 else (Cout, Cin, 3, 3, 3), dtype=torch.float32, device=x.device)
    call("mvd_conv3d_weight_grad_f32", x.device, x, gy, gw, B, Di, hi, wi, Cin, Cout, mode, ws, nbytes)
    return gw


class _Conv3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, mode):
        ctx.save_for_backward(x, weight)
        ctx.mode = mode
        return _conv3d_plain(x.detach(), weight.detach(), mode)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gx = gw = None
        with torch.no_grad():
            gy = gy.float().contiguous()
            if ctx.needs_input_grad[0]:
                gx = _conv3d_blocked(gy, *conv3d_adjoint(weight.detach(), ctx.mode))
            if ctx.needs_input_grad[1]:
                gw = conv3d_weight_grad(x.detach(), gy, ctx.mode)
        return gx, gw, None


def conv3d_autograd(x, weight, mode):
    """Differentiable K4 layer without epilogue: x (B,D,h,w,Cin) channel-last fp32, weight in the layer's torch layout
    ((Cout,Cin,3,3,3), or (Cin,Cout,3,3,3) for DECONV3D_STRIDE2) -> (B,Do,ho,wo,Cout).  Forward and the gradient w.r.t. x run on
    mvd_conv3d_bn_relu_f32 (the latter with conv3d_adjoint's weights and blocked accumulation, _conv3d_blocked), the gradient
    w.r.t. weight on mvd_conv3d_weight_grad_f32.  Nothing is converted: a silent .float() / .cuda() copy would detach the
    caller's tensor from its gradient."""
    x, weight = L.as_dtype(torch.float32, False, x, "x"), L.as_dtype(torch.float32, False, weight, "weight")
    if x.dim() != 5 or weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or x.shape[-1] != _conv3d_channels(weight, mode)[0]:
        raise ValueError(f"x {tuple(x.shape)} / weight {tuple(weight.shape)}: expected (B,D,h,w,Cin) and a 3x3x3 weight with Cin inputs")
    return _Conv3d.apply(x.contiguous(), weight.contiguous(), mode)


def needs_grad(*objs):
    return torch.is_grad_enabled() and any(t.requires_grad for t in _tensors(objs))
