"""CVP-MVSNet (rmvd/models/cvp_mvsnet.py:36-321, blocks/cvp_mvsnet_components.py) as a native model on the engine, inference only
like the reference's (`register_model(trainable=False)`), with the reference's protocol and state-dict keys:

  FeaturePyramid     cvp_mvsnet_components.py:40-82    nine 3x3 Conv2d + bias + LeakyReLU(0.1) on ops.conv2d_split, five scales, all views
                                                       batched, channel-last; the last layer writes the key view dense and the source
                                                       views straight into zero-bordered maps
  coarse level       cvp_mvsnet.py:116-169             48 shared hypotheses -> ops.sweep_reduce_nhwc (KEYSQ) -> CVPCostRegNet -> K5
  refinement 3 .. 0  cvp_mvsnet.py:171-217             bicubic x2, depth_hypotheses (calDepthHypo's test-mode schedule), per-pixel
                                                       ops.sweep_reduce_nhwc (KEYSQ) -> CVPCostRegNet -> ops.softmax_regress_pp
  CVPCostRegNet      cvp_mvsnet_components.py:85-127   eleven fused 3-D layers on ops.conv3d_bn_relu (fp32 MFMA), BN folded

The cost volume is the one the reference computes, i.e. WITH its sum / sum-of-squares aliasing (REDUCE_VARIANCE_KEYSQ,
cvp_mvsnet.py:129-130, cvp_mvsnet_components.py:393-394): the model exists to match the reference.

Two deliberate differences from the reference, both because the reference's own model cannot be run through run():
  * its input_adapter emits min_depth / max_depth while its forward demands depth_range (cvp_mvsnet.py:51,293-300); here the adapter
    passes depth_range and forward receives it;
  * its coarse hypotheses are torch.range(min, max, (max - min) / 47), whose COUNT depends on rounding: 48 for e.g. 2 .. 10 or
    425 .. 935, but 47 for its default 0.2 .. 100, which its stride-2 regulariser then refuses.  Here the count is fixed at 48 (see
    coarse_hypotheses): bit-identical values where the reference yields 48, and a working model where it yields 47.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ops
from .blocks import Conv3dLayer, ConvBnReLU3D, PackedWeights, Slots, _deconv_block
from .models import _as_batch, _key_positions, _stack_views, _upscale_to_multiple
from .registry import build_model_with_cfg, register_model
from .sweep_modes import _cvp_transform
from .utils import exclude_index, get_torch_model_device, select_by_index, to_numpy, to_torch

NUM_COARSE = 48   # nhypothesis_init, cvp_mvsnet_components.py:163
NUM_REFINE = 8    # 2 d with d = 4, cvp_mvsnet_components.py:262,287
NUM_SCALES = 5    # args.nscale, cvp_mvsnet.py:44


def coarse_hypotheses(min_depth, max_depth, device=None):
    """calSweepingDepthHypo (cvp_mvsnet_components.py:162-189) for one range -> (48,) float32: torch.range's values, start + k * step
    in double rounded to float32, with the float32 step (max - min) / 47 the reference computes.  The count is fixed at 48:
    torch.range derives it as floor((max - min) / step + 1) in double, which is 48 for most ranges but 47 when the float32 step
    rounds up (the reference's default 0.2 .. 100 does): where the reference yields 48 these are its values to the bit, where it yields
    47 it cannot run at all (its regulariser needs an even count) and this model still works.  min_depth / max_depth: python
    numbers, arrays or tensors (element 0 is used, as the reference uses batch element 0's range for all); computed on `device`
    without host synchronisation when they already live there."""
    lo = torch.as_tensor(min_depth, dtype=torch.float32, device=device).reshape(-1)[0]
    hi = torch.as_tensor(max_depth, dtype=torch.float32, device=device).reshape(-1)[0]
    step = (hi - lo) / (NUM_COARSE - 1)  # float32, cvp_mvsnet_components.py:167-168
    k = torch.arange(NUM_COARSE, dtype=torch.float64, device=lo.device)
    return (lo.double() + k * step.double()).float()


def depth_hypotheses(depth_up, ref_in, src_in, ref_ex, src_ex):
    """calDepthHypo's test-mode schedule (cvp_mvsnet_components.py:279-372): depth_up (B,h,w) float32, the upsampled depth of the level
    below; ref_in / src_in (B,3,3) the level's intrinsics of the key view and of source view 0 (the reference uses source 0 only);
    ref_ex / src_ex (B,4,4) -> (B,8,h,w) float32 hypotheses depth_up + l * interval_b, l = -4 .. 3.

    What it computes, per batch element, in float64: every key pixel is lifted to its depth D and to D + 1, both points are
    projected into the source view, and the direction of that image segment is the pixel's epipolar direction.  The point one pixel
    further along it, p3, is mapped back by the infinite homography A = K_r R_r (K_s R_s)^-1, and the key-view depth `a` at which
    the key pixel's ray meets p3's ray solves, in the rows y and z of  a (x, y, 1)^T + c A p3 = z1 A p1:
        a y + c (A p3)_y = z1 (A p1)_y,   a + c (A p3)_z = z1 (A p1)_z.
    interval_b = mean over the pixels of |a|.  Pure torch on the inputs' device, vectorised over pixels and batch, no host round trip.
    A key / source pair related by a pure translation along x makes the 2x2 systems singular (the reference's torch.inverse raises
    there; here the interval becomes inf / NaN)."""
    B, h, w = depth_up.shape
    dev, f64 = depth_up.device, torch.float64
    Kr, Ks, Er, Es = ref_in.to(f64), src_in.to(f64), ref_ex.to(f64), src_ex.to(f64)
    inv = lambda m: torch.linalg.inv_ex(m, check_errors=False).inverse
    ys, xs = torch.meshgrid(torch.arange(h, dtype=f64, device=dev), torch.arange(w, dtype=f64, device=dev), indexing="ij")
    pix = torch.stack((xs.reshape(-1), ys.reshape(-1), torch.ones(h * w, dtype=f64, device=dev)), 0)[None]  # (1,3,P)
    d1 = depth_up.reshape(B, 1, h * w)  # float32, like the reference's D1 (D2 = D1 + 1 is a float32 sum there too)
    T = Es @ inv(Er)       # key camera -> source camera
    Kr_inv = inv(Kr)

    def project(d):
        cam = T[:, :3, :3] @ (Kr_inv @ (pix * d)) + T[:, :3, 3:4]
        p = Ks @ cam
        z = p[:, 2:3]
        return p / z, z

    p1, z1 = project(d1.to(f64))
    p2, _ = project((d1 + 1).to(f64))
    theta = torch.atan((p2[:, 1] - p1[:, 1]) / (p2[:, 0] - p1[:, 0]))
    p3 = p1 + torch.stack((torch.cos(theta), torch.sin(theta), torch.zeros_like(theta)), 1)
    A = (Kr @ Er[:, :3, :3]) @ inv(Ks @ Es[:, :3, :3])
    t1, t2 = z1 * (A @ p1), A @ p3
    y = pix[:, 1]
    a = (t1[:, 1] * t2[:, 2] - t2[:, 1] * t1[:, 2]) / (y * t2[:, 2] - t2[:, 1])  # Cramer's rule on the 2x2 system
    interval = a.abs().mean(dim=1).view(B, 1, 1, 1)
    lvl = torch.arange(-NUM_REFINE // 2, NUM_REFINE // 2, dtype=f64, device=dev).view(1, NUM_REFINE, 1, 1)
    return (depth_up.to(f64).unsqueeze(1) + lvl * interval).float()  # float64 inside, one rounding out (:362-371)


def _conv_leaky(cin, cout):
    return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, bias=True), nn.LeakyReLU(0.1))


class FeaturePyramid(PackedWeights, nn.Module):
    """cvp_mvsnet_components.py:40-82.  Parameters live in the reference's nn.Sequential(Conv2d, LeakyReLU) blocks (its checkpoints
    load); forward_levels runs the nine layers of every scale on the split-operand kernel, channel-last."""
    LAYERS = [("conv0aa", 3, 64), ("conv0ba", 64, 64), ("conv0bb", 64, 64), ("conv0bc", 64, 32), ("conv0bd", 32, 32),
              ("conv0be", 32, 32), ("conv0bf", 32, 16), ("conv0bg", 16, 16), ("conv0bh", 16, 16)]

    def __init__(self):
        super().__init__()
        for name, cin, cout in self.LAYERS:
            setattr(self, name, _conv_leaky(cin, cout))

    def _pack(self):
        return [ops.pack_conv2d_weights_split(getattr(self, name)[0].weight.detach(), getattr(self, name)[0].bias,
                                              cin_pad=(cin + 7) // 8 * 8) for name, cin, _ in self.LAYERS]

    @ops.inference_only
    def forward_levels(self, images, n_key, image_bufs, src_bufs):
        """images (M,3,H,W), the key views first (n_key of them), then the source views; image_bufs[s] (M,H/2^s,W/2^s,8) whose
        channels 3 .. 7 read zero; src_bufs[s] (M - n_key, h+3, w+3, 16) whose border reads zero.  Returns the key features per scale,
        (n_key,h,w,16) dense channel-last; the source features are written into the interior of src_bufs[s]."""
        wts = self._prepare()
        slots = Slots(len(image_bufs) * len(wts), images.device)  # one fill for all scales
        keys = []
        img = images
        for s, (ibuf, sbuf) in enumerate(zip(image_bufs, src_bufs)):
            if s > 0:  # cvp_mvsnet_components.py:67-69
                img = F.interpolate(img, scale_factor=0.5, mode="bilinear", align_corners=None)
            ibuf[..., :3].copy_(img.permute(0, 2, 3, 1))
            x, a = ibuf, ops.absmax(img)
            for wt in wts[:-1]:
                a_out = slots.take()
                x = ops.conv2d_split(x, a, wt, act=1, slope=0.1, out_absmax=a_out)
                a = a_out
            h, w = x.shape[1], x.shape[2]
            keys.append(ops.conv2d_split(x[:n_key], a, wts[-1], act=1, slope=0.1))
            ops.conv2d_split(x[n_key:], a, wts[-1], act=1, slope=0.1, out=sbuf[:, 1:h + 1, 1:w + 1, :])
        return keys


class CVPCostRegNet(PackedWeights, nn.Module):
    """cvp_mvsnet_components.py:85-127, the reference's parameter names; forward_channels_last folds BN (eval mode) and runs the
    eleven layers on ops.conv3d_bn_relu, channel-last.  conv5 is a STRIDE-1 ConvTranspose3d: packed once as the stride-1 convolution
    it equals (taps flipped, channel axes swapped).  The two skip additions follow the ReLU, which is what the kernel's `skip` does."""
    FOLDS_BN = "CVPCostRegNet"
    CONVS = [("conv0", 16, 16, 1), ("conv0a", 16, 16, 1), ("conv1", 16, 32, 2), ("conv2", 32, 32, 1), ("conv2a", 32, 32, 1),
             ("conv3", 32, 64, 1), ("conv4", 64, 64, 1), ("conv4a", 64, 64, 1)]

    def __init__(self):
        super().__init__()
        for name, cin, cout, stride in self.CONVS:
            setattr(self, name, ConvBnReLU3D(cin, cout, stride=stride))
        self.conv5 = nn.Sequential(nn.ConvTranspose3d(64, 32, kernel_size=3, padding=1, output_padding=0, stride=1, bias=False),
                                   nn.BatchNorm3d(32), nn.ReLU(inplace=True))
        self.conv6 = _deconv_block(32, 16)
        self.prob0 = nn.Conv3d(16, 1, 3, stride=1, padding=1)

    def _pack(self):
        pk = {}
        for name, _, _, stride in self.CONVS:
            m = getattr(self, name)
            pk[name] = Conv3dLayer.pack(m.conv.weight, L.CONV3D_STRIDE1 if stride == 1 else L.CONV3D_STRIDE2, bn=m.bn)
        w5 = self.conv5[0].weight.detach().flip(2, 3, 4).transpose(0, 1).contiguous()  # (Cin,Cout,k,k,k) deconv -> (Cout,Cin,k,k,k) conv
        pk["conv5"] = Conv3dLayer.pack(w5, L.CONV3D_STRIDE1, bn=self.conv5[1])
        pk["conv6"] = Conv3dLayer.pack(self.conv6[0].weight, L.DECONV3D_STRIDE2, bn=self.conv6[1])
        pk["prob0"] = Conv3dLayer.pack(self.prob0.weight, L.CONV3D_STRIDE1, bias=self.prob0.bias)
        return pk

    @ops.inference_only
    def forward_channels_last(self, x):
        """x (B,D,h,w,16) channel-last -> cost (B,D,h,w)."""
        if x.dim() != 5 or x.shape[4] != 16 or x.shape[1] % 2 or x.shape[2] % 2 or x.shape[3] % 2:
            raise ValueError(f"CVPCostRegNet needs (B,D,h,w,16) with even D, h, w, got {tuple(x.shape)}")
        pk = self._prepare()
        conv0 = pk["conv0a"](pk["conv0"](x))
        conv2 = pk["conv2a"](pk["conv2"](pk["conv1"](conv0)))
        conv4 = pk["conv4a"](pk["conv4"](pk["conv3"](conv2)))
        conv5 = pk["conv5"](conv4, skip=conv2)
        conv6 = pk["conv6"](conv5, skip=conv0)
        return pk["prob0"](conv6, relu=False).squeeze(-1)

    def forward(self, x):
        """Reference layout: (B,16,D,h,w) -> (B,D,h,w)."""
        return self.forward_channels_last(ops.to_channels_last_3d(x))


class CVPMVSNet(nn.Module):
    def __init__(self, num_sampling_steps=192):
        super().__init__()
        self.featurePyramid = FeaturePyramid()
        self.cost_reg_refine = CVPCostRegNet()
        self.num_sampling_steps = num_sampling_steps  # kept for the reference's constructor; the schedule has fixed counts
        self._bufs = {}
        self._mark = None  # measurement hook (tools/bench_cvp_mvsnet.py): called with a stage's name when the stage has been enqueued

    def _frame_buffers(self, n, H, W, V, dev):
        """The buffers whose pad channels / borders must read zero, allocated once per (n, H, W, V, device, stream) and reused: every
        forward overwrites everything else in them."""
        key = (n, H, W, V, str(dev), torch.cuda.current_stream(dev).cuda_stream)
        b = self._bufs.get(key)
        if b is None:
            if len(self._bufs) >= 8:  # shapes come and go: drop them all, but only once nothing in flight uses them
                torch.cuda.synchronize(dev)
                self._bufs.clear()
            z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
            b = self._bufs[key] = {
                "image": [z((V + 1) * n, H >> s, W >> s, 8) for s in range(NUM_SCALES)],
                "src": [z(V * n, (H >> s) + 3, (W >> s) + 3, 16) for s in range(NUM_SCALES)]}
        return b

    @ops.inference_only
    def forward(self, images, poses, intrinsics, keyview_idx, depth_range=None, **_):
        """images: list of (N,3,H,W) in 0..1, H and W multiples of 32; poses (N,4,4) and intrinsics (N,3,3) per view;
        depth_range: (min, max), element 0 of each is used for the whole batch (as the reference does), default 0.2 .. 100.
        Returns ({"depth": (N,1,H,W), "depth_uncertainty": (N,1,H,W)}, {"depths_all": the five levels' (N,h,w) maps, finest first})."""
        n, _, H, W = images[0].shape
        dev = images[0].device
        if H % 32 or W % 32:
            raise ValueError(f"cvp_mvsnet needs H and W divisible by 32 (five scales and a stride-2 regulariser), got {H}x{W}")
        if len(images) < 2:
            raise ValueError("cvp_mvsnet needs at least one source view")
        key_pos = _key_positions(keyview_idx, n)
        kidx = key_pos[0] if all(k == key_pos[0] for k in key_pos) else key_pos
        order = lambda xs: [select_by_index(xs, kidx)] + exclude_index(xs, kidx)
        views = order(images)
        Ks = [k.to(dev, torch.float32) for k in order(intrinsics)]
        Es = [p.to(dev, torch.float32) for p in order(poses)]
        V = len(views) - 1
        bufs = self._frame_buffers(n, H, W, V, dev)
        mark = self._mark or (lambda name: None)
        keys = self.featurePyramid.forward_levels(_as_batch([v.float() for v in views]), n, bufs["image"], bufs["src"])
        mark("pyramid")

        def level_inputs(level):
            # conditionIntrinsics (cvp_mvsnet_components.py:144-159): rows 0 and 1 divided by the level's down ratio
            Kl = [torch.cat((k[:, :2] / float(1 << level), k[:, 2:]), 1) for k in Ks]
            Ms = [_cvp_transform(Kl[0], Kl[v], Es[0], Es[v], check_errors=False) for v in range(1, V + 1)]  # no host synchronisation
            srcs = [bufs["src"][level][(v - 1) * n:v * n] for v in range(1, V + 1)]
            return Kl, Ms, srcs

        lo, hi = (0.2, 100.0) if depth_range is None else (depth_range[0], depth_range[1])
        on_dev = lambda t: t.to(dev, non_blocking=True) if isinstance(t, torch.Tensor) else t
        hyp = coarse_hypotheses(on_dev(lo), on_dev(hi), device=dev).expand(n, NUM_COARSE).contiguous()
        level = NUM_SCALES - 1
        _, Ms, srcs = level_inputs(level)
        mark("schedule 4")
        vol = ops.sweep_reduce_nhwc(keys[level], srcs, Ms, hyp, L.REDUCE_VARIANCE_KEYSQ)
        mark("volume 4")
        cost = self.cost_reg_refine.forward_channels_last(vol)
        del vol
        mark("regulariser 4")
        depth, _ = ops.softmax_regress(cost, hyp, with_confidence=False)
        mark("regression 4")
        depths, conf = [depth], None
        for level in range(NUM_SCALES - 2, -1, -1):
            depth_up = F.interpolate(depth[None], scale_factor=2, mode="bicubic", align_corners=None)[0]
            Kl, Ms, srcs = level_inputs(level)
            hyp = depth_hypotheses(depth_up, Kl[0], Kl[1], Es[0], Es[1])
            mark(f"schedule {level}")
            vol = ops.sweep_reduce_nhwc(keys[level], srcs, Ms, hyp, L.REDUCE_VARIANCE_KEYSQ)
            mark(f"volume {level}")
            cost = self.cost_reg_refine.forward_channels_last(vol)
            del vol
            mark(f"regulariser {level}")
            depth, conf = ops.softmax_regress_pp(cost, hyp, with_confidence=level == 0)
            mark(f"regression {level}")
            depths.append(depth)
        depths.reverse()
        pred = {"depth": depth.unsqueeze(1), "depth_uncertainty": (1 - conf).unsqueeze(1)}
        return pred, {"depths_all": depths}

    def input_adapter(self, images, keyview_idx, poses=None, intrinsics=None, depth_range=None, **_):
        """cvp_mvsnet.py:257-301 on the device: resize to the next multiple of 64, images / 255, default range 0.2 .. 100 — and the
        range is handed on as `depth_range`, the name forward takes (the reference emits min_depth / max_depth, which its forward
        never receives)."""
        device = get_torch_model_device(self)
        images, intrinsics, _, _ = _upscale_to_multiple(images, intrinsics, 64, device)
        c255 = torch.full((1,), 255.0, dtype=torch.float32, device=device)
        images = _stack_views(images, lambda im: im.float() / c255)
        poses, intrinsics = to_torch((poses, intrinsics), device=device)
        keyview_idx = to_torch(keyview_idx)  # stays on the host: it only orders the views
        depth_range = (0.2, 100.0) if depth_range is None else depth_range
        depth_range = [torch.as_tensor(d, dtype=torch.float32) for d in depth_range]
        return {"images": images, "poses": [p.float() for p in poses], "intrinsics": [k.float() for k in intrinsics],
                "keyview_idx": keyview_idx, "depth_range": depth_range}

    def output_adapter(self, model_output):
        pred, aux = model_output
        return to_numpy(pred), to_numpy(aux)


@register_model(trainable=False, listed=False)  # by name only: see register_model
def cvp_mvsnet(pretrained=True, weights=None, train=False, num_gpus=1, **kwargs):
    """cvp_mvsnet.py:308-321.  The reference ships no weights for this model (weights=None there); pass a checkpoint
    {'model_state_dict': ...} with its state-dict keys via `weights`, or load a state dict into the returned model."""
    cfg = {"num_sampling_steps": 192}
    return build_model_with_cfg(model_cls=CVPMVSNet, cfg=cfg, weights=weights, train=train, num_gpus=num_gpus, **kwargs)
