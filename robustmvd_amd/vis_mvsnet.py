"""Vis-MVSNet (rmvd/models/vis_mvsnet.py:25-243, blocks/vis_mvsnet_singlestage.py, blocks/vis_mvsnet_unet_modular.py,
blocks/vis_mvsnet_feature_extractor.py, blocks/list_module.py) as a native model on the engine, inference only, with the reference's
protocol and state-dict keys (367 entries):

  FeatExt            vis_mvsnet_feature_extractor.py   5x5 stride-2 stem, a 2-D residual U-Net, three 3x3 heads at 1/8, 1/4, 1/2
                                                       resolution: stock torch.nn modules on the vendor library (follow-up: on
                                                       ops.conv2d_split, which lacks a 3x3 transposed layer, a residual before the
                                                       activation and a 1x1 layer with 16 inputs)
  SingleStage x 3    vis_mvsnet_singlestage.py:149-348 depth_num 64 / 32 / 16 at 1/8, 1/4, 1/2 resolution, intervals x 4 / 2 / 1:
    pair volumes     :86-122,242                       ops.sweep_groupcorr_nhwc, all V pairs into one (V B,D,h,w,8) buffer
    Reg / RegFuse    :21-54, unet_modular.py           nine fused 3-D layers on ops.conv3d_bn_relu, BN folded, the V pairs as one batch
    pair head        :245-260                          reg_pair (8 -> 1) -> ops.soft_argmin (depth, entropy) -> UncertNet (torch)
    fusion           :263-266,302-303                  ops.vis_fuse with head 0 as the uncertainty
    regression       :313-333                          RegFuse + 8 -> 1 -> ops.soft_argmin with window 2 (depth, probability map)
  between stages     vis_mvsnet.py:115-156             bilinear interpolation of the depth, minus half the next stage's range (torch)

Only what the reference's forward reaches is built: mode "soft", mem False, no upsampling, no refinement (vis_mvsnet.py:84-88,168).
One deliberate difference: the registry entry honours a `weights` file (the reference drops it, SURVEY.md bugs 1).

A residual block's relu(bn2(conv2) + residual) is the fused layer with relu=False and skip=residual (the kernel adds `skip` after
its activation, so with the activation off it is the sum) followed by an in-place ReLU: one extra pass over the block's output
(follow-up: a residual-before-ReLU epilogue in the 3-D convolution kernel)."""
import contextlib
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ops
from .blocks import Conv3dLayer, PackedWeights
from .models import _as_batch, _key_positions, _stack_views, _upscale_to_multiple
from .registry import build_model_with_cfg, register_model
from .sweep_modes import _vis_transform
from .utils import exclude_index, get_torch_model_device, select_by_index, to_numpy, to_torch

DEPTH_NUMS = (64, 32, 16)           # vis_mvsnet.py:84
INTERVAL_SCALES = (4.0, 2.0, 1.0)   # vis_mvsnet.py:85
S_SCALES = (8, 4, 2)                # vis_mvsnet.py:113,139,165
GROUPS = 8                          # vis_mvsnet_singlestage.py:242
WINDOW = 2.0                        # vis_mvsnet_singlestage.py:331
GRID_CLAMP = 1.1                    # blocks/utils.py:168: matters on maps narrower than 10 pixels (stage 1 of a 64-pixel image)


@contextlib.contextmanager
def _deterministic_convs():
    """The vendor library's convolutions (FeatExt, UncertNet) with its deterministic attribute set: some of its solvers accumulate with
    float atomics (measured: FeatExt's 64 -> 128 stride-2 level and its first transposed layer), and the same frame is to give the
    same bits.  Every other backend flag stays as the caller has it."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = prev


class ListModule(nn.Module):
    """list_module.py: children named by an OrderedDict's keys or a list's positions; a child that is itself a list becomes a nested
    ListModule.  (nn.ModuleList / nn.ModuleDict would give other state-dict keys for the nested lists.)"""

    def __init__(self, modules):
        super().__init__()
        items = modules.items() if isinstance(modules, OrderedDict) else enumerate(modules)
        for name, m in items:
            self.add_module(str(name), m if isinstance(m, nn.Module) else ListModule(m))

    def __getitem__(self, i):
        return list(self._modules.values())[i]

    def __iter__(self):
        return iter(self._modules.values())

    def __len__(self):
        return len(self._modules)


def _conv(dim, cin, cout, k, stride=1):
    return (nn.Conv2d if dim == 2 else nn.Conv3d)(cin, cout, k, stride, k // 2, bias=False)


def _bn(dim, c):
    return (nn.BatchNorm2d if dim == 2 else nn.BatchNorm3d)(c)


class BasicBlock(nn.Module):
    """vis_mvsnet_unet_modular.py:14-69: conv-bn-relu, conv-bn, + residual (through `downsample` where there is one), relu."""

    def __init__(self, cin, cout, stride, downsample, dim):
        super().__init__()
        self.conv1, self.bn1 = _conv(dim, cin, cout, 3, stride), _bn(dim, cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv2, self.bn2 = _conv(dim, cout, cout, 3), _bn(dim, cout)
        self.downsample = downsample

    def forward(self, x):
        out = self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x)))))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


def _make_layer(cin, cout, blocks, stride, dim):
    """vis_mvsnet_unet_modular.py:72-110: `blocks` BasicBlocks, the first with the stride and a 1x1 conv + BN shortcut where it changes
    the shape."""
    down = None
    if stride != 1 or cin != cout:
        down = nn.Sequential(_conv(dim, cin, cout, 1, stride), _bn(dim, cout))
    return nn.Sequential(BasicBlock(cin, cout, stride, down, dim), *[BasicBlock(cout, cout, 1, None, dim) for _ in range(1, blocks)])


class UNet(nn.Module):
    """vis_mvsnet_unet_modular.py:113-242 for the two configurations the model uses (no bottom and no head blocks, which leave
    empty ListModules without state-dict entries): encoder levels named <prefix><scale>_<index>, the first at stride 1 and the
    others at stride 2, then per decoder level [transposed 3x3 stride 2, 3x3 on the concatenation with the encoder level (, blocks)]."""

    def __init__(self, inplanes, enc, dec, initial_scale, filters, prefix, dim):
        super().__init__()
        deconv = nn.ConvTranspose2d if dim == 2 else nn.ConvTranspose3d
        scale, idx, prev = initial_scale, 0, inplanes
        self.bottom_blocks = ListModule([])
        levels = OrderedDict()
        for f in filters:
            levels[f"{prefix}{scale}_{idx}"] = _make_layer(prev, f, enc, 1 if idx == 0 else 2, dim)
            idx, scale, prev = idx + 1, scale * 2, f
        self.enc_blocks = ListModule(levels)
        levels = OrderedDict()
        for f in reversed(filters[:-1]):
            block = [deconv(prev, f, 3, 2, 1, 1, bias=False), _conv(dim, 2 * f, f, 3)]
            if dec > 0:
                block.append(_make_layer(f, f, dec, 1, dim))
            levels[f"{prefix}{scale}_{idx}"] = block
            idx, scale, prev = idx + 1, scale // 2, f
        self.dec_blocks = ListModule(levels)
        self.head_blocks = ListModule([])

    def forward(self, x):
        """-> every decoder scale, coarse first (the encoder's last output, then each decoder level's)."""
        enc = []
        for b in self.enc_blocks:
            x = b(x)
            enc.append(x)
        outs = [x]
        for i, b in enumerate(self.dec_blocks):
            x = b[1](torch.cat([b[0](x), enc[-2 - i]], 1))
            if len(b) == 3:
                x = b[2](x)
            outs.append(x)
        return outs


class FeatExt(nn.Module):
    """vis_mvsnet_feature_extractor.py:12-30 -> 32-channel features at 1/8, 1/4 and 1/2 resolution."""

    def __init__(self):
        super().__init__()
        self.init_conv = nn.Sequential(nn.Conv2d(3, 16, 5, 2, 2, bias=False), nn.BatchNorm2d(16), nn.ReLU())
        self.unet = UNet(16, 2, 1, 2, [32, 64, 128], "2d", 2)
        self.final_conv_1 = nn.Conv2d(128, 32, 3, 1, 1, bias=False)
        self.final_conv_2 = nn.Conv2d(64, 32, 3, 1, 1, bias=False)
        self.final_conv_3 = nn.Conv2d(32, 32, 3, 1, 1, bias=False)

    def forward(self, x):
        o1, o2, o3 = self.unet(self.init_conv(x))
        return self.final_conv_1(o1), self.final_conv_2(o2), self.final_conv_3(o3)


def center_tap_weight(w1):
    """A 1x1x1 convolution's weight (Cout,Cin,1,1,1) as the 3x3x3 weight that is zero but for its centre tap.  At stride 2 with
    padding 1 the centre tap of output o reads input 2 o, which is what the 1x1x1 stride-2 convolution reads: the two are equal."""
    w3 = w1.new_zeros((w1.shape[0], w1.shape[1], 3, 3, 3))
    w3[:, :, 1, 1, 1] = w1[:, :, 0, 0, 0]
    return w3


def split_concat_weight(w):
    """The weight (Cout, 2 f, 3,3,3) of a convolution over cat([a, b], 1) as the two weights of conv(a) + conv(b)."""
    f = w.shape[1] // 2
    return w[:, :f].contiguous(), w[:, f:].contiguous()


class Reg3d(PackedWeights, nn.Module):
    """The pair regulariser Reg and the fused one RegFuse (vis_mvsnet_singlestage.py:21-54): UNet(8, 1, 0, 4, [], [8, 16], [], prefix,
    dim=3), and RegFuse's final 8 -> 1 convolution.  forward is the reference's on torch (NCDHW); forward_channels_last runs the nine
    fused layers on ops.conv3d_bn_relu."""
    FOLDS_BN = "Vis-MVSNet's"

    def __init__(self, prefix, final):
        super().__init__()
        self.unet = UNet(8, 1, 0, 4, [8, 16], prefix, 3)
        if final:
            self.final_conv = nn.Conv3d(8, 1, 3, 1, 1, bias=False)

    def forward(self, x):
        out = self.unet(x)[-1]
        return self.final_conv(out) if hasattr(self, "final_conv") else out

    def _pack(self):
        b0, b1 = self.unet.enc_blocks[0][0], self.unet.enc_blocks[1][0]
        deconv, post = self.unet.dec_blocks[0][0], self.unet.dec_blocks[0][1]
        wa, wb = split_concat_weight(post.weight.detach())
        return {"b0c1": Conv3dLayer.pack(b0.conv1.weight, L.CONV3D_STRIDE1, bn=b0.bn1),
                "b0c2": Conv3dLayer.pack(b0.conv2.weight, L.CONV3D_STRIDE1, bn=b0.bn2),
                "b1c1": Conv3dLayer.pack(b1.conv1.weight, L.CONV3D_STRIDE2, bn=b1.bn1),
                "b1down": Conv3dLayer.pack(center_tap_weight(b1.downsample[0].weight.detach()), L.CONV3D_STRIDE2, bn=b1.downsample[1]),
                "b1c2": Conv3dLayer.pack(b1.conv2.weight, L.CONV3D_STRIDE1, bn=b1.bn2),
                "deconv": Conv3dLayer.pack(deconv.weight, L.DECONV3D_STRIDE2),
                "post_a": Conv3dLayer.pack(wa, L.CONV3D_STRIDE1),
                "post_b": Conv3dLayer.pack(wb, L.CONV3D_STRIDE1)}

    @ops.inference_only
    def forward_channels_last(self, x, mark=None):
        """x (B,D,h,w,8) channel-last, D, h, w even -> the U-Net's output (B,D,h,w,8) (without the final convolution)."""
        if x.dim() != 5 or x.shape[4] != 8 or x.shape[1] % 2 or x.shape[2] % 2 or x.shape[3] % 2:
            raise ValueError(f"the Vis-MVSNet regulariser needs (B,D,h,w,8) with even D, h, w, got {tuple(x.shape)}")
        pk = self._prepare()

        def relu_(t):
            t = torch.relu_(t)
            if mark is not None:
                mark("relu")
            return t

        e0 = relu_(pk["b0c2"](pk["b0c1"](x), relu=False, skip=x))
        e1 = relu_(pk["b1c2"](pk["b1c1"](e0), relu=False, skip=pk["b1down"](e0, relu=False)))
        up = pk["deconv"](e1, relu=False)
        return pk["post_b"](e0, relu=False, skip=pk["post_a"](up, relu=False))


class RegPair(nn.Module):
    """vis_mvsnet_singlestage.py:33-40."""

    def __init__(self):
        super().__init__()
        self.final_conv = nn.Conv3d(8, 1, 3, 1, 1, bias=False)

    def forward(self, x):
        return self.final_conv(x)


class UncertNet(nn.Module):
    """vis_mvsnet_singlestage.py:57-75: two 3x3 conv-bn-relu on the entropy map, plus the entropy map itself (broadcast over the 8
    channels), then one 3x3 head per output.  Stock torch modules."""

    def __init__(self, num_heads=1):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(1, 8, 3, 1, 1, bias=False), nn.BatchNorm2d(8), nn.ReLU())
        self.conv2 = nn.Sequential(nn.Conv2d(8, 8, 3, 1, 1, bias=False), nn.BatchNorm2d(8), nn.ReLU())
        self.head_convs = ListModule([nn.Conv2d(8, 1, 3, 1, 1, bias=False) for _ in range(num_heads)])

    def forward(self, x):
        out = self.conv2(self.conv1(x)) + x
        return [conv(out) for conv in self.head_convs]


def scale_camera(cam, scale):
    """blocks/utils.py:189-218: cam (B,2,4,4) [extrinsic; intrinsic] with the two focal lengths and the principal point times
    `scale`; every other entry, the skew included, as it is."""
    cam = cam.clone()
    for r, c in ((0, 0), (1, 1), (0, 2), (1, 2)):
        cam[:, 1, r, c] = cam[:, 1, r, c] * scale
    return cam


class SingleStage(PackedWeights, nn.Module):
    """vis_mvsnet_singlestage.py:78-348 on the engine (see the module's header)."""

    def __init__(self):
        super().__init__()
        self.reg = Reg3d("reg1", final=False)
        self.reg_fuse = Reg3d("reg2", final=True)
        self.reg_pair = RegPair()
        self.uncert_net = UncertNet(2)

    def _packed_from(self):
        return self.reg_pair.final_conv, self.reg_fuse.final_conv

    def _pack(self):
        """The two 8 -> 1 convolutions without BN: (reg_pair's, reg_fuse's)."""
        return [Conv3dLayer.pack(conv.weight, L.CONV3D_STRIDE1) for conv in self._packed_from()]

    @ops.inference_only
    def pair_scores(self, volumes, mark=None):
        """volumes (M,D,h,w,8) channel-last, the cost volumes of M pairs -> (interm (M,D,h,w,8), score (M,D,h,w)): Reg, reg_pair."""
        interm = self.reg.forward_channels_last(volumes, mark)
        return interm, self._prepare()[0](interm, relu=False).squeeze(-1)

    @ops.inference_only
    def fused_score(self, fused, mark=None):
        """fused (B,D,h,w,8) channel-last -> score (B,D,h,w): RegFuse."""
        out = self.reg_fuse.forward_channels_last(fused, mark)
        return self._prepare()[1](out, relu=False).squeeze(-1)

    @ops.inference_only
    def forward(self, key_feat, src_feats, ref_cam, srcs_cam, depth_num, depth_start, depth_interval, s_scale, mark=None):
        """key_feat (B,h,w,32) dense channel-last; src_feats V x (B,h+3,w+3,32) zero-bordered channel-last; ref_cam / srcs_cam[v]
        (B,2,4,4) [extrinsic; intrinsic] at full resolution; depth_start (B,1,1,1) or (B,1,h,w); depth_interval (B,1,1,1).
        Returns (est_depth (B,1,h,w), prob_map (B,1,h,w), [[pair_depth (B,1,h,w), [head0, head1]] per view])."""
        mark = mark or (lambda name: None)
        B, h, w, _ = key_feat.shape
        V = len(src_feats)
        dev = key_feat.device

        ref_s = scale_camera(ref_cam, 1 / s_scale)
        Ms = [_vis_transform(ref_s, scale_camera(c, 1 / s_scale), check_errors=False) for c in srcs_cam]  # no host synchronisation
        k = torch.arange(depth_num, dtype=torch.float32, device=dev).view(1, depth_num, 1, 1)
        depth = depth_start.float() + depth_interval.float() * k  # as sweep_modes.vis_cost_volumes forms it
        per_pixel = tuple(depth.shape[2:]) != (1, 1)
        depth = depth.expand(B, depth_num, h, w).contiguous() if per_pixel else depth.reshape(B, depth_num)
        volumes = torch.empty((V * B, depth_num, h, w, GROUPS), dtype=torch.float32, device=dev)
        ops.sweep_groupcorr_nhwc(key_feat, src_feats, Ms, depth, GROUPS, pix_offset=0.5, stretch=False, grid_clamp=GRID_CLAMP, out=volumes)
        mark("volume")
        interm, score = self.pair_scores(volumes, mark)
        del volumes
        mark("Reg")
        start = depth_start.float().reshape(B, -1)
        interval = depth_interval.float().reshape(B)
        pair_depth, ent, _ = ops.soft_argmin(score, start.repeat(V, 1), interval.repeat(V), with_entropy=True)
        del score
        mark("pair head")
        with _deterministic_convs():
            heads = self.uncert_net(ent.unsqueeze(1))
        mark("UncertNet")
        fused = ops.vis_fuse([interm[v * B:(v + 1) * B] for v in range(V)], [heads[0][v * B:(v + 1) * B] for v in range(V)])
        del interm
        mark("fusion")
        score = self.fused_score(fused, mark)
        del fused
        mark("RegFuse")
        est_depth, _, prob_map = ops.soft_argmin(score, start, interval, window=WINDOW)
        mark("regression")
        pairs = [[pair_depth[v * B:(v + 1) * B].unsqueeze(1), [hd[v * B:(v + 1) * B] for hd in heads]] for v in range(V)]
        return est_depth.unsqueeze(1), prob_map.unsqueeze(1), pairs


class VisMvsnet(nn.Module):
    def __init__(self, num_sampling_steps=192):
        super().__init__()
        self.feat_ext = FeatExt()
        self.stage1 = SingleStage()
        self.stage2 = SingleStage()
        self.stage3 = SingleStage()
        self.num_sampling_steps = num_sampling_steps
        self._bufs = {}
        self._mark = None  # measurement hook (tools/bench_vis_mvsnet.py): called with a part's name when the part has been enqueued

    def _frame_buffers(self, n, H, W, V, dev):
        """The feature maps in the sweep's layouts, allocated once per (n, H, W, V, device, stream) and reused: the source maps'
        borders must read zero, every forward overwrites everything else."""
        key = (n, H, W, V, str(dev), torch.cuda.current_stream(dev).cuda_stream)
        b = self._bufs.get(key)
        if b is None:
            if len(self._bufs) >= 8:  # shapes come and go: drop them all, but only once nothing in flight uses them
                torch.cuda.synchronize(dev)
                self._bufs.clear()
            z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
            b = self._bufs[key] = {"key": [z(n, H // s, W // s, 32) for s in S_SCALES],
                                   "src": [z(V * n, H // s + 3, W // s + 3, 32) for s in S_SCALES]}
        return b

    @ops.inference_only
    def forward(self, images, poses, intrinsics, keyview_idx, depth_range=None, **_):
        """images: list of (N,3,H,W), normalised as input_adapter does, H and W multiples of 16; poses (N,4,4) and intrinsics (N,3,3)
        per view; depth_range (min, max), scalars or (N,), default 0.2 .. 100.  Returns the reference's (pred, aux): pred depth and
        depth_uncertainty (N,1,H/2,W/2) (stage 3's, at half resolution, as the reference's); aux outputs (per stage [est_depth,
        [[pair_depth, [head0, head1]] per view]]), prob_maps ([x4 of stage 1's, x2 of stage 2's, stage 3's]) and ref_cam."""
        n, _, H, W = images[0].shape
        dev = images[0].device
        if H % 16 or W % 16:
            raise ValueError(f"vis_mvsnet needs H and W divisible by 16 (1/8 resolution and a stride-2 regulariser), got {H}x{W}")
        if len(images) < 2:
            raise ValueError("vis_mvsnet needs at least one source view")
        mark = self._mark or (lambda name: None)
        lo, hi = (0.2, 100.0) if depth_range is None else (depth_range[0], depth_range[1])
        as_n = lambda t: torch.as_tensor(t, dtype=torch.float32).to(dev, non_blocking=True).reshape(-1).expand(n)
        lo, hi = as_n(lo), as_n(hi)
        step = (hi - lo) / self.num_sampling_steps
        cams = []
        for K, P in zip(intrinsics, poses):  # vis_mvsnet.py:49-62
            cam = torch.zeros((n, 2, 4, 4), dtype=torch.float32, device=dev)
            cam[:, 0] = P.to(dev, torch.float32)
            cam[:, 1, :3, :3] = K.to(dev, torch.float32)
            cam[:, 1, 3, 0], cam[:, 1, 3, 1], cam[:, 1, 3, 2], cam[:, 1, 3, 3] = lo, step, float(self.num_sampling_steps), hi
            cams.append(cam)
        key_pos = _key_positions(keyview_idx, n)
        kidx = key_pos[0] if all(k == key_pos[0] for k in key_pos) else key_pos
        order = lambda xs: [select_by_index(xs, kidx)] + exclude_index(xs, kidx)
        views, cams = order(images), order(cams)
        ref_cam, srcs_cam = cams[0], cams[1:]
        V = len(srcs_cam)
        bufs = self._frame_buffers(n, H, W, V, dev)
        with _deterministic_convs():
            feats = self.feat_ext(_as_batch([v.float() for v in views]))  # key views first, then the source views, view-major
        for f, kb, sb in zip(feats, bufs["key"], bufs["src"]):
            h, w = f.shape[2], f.shape[3]
            kb.copy_(f[:n].permute(0, 2, 3, 1))
            sb[:, 1:h + 1, 1:w + 1, :].copy_(f[n:].permute(0, 2, 3, 1))
        del feats
        mark("FeatExt")
        depth_start = ref_cam[:, 1:2, 3:4, 0:1]     # n111
        depth_interval = ref_cam[:, 1:2, 3:4, 1:2]  # n111
        outputs, prob_maps, est = [], [], None
        for i, stage in enumerate((self.stage1, self.stage2, self.stage3)):
            kb, sb = bufs["key"][i], bufs["src"][i]
            interval = depth_interval * INTERVAL_SCALES[i]
            if est is None:
                start = depth_start
            else:  # vis_mvsnet.py:122-130,148-156
                start = F.interpolate(est, size=(kb.shape[1], kb.shape[2]), mode="bilinear", align_corners=False) \
                    - DEPTH_NUMS[i] * depth_interval * INTERVAL_SCALES[i] / 2
            mark("between stages")
            est, prob, pairs = stage(kb, [sb[v * n:(v + 1) * n] for v in range(V)], ref_cam, srcs_cam, DEPTH_NUMS[i], start, interval,
                                     S_SCALES[i], mark)
            outputs.append([est, pairs])
            prob_maps.append(prob)
        prob_maps = [F.interpolate(prob_maps[0], scale_factor=4, mode="bilinear", align_corners=False),
                     F.interpolate(prob_maps[1], scale_factor=2, mode="bilinear", align_corners=False), prob_maps[2]]
        mark("between stages")
        pred = {"depth": est, "depth_uncertainty": 1 - prob_maps[2]}
        return pred, {"outputs": outputs, "prob_maps": prob_maps, "ref_cam": ref_cam}

    def input_adapter(self, images, keyview_idx, poses=None, intrinsics=None, depth_range=None, **_):
        """vis_mvsnet.py:188-225 on the device: resize to the next multiple of 64, truncate to integers (its astype(np.uint8)), / 255,
        ImageNet mean / std, RGB -> BGR; default range 0.2 .. 100."""
        device = get_torch_model_device(self)
        images, intrinsics, _, _ = _upscale_to_multiple(images, intrinsics, 64, device)
        images = _stack_views(images, normalise_image)
        poses, intrinsics = to_torch((poses, intrinsics), device=device)
        keyview_idx = to_torch(keyview_idx)  # stays on the host: it only orders the views
        depth_range = (0.2, 100.0) if depth_range is None else depth_range
        depth_range = [torch.as_tensor(d, dtype=torch.float32) for d in depth_range]
        return {"images": images, "poses": [p.float() for p in poses], "intrinsics": [k.float() for k in intrinsics],
                "keyview_idx": keyview_idx, "depth_range": depth_range}

    def output_adapter(self, model_output):
        pred, aux = model_output
        return to_numpy(pred), to_numpy(aux)


IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def normalise_image(im):
    """(N,3,H,W) RGB in 0 .. 255 -> the model's input: truncated to an integer (astype(np.uint8)), / 255 (ToTensor), minus the
    ImageNet mean over its std per channel (Normalize), channels flipped to BGR (vis_mvsnet.py:204-210).  float32 throughout."""
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32, device=im.device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32, device=im.device).view(1, 3, 1, 1)
    c255 = torch.full((1,), 255.0, dtype=torch.float32, device=im.device)
    return ((im.float().trunc() / c255 - mean) / std).flip(1)


@register_model(trainable=False, listed=False)  # by name only: see register_model
def vis_mvsnet(pretrained=True, weights=None, train=False, num_gpus=1, **kwargs):
    """vis_mvsnet.py:232-242.  The reference's pretrained weights are a URL; offline pass a checkpoint {'model_state_dict': ...} with
    its state-dict keys via `weights` (honoured here; the reference ignores the argument), or load a state dict into the returned
    model.  With no file the model is untrained."""
    cfg = {"num_sampling_steps": 192}
    return build_model_with_cfg(model_cls=VisMvsnet, cfg=cfg, weights=weights, train=train, num_gpus=num_gpus, **kwargs)
