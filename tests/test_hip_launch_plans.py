"""Which C entry points a model configuration launches, in which order and with which integer arguments: CostRegNet, FeatureNet and
RobustMVD's engine, every configuration that takes another path through their forward.  The expected lists were recorded from the
commit before the model layers got their shared packed-weight cache, layer records and slot allocator (ops.call wrapped as here, a
second forward, on an MI355X), and written down literally: an edit of these forwards that adds, drops, reorders or re-routes a launch
fails here even where the outputs still agree."""
import pytest
import torch

import gen_common as gc

pytestmark = pytest.mark.gpu

ABSMAX = "mvd_absmax_f32"
K4, K4_F16IN, K4_SPLIT = "mvd_conv3d_bn_relu_f32", "mvd_conv3d_bn_relu_f16in", "mvd_conv3d_bn_relu_f32_split"
K4_IGEMM, K4_DSPLIT = "mvd_conv3d_bn_relu_igemm_f32", "mvd_deconv3d_bn_relu_f32_split"
K6, C2S, ZERO_BORDER = "mvd_conv2d_bn_relu_f32", "mvd_conv2d_split_f32", "mvd_zero_border_nhwc_f32"
HEAD, HEAD_SPLIT = "mvd_conv2d_head_f32", "mvd_conv2d_head_split_f32"
SWEEP, FUSE, UP2, DISP_HEAD = "mvd_sweep_corr_nhwc_f32", "mvd_fuse_views_nhwc_f32", "mvd_upsample2x_nhwc_f32", "mvd_dispnet_head_f32"

# ---- CostRegNet.forward_channels_last at (1, 16, 16, 24, 32)
REG_IGEMM = [(K4_IGEMM, (1, 16, 16, 24, 8, 16, 1, 1, 0)), (K4_IGEMM, (1, 8, 8, 12, 16, 16, 0, 1, 98304)),
             (K4_IGEMM, (1, 8, 8, 12, 16, 32, 1, 1, 24576)), (K4_IGEMM, (1, 4, 4, 6, 32, 32, 0, 1, 0)),
             (K4_IGEMM, (1, 4, 4, 6, 32, 64, 1, 1, 12288)), (K4_IGEMM, (1, 2, 2, 3, 64, 64, 0, 1, 6144))]
REG_DSPLIT = [(K4_DSPLIT, (1, 2, 2, 3, 64, 32, 1)), (K4_DSPLIT, (1, 4, 4, 6, 32, 16, 1)), (K4_DSPLIT, (1, 8, 8, 12, 16, 8, 1))]
REG_UPS_FP32 = [(K4, (1, 2, 2, 3, 64, 32, 2, 1)), (K4, (1, 4, 4, 6, 32, 16, 2, 1)), (K4, (1, 8, 8, 12, 16, 8, 2, 1))]
REG_PROB = (K4, (1, 16, 16, 24, 8, 1, 0, 0))
REG_DEFAULT = [(ABSMAX, (196608,)), (K4_SPLIT, (1, 16, 16, 24, 32, 8, 1)), *REG_IGEMM, *REG_DSPLIT, REG_PROB]
REG_PLANS = {
    "default": REG_DEFAULT,
    "x_absmax": REG_DEFAULT[1:],
    "f16": [(K4_F16IN, (1, 16, 16, 24, 32, 8, 1)), (ABSMAX, (49152,)), *REG_IGEMM, *REG_UPS_FP32, REG_PROB],
    "no_split": [(K4, (1, 16, 16, 24, 32, 8, 0, 1)), (K4, (1, 16, 16, 24, 8, 16, 1, 1)), (K4, (1, 8, 8, 12, 16, 16, 0, 1)),
                 (K4, (1, 8, 8, 12, 16, 32, 1, 1)), (K4, (1, 4, 4, 6, 32, 32, 0, 1)), (K4, (1, 4, 4, 6, 32, 64, 1, 1)),
                 (K4, (1, 2, 2, 3, 64, 64, 0, 1)), *REG_UPS_FP32, REG_PROB],
}

# ---- FeatureNet.forward_layout at (2, 3, 32, 48)
FEAT_HEAD_SPLIT = [(HEAD_SPLIT, (2, 32, 48)), (ABSMAX, (8,))]
FEAT_HEAD_K6 = [(K6, (0, 1, 2, 32, 48, 3, 8, 3, 1, 1)), (K6, (1, 1, 2, 32, 48, 8, 8, 3, 1, 1))]
FEAT_SPLIT = [(C2S, (2, 32, 48, 8, 8, 16, 16, 384, 6144, 1, 5, 5, 2, 0, 2, 0)), (C2S, (2, 16, 24, 16, 16, 16, 16, 384, 6144, 1, 3, 3, 1, 0, 2, 0)),
              (C2S, (2, 16, 24, 16, 16, 16, 16, 384, 6144, 1, 3, 3, 1, 0, 2, 0)), (C2S, (2, 16, 24, 16, 16, 32, 32, 384, 3072, 1, 5, 5, 2, 0, 2, 0)),
              (C2S, (2, 8, 12, 32, 32, 32, 32, 384, 3072, 1, 3, 3, 1, 0, 2, 0))]
FEAT_BORDER = [(ZERO_BORDER, (2, 8, 12, 32)), (C2S, (2, 8, 12, 32, 32, 32, 32, 480, 5280, 1, 3, 3, 1, 0, 0, 0))]
FEAT_PLANS = {
    "nchw_absmax": [*FEAT_HEAD_SPLIT, *FEAT_SPLIT, (C2S, (2, 8, 12, 32, 32, 32, 1, 12, 3072, 96, 3, 3, 1, 0, 0, 0)), (ABSMAX, (6144,))],
    "nhwc": [*FEAT_HEAD_SPLIT, *FEAT_SPLIT, (C2S, (2, 8, 12, 32, 32, 32, 32, 384, 3072, 1, 3, 3, 1, 0, 0, 0))],
    "border": [*FEAT_HEAD_SPLIT, *FEAT_SPLIT, *FEAT_BORDER],
    "no_split_layers": [*FEAT_HEAD_K6, (K6, (1, 1, 2, 32, 48, 8, 16, 5, 2, 1)), (K6, (1, 1, 2, 16, 24, 16, 16, 3, 1, 1)),
                        (K6, (1, 1, 2, 16, 24, 16, 16, 3, 1, 1)), (K6, (1, 1, 2, 16, 24, 16, 32, 5, 2, 1)), (K6, (1, 1, 2, 8, 12, 32, 32, 3, 1, 1)),
                        (K6, (1, 2, 2, 8, 12, 32, 32, 3, 1, 0)), (ABSMAX, (10560,))],
    "unfused_head": [*FEAT_HEAD_K6, (ABSMAX, (24576,)), *FEAT_SPLIT, *FEAT_BORDER],
    "fp32_head": [(HEAD, (2, 32, 48)), (ABSMAX, (8,)), *FEAT_SPLIT, *FEAT_BORDER],
}

# ---- RobustMVD through its engine at 64 x 128
RMVD_KEY = [(ABSMAX, (24576,)), (C2S, (1, 64, 128, 8, 0, 64, 104, 6656, 212992, 1, 7, 7, 2, 2, 1, 0)),
            (C2S, (1, 32, 64, 64, 104, 128, 200, 6400, 102400, 1, 5, 5, 2, 0, 1, 1048576)),
            (C2S, (1, 16, 32, 128, 200, 256, 256, 4096, 32768, 1, 3, 3, 2, 0, 1, 1048576)),
            (C2S, (1, 8, 16, 256, 256, 32, 288, 4608, 36864, 1, 1, 1, 1, 0, 1, 65536))]
RMVD_SOURCES_V2 = [(ABSMAX, (49152,)), (C2S, (2, 64, 128, 8, 0, 64, 64, 4096, 131072, 1, 7, 7, 2, 2, 1, 0)),
                   (C2S, (2, 32, 64, 64, 64, 128, 128, 4096, 65536, 1, 5, 5, 2, 0, 1, 2097152)),
                   (C2S, (2, 16, 32, 128, 128, 256, 256, 4864, 53504, 1, 3, 3, 2, 0, 1, 2097152))]
RMVD_FUSION_V2 = [(SWEEP, (0, 1, 256, 8, 16, 8, 16, 256, 2, 256)), (C2S, (2, 8, 16, 256, 256, 128, 128, 2048, 16384, 1, 3, 3, 1, 0, 2, 524288)),
                  (C2S, (2, 8, 16, 128, 128, 1, 1, 16, 128, 1, 1, 1, 1, 0, 0, 32768)), (FUSE, (1, 256, 8, 16, 2, 256, 288))]
RMVD_SOURCES_V1 = [(ABSMAX, (24576,)), (C2S, (1, 64, 128, 8, 0, 64, 64, 4096, 131072, 1, 7, 7, 2, 2, 1, 0)),
                   (C2S, (1, 32, 64, 64, 64, 128, 128, 4096, 65536, 1, 5, 5, 2, 0, 1, 1048576)),
                   (C2S, (1, 16, 32, 128, 128, 256, 256, 4864, 38912, 1, 3, 3, 2, 0, 1, 1048576))]
RMVD_FUSION_V1 = [(SWEEP, (0, 1, 256, 8, 16, 8, 16, 256, 1, 288))]
RMVD_REST = [  # cost-volume encoder, then per decoder level: head, (deconv, upsampled prediction, rfeat)
    (C2S, (1, 8, 16, 288, 288, 256, 392, 6272, 50176, 1, 3, 3, 1, 0, 1, 524288)),
    (C2S, (1, 8, 16, 256, 392, 512, 512, 4096, 16384, 1, 3, 3, 2, 0, 1, 1048576)),
    (C2S, (1, 4, 8, 512, 512, 512, 776, 6208, 24832, 1, 3, 3, 1, 0, 1, 524288)),
    (C2S, (1, 4, 8, 512, 776, 512, 512, 2048, 4096, 1, 3, 3, 2, 0, 1, 524288)),
    (C2S, (1, 2, 4, 512, 512, 512, 1032, 4128, 8256, 1, 3, 3, 1, 0, 1, 131072)),
    (C2S, (1, 2, 4, 512, 1032, 1024, 1024, 2048, 2048, 1, 3, 3, 2, 0, 1, 262144)),
    (C2S, (1, 1, 2, 1024, 1024, 1024, 1024, 2048, 2048, 1, 3, 3, 1, 0, 1, 131072)),
    (C2S, (1, 1, 2, 1024, 1024, 2, 1, 2, 4, 2, 3, 3, 1, 0, 0, 2048)), (DISP_HEAD, (1, 2)),
    (C2S, (1, 1, 2, 1024, 1024, 512, 1032, 4128, 8256, 1, 4, 4, 2, 1, 1, 262144)), (UP2, (1, 2, 1, 2, 1032)),
    (C2S, (1, 2, 4, 1032, 1032, 512, 512, 2048, 4096, 1, 3, 3, 1, 0, 1, 524288)),
    (C2S, (1, 2, 4, 512, 512, 2, 1, 4, 16, 8, 3, 3, 1, 0, 0, 4096)), (DISP_HEAD, (1, 8)),
    (C2S, (1, 2, 4, 512, 512, 256, 776, 6208, 24832, 1, 4, 4, 2, 1, 1, 262144)), (UP2, (1, 2, 2, 4, 776)),
    (C2S, (1, 4, 8, 776, 776, 256, 256, 2048, 8192, 1, 3, 3, 1, 0, 1, 1048576)),
    (C2S, (1, 4, 8, 256, 256, 2, 1, 8, 64, 32, 3, 3, 1, 0, 0, 8192)), (DISP_HEAD, (1, 32)),
    (C2S, (1, 4, 8, 256, 256, 128, 392, 6272, 50176, 1, 4, 4, 2, 1, 1, 262144)), (UP2, (1, 2, 4, 8, 392)),
    (C2S, (1, 8, 16, 392, 392, 128, 128, 2048, 16384, 1, 3, 3, 1, 0, 1, 1048576)),
    (C2S, (1, 8, 16, 128, 128, 2, 1, 16, 256, 128, 3, 3, 1, 0, 0, 16384)), (DISP_HEAD, (1, 128)),
    (C2S, (1, 8, 16, 128, 128, 64, 200, 6400, 102400, 1, 4, 4, 2, 1, 1, 262144)), (UP2, (1, 2, 8, 16, 200)),
    (C2S, (1, 16, 32, 200, 200, 64, 64, 2048, 32768, 1, 3, 3, 1, 0, 1, 1048576)),
    (C2S, (1, 16, 32, 64, 64, 2, 1, 32, 1024, 512, 3, 3, 1, 0, 0, 0)), (DISP_HEAD, (1, 512)),
    (C2S, (1, 16, 32, 64, 64, 32, 104, 6656, 212992, 1, 4, 4, 2, 1, 1, 0)), (UP2, (1, 2, 16, 32, 104)),
    (C2S, (1, 32, 64, 104, 104, 32, 32, 2048, 65536, 1, 3, 3, 1, 0, 1, 1048576)),
    (C2S, (1, 32, 64, 32, 32, 2, 1, 64, 4096, 2048, 3, 3, 1, 0, 0, 0)), (DISP_HEAD, (1, 2048))]
RMVD_PLANS = {2: [*RMVD_KEY, *RMVD_SOURCES_V2, *RMVD_FUSION_V2, *RMVD_REST],
              1: [*RMVD_KEY, *RMVD_SOURCES_V1, *RMVD_FUSION_V1, *RMVD_REST]}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def launches(monkeypatch, forward):
    """forward() once unrecorded (it packs the weights), then once with every ops.call written down as (name, its int arguments)"""
    from robustmvd_amd import ops
    real, log = ops.call, []

    def recorder(name, dev, *args):
        log.append((name, tuple(a for a in args if type(a) is int)))
        return real(name, dev, *args)

    with torch.no_grad():
        forward()
        monkeypatch.setattr(ops, "call", recorder)
        forward()
    monkeypatch.setattr(ops, "call", real)
    torch.cuda.synchronize()
    return log


def assert_plan(got, want):
    assert [name for name, _ in got] == [name for name, _ in want]
    assert got == want


@pytest.mark.parametrize("config", list(REG_PLANS))
def test_costregnet(config, dev, monkeypatch):
    import robustmvd_amd as R
    from robustmvd_amd import ops
    net = R.CostRegNet(conv0_split=config != "no_split").eval().to(dev)
    x = torch.rand(1, 16, 16, 24, 32, device=dev)
    if config == "f16":
        x = x.half()
    kw = dict(x_absmax=ops.absmax(x)) if config == "x_absmax" else {}
    assert_plan(launches(monkeypatch, lambda: net.forward_channels_last(x, **kw)), REG_PLANS[config])


@pytest.mark.parametrize("config", list(FEAT_PLANS))
def test_featurenet(config, dev, monkeypatch):
    from robustmvd_amd import _lib as L
    from robustmvd_amd.blocks import FeatureNet
    net = FeatureNet(split_layers=config != "no_split_layers").eval().to(dev)
    net.fused_head = config != "unfused_head"
    net.head_split = config != "fp32_head"
    layout, absmax = {"nchw_absmax": (L.LAYOUT_NCHW, True), "nhwc": (L.LAYOUT_NHWC, False), "border": (L.LAYOUT_NHWC_BORDER, False)}.get(
        config, (L.LAYOUT_NHWC_BORDER, True))  # the other three as MVSNet calls it
    img = torch.rand(2, 3, 32, 48, device=dev)
    assert_plan(launches(monkeypatch, lambda: net.forward_layout(img, layout, return_absmax=absmax)), FEAT_PLANS[config])


@pytest.mark.parametrize("V", [2, 1])
def test_robustmvd_engine(V, dev, monkeypatch):
    import robustmvd_amd as R
    from robustmvd_amd.registry import add_batch_dim
    model = R.RobustMVD().eval()
    sd = gc.robustmvd_weights({k: tuple(v.shape) for k, v in model.state_dict().items()}, 2)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(dev)
    s = gc.synthetic_sample(1, 64, 128, V)
    images, key, poses, intrinsics, _ = add_batch_dim(s["images"], s["keyview_idx"], s["poses"], s["intrinsics"], None)
    inputs = model.input_adapter(images=images, keyview_idx=key, poses=poses, intrinsics=intrinsics)
    assert_plan(launches(monkeypatch, lambda: model(**inputs)), RMVD_PLANS[V])
    assert model._engine is not None


def test_second_forward_packs_nothing_in_the_other_models(dev, monkeypatch):
    """the four packed-weight owners of CVP-MVSNet and Vis-MVSNet: a second forward launches no pack entry point and reuses the object"""
    from robustmvd_amd import cvp_mvsnet as C, vis_mvsnet as V
    pyramid, reg, stage = C.FeaturePyramid().eval().to(dev), C.CVPCostRegNet().eval().to(dev), V.SingleStage().eval().to(dev)
    # shapes the models' own tests run these parts at: one 8 x 12 pyramid scale of three views, CVP's coarse volume, Vis's stage 1
    images = torch.rand(3, 3, 8, 12, device=dev)
    ibuf, sbuf = [torch.zeros(3, 8, 12, 8, device=dev)], [torch.zeros(2, 11, 15, 16, device=dev)]
    vol16, vol8 = torch.rand(1, 48, 4, 6, 16, device=dev), torch.rand(1, 64, 8, 8, 8, device=dev)
    for owner, forward in ((pyramid, lambda: pyramid.forward_levels(images, 1, ibuf, sbuf)), (reg, lambda: reg.forward_channels_last(vol16)),
                           (stage, lambda: stage.fused_score(vol8)), (stage.reg, lambda: stage.pair_scores(vol8))):
        assert owner._packed is None
        log = launches(monkeypatch, forward)
        pk = owner._packed
        assert pk is not None and log and not [name for name, _ in log if name.startswith("mvd_pack")]
        assert owner._prepare() is pk
