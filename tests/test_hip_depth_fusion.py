"""GPU checks of the depth-fusion kernels (csrc/depth_fusion.hip) and of DepthFusion on GPU tensors, on the analytic scenes of
fusion_cases.py.  The reference project has no counterpart: the yardstick is fuse_numpy in float64.

Kernel against the definition (scene A, every view as key against the other four, and one V = 1 call).  The bands come from the
reference side alone (fusion_cases.reference): the largest difference in err, rel and d'/d between fuse_numpy in float64 and the
same chain in numpy float32 on the float32-rounded matrices, over the pairs valid in both, times four: the kernel's chain may
contract to FMAs, order its sums differently, divide the forward projection by d first and use a 1-ulp reciprocal, each of the order
of one more float32 rounding of the same chain.  A pair is left out of the bit-for-bit comparison when its float64 err or rel is
within its band of the threshold or when its validity differs between the two numpy chains (a projection on the image border); at
most 0.5 % of a case's pairs may be left out.  On all other pairs view_bits equals the float64 bits; on pixels without such a pair
count and mask are equal and fused is within the d'/d band (relative to d) of the float64 value.

Measured (gaps, bands and excluded shares from the two numpy chains alone; the kernel's columns on an MI355X):
    case               gap err [px]  gap rel   gap d'/d  excluded  kernel: wrong bits  max |fused - f64| / d  (band = 4 x gap d'/d)
    37x53  key 0       3.25e-05      5.37e-06  5.37e-06  0.038 %   0                   2.03e-07
    37x53  key 1       2.99e-05      2.91e-06  2.91e-06  0.038 %   0                   2.78e-07
    37x53  key 2       3.95e-05      4.28e-06  4.28e-06  0.013 %   0                   4.34e-07
    37x53  key 3       3.17e-05      3.12e-06  3.12e-06  0.013 %   0                   1.59e-07
    37x53  key 4       3.95e-05      5.13e-06  5.14e-06  0.038 %   0                   4.85e-07
    96x131 key 0       1.49e-04      1.01e-05  1.01e-05  0.113 %   0                   2.05e-06
    96x131 key 1       2.49e-04      8.69e-06  8.68e-06  0.080 %   0                   4.04e-06
    96x131 key 2       2.97e-04      1.61e-05  1.61e-05  0.159 %   0                   1.46e-06
    96x131 key 3       2.08e-04      1.18e-05  1.18e-05  0.129 %   0                   7.00e-07
    96x131 key 4       2.09e-04      1.08e-05  1.08e-05  0.119 %   0                   7.02e-07
    37x53  key 0, V 1  3.25e-05      5.37e-06  5.37e-06  0.051 %   0                   1.74e-07
64-77 % of the pairs are consistent and 73-83 % valid, so both tests and the bounds check decide pairs in every case.
"""
import numpy as np
import pytest
import torch

import fusion_cases as FC
from robustmvd_amd import depth_fusion as DF
from robustmvd_amd import ops
from test_depth_fusion_cpu import (bit, check_identity_source, check_invalid_depths, check_mask_and_uncertainty, check_reconstruct,
                                   check_source_facing_away)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_EXCLUDED_SHARE = 0.005


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_fuse(key_depth, key_K, key_T, src_depths, src_Ks, src_Ts, uncertainty=None, **kwargs):
    """fuse_numpy's arguments -> its dict, from the kernel"""
    mats = DF.compose_matrices(key_K, key_T, src_Ks, src_Ts).astype(np.float32)
    bits, fused, mask, count = ops.geo_consistency(up(key_depth), [up(s) for s in src_depths], up(mats),
                                                   None if uncertainty is None else up(uncertainty), **kwargs)
    assert bits.dtype == torch.uint32 and mask.dtype == torch.uint8 and count.dtype == torch.uint8
    return {"view_bits": bits.cpu().numpy(), "fused": fused.cpu().numpy(), "mask": mask.cpu().numpy(), "count": count.cpu().numpy()}


def popcount(bits):
    return sum(bit(bits, s) for s in range(32)).astype(np.uint8)


CASES = [(size, key, None) for size in FC.SIZES for key in range(5)] + [(FC.SIZES[0], 0, (2,))]


@pytest.mark.parametrize("size,key,src", CASES, ids=[f"{s[0]}x{s[1]}-key{k}" + ("-V1" if v else "") for s, k, v in CASES])
def test_kernel_against_the_definition(size, key, src):
    ref = FC.reference("A", *size, key, src)
    r64, excluded, band = ref["f64"], ref["excluded"], ref["band"]
    V = len(excluded)
    args = FC.key_and_sources(FC.scene("A", *size), key, src)
    got = device_fuse(*args)
    d = args[0].astype(np.float64)
    wrong = sum(int((bit(got["view_bits"], s) != bit(r64["view_bits"], s))[~excluded[s]].sum()) for s in range(V))
    clean = ~excluded.any(0)
    with np.errstate(all="ignore"):
        fused_gap = np.where(d > 0, np.abs(got["fused"] - r64["fused"]) / d, np.abs(got["fused"]))[clean].max()
    print(f"\n{size[0]}x{size[1]} key {key} V {V}: gap err {ref['gap']['err']:.2e} px, rel {ref['gap']['rel']:.2e}, d'/d "
          f"{ref['gap']['dd']:.2e}; excluded {100 * ref['share']:.3f} %; kernel: wrong bits {wrong}, fused gap {fused_gap:.2e}")
    assert ref["share"] <= MAX_EXCLUDED_SHARE
    assert wrong == 0
    assert got["view_bits"].max() < (1 << V)
    assert np.array_equal(got["count"], popcount(got["view_bits"]))
    assert np.array_equal(got["count"][clean], r64["count"][clean])
    assert np.array_equal(got["mask"][clean], r64["mask"][clean])
    assert fused_gap <= band["dd"]
    assert (got["fused"][~(d > 0)] == 0).all()


def test_thirty_two_sources():
    """Scene B's four sources eight times over: bit j repeats bit j % 4, bit 31 included, and the count reaches 32."""
    H, W = FC.SIZES[0]
    args = FC.key_and_sources(FC.scene("B", H, W), 0)
    four = device_fuse(*args)
    rep = lambda xs: list(xs) * 8
    got = device_fuse(args[0], args[1], args[2], rep(args[3]), rep(args[4]), rep(args[5]), min_consistent_views=32)
    assert got["view_bits"].dtype == np.uint32
    for j in range(32):
        assert np.array_equal(bit(got["view_bits"], j), bit(four["view_bits"], j % 4)), j
    assert np.array_equal(got["view_bits"] >> np.uint32(31), bit(four["view_bits"], 3))  # an unsigned word: no sign to extend
    assert np.array_equal(got["count"].astype(np.int64), 8 * four["count"].astype(np.int64))
    assert got["count"].max() == 32 and (four["count"] == 4).any()
    assert np.array_equal(got["mask"], got["count"] == 32)
    d = args[0].astype(np.float64)
    assert (np.abs(got["fused"] - d) / d).max() < 1e-4
    with pytest.raises(ValueError, match="33 views"):
        device_fuse(args[0], args[1], args[2], [args[3][0]] * 33, [args[4][0]] * 33, [args[5][0]] * 33)


@pytest.mark.parametrize("check", [check_identity_source, check_invalid_depths, check_source_facing_away, check_mask_and_uncertainty],
                         ids=lambda f: f.__name__[6:])
def test_edge_cases_on_the_device(check):
    check(device_fuse)


def test_wrapper_errors():
    d = up(FC.scene("B", *FC.SIZES[0])["depths"][0])
    mats = torch.zeros(1, 24, device=DEV)
    with pytest.raises(ValueError, match="H, W >= 2"):
        ops.geo_consistency(d[:1], [d[:1]], mats)
    with pytest.raises(ValueError, match="shape"):
        ops.geo_consistency(d, [d[:, :-1]], mats)
    with pytest.raises(ValueError, match="shape"):
        ops.geo_consistency(d, [d], torch.zeros(2, 24, device=DEV))
    with pytest.raises(ValueError, match="shape"):
        ops.geo_consistency(d, [d], mats, uncertainty=d[:-1], max_uncertainty=1.0)
    with pytest.raises(ValueError, match="shape"):
        ops.compact_points(torch.zeros(d.shape, dtype=torch.uint8, device=DEV), d[:-1], torch.zeros(12, device=DEV))
    with pytest.raises(ValueError, match="dtype"):
        ops.compact_points(torch.zeros(d.shape, dtype=torch.bool, device=DEV), d, torch.zeros(12, device=DEV))


# 66,563 pixels = 261 chunks of 256: the one-workgroup scan (csrc/compact.h) gives lanes 0-129 two counts each, lane 130 one and the
# rest none, where both sizes of FC.SIZES (20 and 50 chunks) give every lane at most one
SCAN_SIZE = (259, 257)


def compaction_masks():
    out = []
    for size in FC.SIZES + (SCAN_SIZE,):
        H, W = size
        single = np.zeros((H, W), dtype=np.uint8)
        single.reshape(-1)[H * W - 3] = 1  # in the last ballot of the last chunk of 256, both partial at every size
        assert (H * W) % 256 and (H * W) % 64 and H * W - 3 >= (H * W) // 64 * 64
        out += [(size, "zeros", np.zeros((H, W), dtype=np.uint8)), (size, "ones", np.ones((H, W), dtype=np.uint8)),
                (size, "sceneA", FC.reference("A", H, W, 0)["f64"]["mask"]), (size, "single", single)]
    return out


@pytest.mark.parametrize("size,name,mask", compaction_masks(), ids=lambda v: v if isinstance(v, str) else None)
def test_compaction(size, name, mask):
    """Row-major (np.nonzero) order, count, colours bit for bit; xyz against the float64 back-projection of the same depths within
    4e-6: the float32 roundings of B's entries, of the three FMAs and of the depth product, at most 2^-24 relative each on coordinates
    below 8, are some six times 4.8e-7."""
    H, W = size
    sc = FC.scene("A", H, W)
    depth = sc["depths"][2]
    K, T = sc["K"], sc["Ts"][2]
    bp = up(DF.compose_backprojection(K, T).astype(np.float32))
    want_xyz, want_rgb = DF.points_numpy(mask, depth, K, T, sc["images"][2])
    M = len(want_xyz)
    assert M == {"zeros": 0, "ones": H * W, "single": 1}.get(name, M) and (name != "sceneA" or 0 < M < H * W)
    for image in (None, sc["images"][2]):
        xyz, rgb, count = ops.compact_points(up(mask), up(depth), bp, None if image is None else up(image))
        assert xyz.shape == (H * W, 3) and count.dtype == torch.int64 and int(count.item()) == M
        np.testing.assert_allclose(xyz[:M].cpu().numpy(), want_xyz, rtol=0, atol=4e-6)
        if image is None:
            assert rgb is None
        else:
            assert np.array_equal(rgb[:M].cpu().numpy(), want_rgb)


def fusion_outputs(out):
    return out.mask + out.fused_depth + out.num_consistent + out.view_bits + [out.points, out.colors, out.view_index]


def test_depth_fusion_on_the_device_is_deterministic():
    H, W = FC.SIZES[1]
    sc = FC.scene("A", H, W)
    unc = [np.abs(d - np.float32(3.5)) for d in sc["depths"]]
    fusion = DF.DepthFusion(max_uncertainty=0.7)
    runs = [fusion([up(d) for d in sc["depths"]], sc["Ks"], sc["Ts"], [up(u) for u in unc], [up(im) for im in sc["images"]])
            for _ in range(2)]
    for a, b in zip(fusion_outputs(runs[0]), fusion_outputs(runs[1])):
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    out = runs[0]
    masks = [m.cpu().numpy() for m in out.mask]
    assert len(out.points) == sum(int(m.sum()) for m in masks) > 1000
    assert np.array_equal(out.view_index.cpu().numpy(), np.concatenate([np.full(int(m.sum()), i) for i, m in enumerate(masks)]))
    # the same call on the host: the verdicts differ only within the bands, a handful of pixels
    host = fusion(sc["depths"], sc["Ks"], sc["Ts"], unc, sc["images"])
    for i in range(5):
        excluded = FC.reference("A", H, W, i)["excluded"].any(0)
        assert np.array_equal(masks[i][~excluded], host.mask[i][~excluded])
        ys, xs = np.nonzero(masks[i])
        pts = out.points[out.view_index == i].cpu().numpy()
        want, _ = DF.points_numpy(masks[i], out.fused_depth[i].cpu().numpy(), sc["Ks"][i], sc["Ts"][i])
        np.testing.assert_allclose(pts, want, rtol=0, atol=4e-6)
        assert np.array_equal(out.colors[out.view_index == i].cpu().numpy(), sc["images"][i][:, ys, xs].T)


def test_reconstruct_on_the_device():
    H, W = FC.SIZES[0]
    sc = FC.scene("B", H, W)
    model = FC.StubModel(H, W, to_tensor=up, with_uncertainty=True)
    out = DF.DepthFusion(max_uncertainty=10.0).reconstruct(model, sc["images"], sc["Ks"], sc["Ts"])
    assert out.points.is_cuda and out.mask[0].is_cuda
    check_reconstruct(out, model, sc["images"], sc["Ks"], sc["Ts"], as_numpy=lambda t: t.cpu().numpy())


@pytest.mark.parametrize("how", ["model_device", "device_argument"])
def test_reconstruct_uploads_host_predictions(how):
    """A model that answers in numpy, as every registered model's run does: the predictions go to the GPU that holds the model's
    parameters (or to `device`) and the kernels fuse them; the result is GPU tensors and equals the fusion of the uploaded maps."""
    H, W = FC.SIZES[0]
    sc = FC.scene("B", H, W)
    model = FC.StubModel(H, W, with_uncertainty=True, param=torch.zeros(1, device=DEV) if how == "model_device" else None)
    fusion = DF.DepthFusion(max_uncertainty=10.0)
    out = fusion.reconstruct(model, sc["images"], sc["Ks"], sc["Ts"], **({} if how == "model_device" else {"device": DEV}))
    for t in fusion_outputs(out):
        assert t.is_cuda
    check_reconstruct(out, model, sc["images"], sc["Ks"], sc["Ts"], as_numpy=lambda t: t.cpu().numpy())
    direct = FC.StubModel(H, W, to_tensor=up, with_uncertainty=True)
    want = fusion.reconstruct(direct, sc["images"], sc["Ks"], sc["Ts"])
    for a, b in zip(fusion_outputs(out), fusion_outputs(want)):
        assert torch.equal(a, b)
    again = FC.StubModel(H, W, with_uncertainty=True, param=torch.zeros(1, device=DEV))
    host = fusion.reconstruct(again, sc["images"], sc["Ks"], sc["Ts"], device="cpu")
    assert isinstance(host.points, np.ndarray)


def test_maps_in_different_places_are_refused():
    sc = FC.scene("B", *FC.SIZES[0])
    mixed = [up(sc["depths"][0])] + list(sc["depths"][1:])
    with pytest.raises(ValueError, match="different places"):
        DF.DepthFusion()(mixed, sc["Ks"], sc["Ts"])
    with pytest.raises(ValueError, match="different places"):
        DF.DepthFusion(max_uncertainty=1.0)([up(d) for d in sc["depths"]], sc["Ks"], sc["Ts"], uncertainties=sc["depths"])
    out = DF.DepthFusion()([up(d) for d in sc["depths"]], sc["Ks"], sc["Ts"], images=sc["images"])  # host images only colour
    assert out.colors.is_cuda and len(out.colors) == len(out.points)
