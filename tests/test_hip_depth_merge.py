"""GPU checks of the normals kernel, the merge kernel and the attribute compaction (csrc/depth_fusion.hip) and of
DepthFusion(merge=True, normals=True) on GPU tensors, on the analytic scenes of fusion_cases.py.  The yardsticks are normals_numpy and
merge_numpy in float64; the reference project has no counterpart.

Bands (merge_cases.reference), from the two numpy chains alone as in fusion_cases.reference: four times the largest gap between the
float64 chain and the same chain in float32 on the float32-rounded matrices, in (u,v) over the pairs valid in both and in sin(angle)
between the per-view normals over the pixels valid in both.  The normals' validity never differed between the two chains.

The claims are checked view by view, from the device's OWN view_bits and mask and float64 (u,v), so that one in-band verdict of an
early view cannot cascade into the later ones: a target is certain when both fractional parts of (u,v) are farther than the (u,v)
band from 0.5; every certain target must be set, every ambiguous one must have one of its two or four candidates set, and no byte
outside before | certain | candidates may be set.  At most 0.5 % of the targets may be ambiguous.  Merged colours and normals are
compared at the emitted pixels none of whose targets is ambiguous, against the float64 mean over the device's own members.

Measured (gaps from the two numpy chains alone, in px and in sin(angle); ambiguous = share of the device's targets within the (u,v)
band of a rounding tie; the kernel's columns on an MI355X: sin(angle) of the per-view normals to float64 (bound: 4 x gap normal) and
to scene B's analytic normal (bound 1e-4), relative error of the merged colours (bound 1e-6), sin(angle) of the merged normals to
the float64 sum over the device's members (bound: 4 x gap normal), merged points on the device / in float64):
    case       gap (u,v)  gap normal  ambiguous  kernel: normal  analytic  merged rgb  merged normal  points
    A 37x53    1.35e-05   7.13e-06    0.063 %    6.50e-06        -         4.71e-08    3.55e-06       1835 / 1835
    A 96x131   3.79e-05   1.73e-05    0.069 %    1.63e-05        -         4.77e-08    9.20e-06       12484 / 12484
    B 37x53    1.40e-05   7.12e-06    0.046 %    7.65e-06        9.99e-06  4.71e-08    3.66e-06       1818 / 1818
    B 96x131   3.75e-05   1.90e-05    0.069 %    1.87e-05        2.29e-05  4.77e-08    8.91e-06       11662 / 11662
No certain target was missing, no ambiguous target without a claimed candidate, no stray byte.  DepthFusion(merge=True, normals=True)
on scene A at 96x131: 12484 points on the device and on the host (44561 plain), emission differs at 0 pixels; this is reported, not
asserted, because one in-band verdict can move a claim.
"""
import functools

import numpy as np
import pytest
import torch

import fusion_cases as FC
import merge_cases as MC
from robustmvd_amd import depth_fusion as DF
from robustmvd_amd import ops
from test_depth_merge_cpu import check_analytic_normal, check_normal_faces_the_camera, check_normal_validity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [("A", FC.SIZES[0]), ("A", FC.SIZES[1]), ("B", FC.SIZES[0]), ("B", FC.SIZES[1])]
case_ids = [f"{n}-{s[0]}x{s[1]}" for n, s in CASES]


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def backprojection(K, T):
    return up(DF.compose_backprojection(K, T).astype(np.float32))


def device_normals(depth, K, T):
    """normals_numpy's arguments -> its map, from the kernel"""
    return ops.depth_normals(up(np.asarray(depth, dtype=np.float32)), backprojection(K, T)).cpu().numpy()


def matrices(sc, i, src):
    return up(DF.compose_matrices(sc["Ks"][i], sc["Ts"][i], [sc["Ks"][j] for j in src], [sc["Ts"][j] for j in src]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def device_replay(name, H, W):
    """The scene merged on the device view by view with ops.geo_merge, all five claimed maps copied before and after every view."""
    sc = FC.scene(name, H, W)
    depths, images = [up(d) for d in sc["depths"]], [up(im) for im in sc["images"]]
    normals = [ops.depth_normals(depths[i], backprojection(sc["Ks"][i], sc["Ts"][i])) for i in range(MC.N_VIEWS)]
    claimed = [torch.zeros((H, W), dtype=torch.uint8, device=DEV) for _ in range(MC.N_VIEWS)]
    snapshot = lambda: {j: c.cpu().numpy() for j, c in enumerate(claimed)}
    steps = []
    for i, src in enumerate(MC.SOURCES):
        before = snapshot()
        out = ops.geo_merge(depths[i], [depths[j] for j in src], matrices(sc, i, src), claimed[i], [claimed[j] for j in src],
                            key_image=images[i], src_images=[images[j] for j in src], key_normal=normals[i],
                            src_normals=[normals[j] for j in src])
        step = dict(zip(("view_bits", "fused", "mask", "count", "merged_rgb", "merged_normal"), (t.cpu().numpy() for t in out)))
        step.update(before=before, after=snapshot())
        steps.append(step)
    return {"steps": steps, "normals": [n.cpu().numpy() for n in normals]}


@pytest.mark.parametrize("name,size", CASES, ids=case_ids)
def test_normals_kernel(name, size):
    ref = MC.reference(name, *size)
    got = device_replay(name, *size)["normals"]
    worst = 0.0
    for i in range(MC.N_VIEWS):
        want = ref["f64"]["normals"][i]
        ok = MC.valid_normal(want)
        assert np.array_equal(MC.valid_normal(got[i]), ok)
        assert (np.abs(np.linalg.norm(got[i][:, ok].astype(np.float64), axis=0) - 1) < 1e-6).all()
        worst = max(worst, float(MC.sin_angle(got[i][:, ok], want[:, ok]).max()))
    print(f"\nscene {name} {size[0]}x{size[1]}: normal gap {ref['gap']['normal']:.2e}; kernel: sin(angle) to float64 {worst:.2e}")
    assert ref["same_normal_validity"]
    assert worst <= ref["band"]["normal"]
    if name == "B":
        check_analytic_normal(device_normals, size)


@pytest.mark.parametrize("check", [check_normal_validity, check_normal_faces_the_camera], ids=lambda f: f.__name__[6:])
def test_normal_edge_cases_on_the_device(check):
    check(device_normals)


@pytest.mark.parametrize("size", FC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_kernel_is_the_consistency_kernel_plus_claims(size):
    """No float64 band here: with all-zero claimed maps the four outputs are ops.geo_consistency's bits, and a random key_claimed only
    takes pixels out of the mask."""
    H, W = size
    sc = FC.scene("A", H, W)
    rng = np.random.default_rng(5)
    depths = [up(d) for d in sc["depths"]]
    unc = up(np.abs(sc["depths"][0] - np.float32(3.5)))
    for i, src, kwargs in [(k, MC.SOURCES[k], {}) for k in range(MC.N_VIEWS)] + [(0, [2], {}), (0, MC.SOURCES[0], {"uncertainty": unc,
                                                                                                                   "max_uncertainty": 0.7})]:
        args = (depths[i], [depths[j] for j in src], matrices(sc, i, src))
        plain = ops.geo_consistency(*args, **kwargs)
        zeros = lambda: [torch.zeros((H, W), dtype=torch.uint8, device=DEV) for _ in src]
        got = ops.geo_merge(*args, torch.zeros((H, W), dtype=torch.uint8, device=DEV), zeros(), **kwargs)
        assert got[4] is None and got[5] is None
        for a, b in zip(got[:4], plain):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        key_claimed = up((rng.random((H, W)) < 0.4).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8))
        got = ops.geo_merge(*args, key_claimed, zeros(), **kwargs)
        assert torch.equal(got[2], plain[2] & (key_claimed == 0).to(torch.uint8))
        assert 0 < int(got[2].sum()) < int(plain[2].sum())
        for k in (0, 1, 3):
            assert torch.equal(got[k].view(torch.uint8), plain[k].view(torch.uint8))


@pytest.mark.parametrize("name,size", CASES, ids=case_ids)
def test_claims_step_by_step(name, size):
    ref = MC.reference(name, *size)
    steps = device_replay(name, *size)["steps"]
    total = ambiguous = 0
    for i, (src, step) in enumerate(zip(MC.SOURCES, steps)):
        det = ref["views"][i]["f64"]
        if i:
            for j in range(MC.N_VIEWS):
                assert np.array_equal(step["before"][j], steps[i - 1]["after"][j])
        assert np.array_equal(step["before"][i], step["after"][i])  # the key's own map is read only
        t, a = MC.check_claims(src, step["view_bits"], step["mask"], det["u"], det["v"], ref["band"]["uv"], step["before"], step["after"])
        total, ambiguous = total + t, ambiguous + a
    share = ambiguous / total
    merged = sum(int(s["mask"].sum()) for s in steps)
    print(f"\nscene {name} {size[0]}x{size[1]}: (u,v) gap {ref['gap']['uv']:.2e} px; {total} targets, {100 * share:.3f} % ambiguous; "
          f"{merged} points merged on the device, {sum(int(m.sum()) for m in ref['f64']['mask'])} in float64")
    assert total > 1000 and share <= MC.MAX_AMBIGUOUS_SHARE
    assert not steps[0]["before"][0].any() and all(s["after"][j].max() <= 1 for s in steps for j in s["after"])


@pytest.mark.parametrize("name,size", CASES, ids=case_ids)
def test_merged_colours_and_normals(name, size):
    """The colour sums are at most 33 integers below 2^24, exact in float32: only the division rounds, rtol 1e-6.  The normal is within
    the normal band of the float64 normalised sum over the device's own members, and valid at the same pixels."""
    ref = MC.reference(name, *size)
    sc, replay = ref["scene"], device_replay(name, *size)
    worst_rgb = worst_n = 0.0
    checked = 0
    for i, (src, step) in enumerate(zip(MC.SOURCES, replay["steps"])):
        det = ref["views"][i]["f64"]
        rgb, nrm, clean = MC.member_means(src, step["view_bits"], step["mask"], det["u"], det["v"], ref["band"]["uv"], step["count"],
                                          sc["images"][i], sc["images"], ref["f64"]["normals"][i], ref["f64"]["normals"])
        off = step["mask"] == 0
        assert not step["merged_rgb"][:, off].any() and not step["merged_normal"][:, off].any()
        np.testing.assert_allclose(step["merged_rgb"][:, clean], rgb[:, clean], rtol=1e-6, atol=0)
        with np.errstate(all="ignore"):
            rel = np.abs(step["merged_rgb"][:, clean] - rgb[:, clean]) / np.abs(rgb[:, clean])
        worst_rgb = max(worst_rgb, float(np.nanmax(rel)))
        ok = MC.valid_normal(nrm) & clean
        assert np.array_equal(MC.valid_normal(step["merged_normal"])[clean], MC.valid_normal(nrm)[clean])
        worst_n = max(worst_n, float(MC.sin_angle(step["merged_normal"][:, ok], nrm[:, ok]).max()))
        checked += int(clean.sum())
    print(f"\nscene {name} {size[0]}x{size[1]}: {checked} pixels; merged rgb rel err {worst_rgb:.2e}; merged normal sin(angle) {worst_n:.2e} "
          f"(band {ref['band']['normal']:.2e})")
    assert checked > 1000
    assert worst_n <= ref["band"]["normal"]


def test_one_source_colours_decode_to_the_claimed_pixels():
    """One source and min_consistent_views = 1: twice the merged colour minus the key's is the member's own colour (x + 1000 j, y,
    7 j), which names the view and the pixel it came from.  The decoded pixels are exactly the bytes the call set."""
    H, W = FC.SIZES[1]
    sc = FC.scene("A", H, W)
    i, j = 1, 3
    claimed = [torch.zeros((H, W), dtype=torch.uint8, device=DEV) for _ in range(2)]
    image = lambda k: up(sc["images"][k])
    bits, fused, mask, count, rgb, _ = ops.geo_merge(up(sc["depths"][i]), [up(sc["depths"][j])], matrices(sc, i, [j]), claimed[0],
                                                     [claimed[1]], min_consistent_views=1, key_image=image(i), src_images=[image(j)])
    mask, rgb = mask.cpu().numpy().astype(bool), rgb.cpu().numpy().astype(np.float64)
    assert np.array_equal(mask, bits.cpu().numpy() == 1) and mask.sum() > 1000
    member = 2.0 * rgb[:, mask] - sc["images"][i][:, mask]
    assert (member[2] == 7.0 * j).all()
    tx, ty = member[0] - 1000.0 * j, member[1]
    assert (tx == np.rint(tx)).all() and (ty == np.rint(ty)).all() and (0 <= tx).all() and (tx < W).all() and (0 <= ty).all() and (ty < H).all()
    want = np.zeros((H, W), dtype=np.uint8)
    want[ty.astype(np.int64), tx.astype(np.int64)] = 1
    assert np.array_equal(claimed[1].cpu().numpy(), want) and not claimed[0].any()
    u, v = FC.reference("A", H, W, i, (j,))["f64"]["u"][0][mask], FC.reference("A", H, W, i, (j,))["f64"]["v"][0][mask]
    assert np.abs(tx - u).max() <= 0.5 + MC.reference("A", H, W)["band"]["uv"] and np.abs(ty - v).max() <= 0.5 + MC.reference("A", H, W)["band"]["uv"]


def result_tensors(out):
    return (out.mask + out.fused_depth + out.num_consistent + out.view_bits + out.claimed
            + [out.points, out.colors, out.normals, out.view_index])


def test_depth_fusion_merges_on_the_device():
    H, W = FC.SIZES[1]
    ref = MC.reference("A", H, W)
    sc = ref["scene"]
    fusion = DF.DepthFusion(merge=True, normals=True)
    runs = [fusion([up(d) for d in sc["depths"]], sc["Ks"], sc["Ts"], images=[up(im) for im in sc["images"]]) for _ in range(2)]
    for a, b in zip(result_tensors(runs[0]), result_tensors(runs[1])):
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    out = runs[0]
    masks = [m.cpu().numpy() for m in out.mask]
    final = [c.cpu().numpy() for c in out.claimed]
    total, ambiguous = MC.check_result(MC.SOURCES, [b.cpu().numpy() for b in out.view_bits], masks,
                                       [c.cpu().numpy() for c in out.num_consistent], final, [v["f64"] for v in ref["views"]],
                                       ref["band"]["uv"])
    assert total > 1000 and ambiguous / total <= MC.MAX_AMBIGUOUS_SHARE
    # the same scene step by step through ops.geo_merge: the class is that loop
    steps = device_replay("A", H, W)["steps"]
    for i, step in enumerate(steps):
        assert np.array_equal(masks[i], step["mask"]) and np.array_equal(out.view_bits[i].cpu().numpy(), step["view_bits"])
        assert np.array_equal(final[i], steps[-1]["after"][i])
    plain = DF.DepthFusion()([up(d) for d in sc["depths"]], sc["Ks"], sc["Ts"])
    M = sum(int(m.sum()) for m in masks)
    assert len(out.points) == len(out.colors) == len(out.normals) == len(out.view_index) == M
    assert 1000 < M < len(plain.points) and plain.normals is None and plain.claimed is None
    assert np.array_equal(out.view_index.cpu().numpy(), np.concatenate([np.full(int(m.sum()), i) for i, m in enumerate(masks)]))
    for i, step in enumerate(steps):
        ys, xs = np.nonzero(masks[i])
        sel = out.view_index == i
        want, _ = DF.points_numpy(masks[i], out.fused_depth[i].cpu().numpy(), sc["Ks"][i], sc["Ts"][i])
        np.testing.assert_allclose(out.points[sel].cpu().numpy(), want, rtol=0, atol=4e-6)  # test_hip_depth_fusion.test_compaction's bound
        assert np.array_equal(out.colors[sel].cpu().numpy(), step["merged_rgb"][:, ys, xs].T)
        assert np.array_equal(out.normals[sel].cpu().numpy(), step["merged_normal"][:, ys, xs].T)
    # the host path on the same scene: reported, not asserted
    host = fusion(sc["depths"], sc["Ks"], sc["Ts"], images=sc["images"])
    differ = sum(int((masks[i] != host.mask[i]).sum()) for i in range(MC.N_VIEWS))
    print(f"\nscene A {H}x{W}: {M} points on the device, {len(host.points)} on the host, {len(plain.points)} plain; "
          f"emission differs at {differ} pixels")
    # normals without merge: the plain cloud with each view's own normals
    own = DF.DepthFusion(normals=True)([up(d) for d in sc["depths"]], sc["Ks"], sc["Ts"])
    assert torch.equal(own.points, plain.points) and own.claimed is None and own.colors is None
    normals = device_replay("A", H, W)["normals"]
    for i in range(MC.N_VIEWS):
        ys, xs = np.nonzero(plain.mask[i].cpu().numpy())
        assert np.array_equal(own.normals[own.view_index == i].cpu().numpy(), normals[i][:, ys, xs].T)


def compaction_masks():
    out = []
    for size in FC.SIZES:
        H, W = size
        ragged = FC.reference("A", H, W, 0)["f64"]["mask"]
        out += [(size, "empty", np.zeros((H, W), dtype=np.uint8)), (size, "full", np.ones((H, W), dtype=np.uint8)), (size, "ragged", ragged)]
    return out


@pytest.mark.parametrize("size,name,mask", compaction_masks(), ids=lambda v: v if isinstance(v, str) else None)
def test_attribute_compaction(size, name, mask):
    H, W = size
    sc = FC.scene("A", H, W)
    rng = np.random.default_rng(11)
    attr = rng.standard_normal((3, H, W)).astype(np.float32)
    depth, bp = up(sc["depths"][2]), backprojection(sc["K"], sc["Ts"][2])
    ys, xs = np.nonzero(mask)
    M = len(ys)
    assert M == {"empty": 0, "full": H * W}.get(name, M) and (name != "ragged" or 0 < M < H * W)
    for image in (None, up(sc["images"][2])):
        xyz0, rgb0, count0 = ops.compact_points(up(mask), depth, bp, image)
        got = ops.compact_points(up(mask), depth, bp, image, normals=up(attr))
        assert len(got) == 4
        xyz, rgb, count, nrm = got
        assert int(count.item()) == int(count0.item()) == M and nrm.shape == (H * W, 3)
        assert torch.equal(xyz[:M].view(torch.uint8), xyz0[:M].view(torch.uint8))
        assert (rgb is None and rgb0 is None) if image is None else torch.equal(rgb[:M], rgb0[:M])
        assert np.array_equal(nrm[:M].cpu().numpy(), attr[:, ys, xs].T)
        again = ops.compact_points(up(mask), depth, bp, image, normals=up(attr), out=(xyz, rgb, nrm))  # the buffers, written again
        assert again[3] is nrm and again[0] is xyz


def test_wrapper_errors():
    H, W = FC.SIZES[0]
    sc = FC.scene("B", H, W)
    d = up(sc["depths"][0])
    mats = torch.zeros(1, 24, device=DEV)
    claim = lambda: torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    n = torch.zeros((3, H, W), device=DEV)
    with pytest.raises(ValueError, match="among its own sources"):
        DF.DepthFusion(merge=True)([up(x) for x in sc["depths"]], sc["Ks"], sc["Ts"], sources=[[0, 1], [0], [0], [0], [0]])
    c = claim()
    with pytest.raises(ValueError, match="key_claimed is among src_claimed"):
        ops.geo_merge(d, [d], mats, c, [c])
    with pytest.raises(ValueError, match="key_claimed is among src_claimed"):
        ops.geo_merge(d, [d, d], torch.zeros(2, 24, device=DEV), c, [claim(), c.view(H, W)])
    with pytest.raises(RuntimeError, match="src_claimed.1. is key_claimed"):  # the entry's own refusal, below the wrapper
        ops.call("mvd_geo_merge_f32", d.device, d, [d, d], torch.zeros(2, 24, device=DEV), None, 2, H, W, 1.0, 0.01, 2, 0.0, c, [claim(), c],
                 None, None, None, None, torch.zeros((H, W), dtype=torch.int32, device=DEV), torch.zeros_like(d), claim(), None, None, None)
    with pytest.raises(RuntimeError, match="merged_normal go together"):  # normals without their output buffer
        ops.call("mvd_geo_merge_f32", d.device, d, [d], mats, None, 1, H, W, 1.0, 0.01, 1, 0.0, c, [claim()], None, None, n, [n],
                 torch.zeros((H, W), dtype=torch.int32, device=DEV), torch.zeros_like(d), claim(), None, None, None)
    with pytest.raises(RuntimeError, match="attr and attr_out go together"):
        ops.call("mvd_compact_points_attr_f32", d.device, claim(), d, None, n, torch.zeros(12, device=DEV), H, W,
                 torch.zeros((H * W, 3), device=DEV), None, None, torch.zeros(1, dtype=torch.int64, device=DEV),
                 ops.workspace(4096, d.device), 4096)
    with pytest.raises(ValueError, match="go together"):
        ops.geo_merge(d, [d], mats, claim(), [claim()], key_normal=n)
    with pytest.raises(ValueError, match="go together"):
        ops.geo_merge(d, [d], mats, claim(), [claim()], src_images=[n])
    with pytest.raises(ValueError, match="dtype"):
        ops.geo_merge(d, [d], mats, claim().bool(), [claim()])
    with pytest.raises(ValueError, match="shape"):
        ops.geo_merge(d, [d], mats, claim(), [claim()[:-1]])
    with pytest.raises(ValueError, match="1 entries for 2 views"):
        ops.geo_merge(d, [d, d], torch.zeros(2, 24, device=DEV), claim(), [claim()])
    with pytest.raises(ValueError, match="shape"):
        ops.geo_merge(d, [d], mats, claim(), [claim()], key_image=n[:, :-1], src_images=[n])
    with pytest.raises(ValueError, match="shape"):
        ops.compact_points(claim(), d, torch.zeros(12, device=DEV), normals=n[:2])
    with pytest.raises(ValueError, match="12 floats"):
        ops.depth_normals(d, torch.zeros(9, device=DEV))
    # mixed places: a claimed map on the host, a host backprojection, and a mixed list of maps in merge mode
    with pytest.raises(ValueError, match="cuda"):
        ops.geo_merge(d, [d], mats, claim().cpu(), [claim()])
    with pytest.raises(ValueError, match="cuda"):
        ops.depth_normals(d, torch.zeros(12))
    with pytest.raises(ValueError, match="different places"):
        DF.DepthFusion(merge=True, normals=True)([d] + list(sc["depths"][1:]), sc["Ks"], sc["Ts"])
