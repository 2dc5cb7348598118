"""GPU checks of the TSDF kernels (csrc/tsdf.hip) and of TSDFVolume on a GPU, on the cases of tsdf_cases.py.  The reference project
has no counterpart: the yardsticks are integrate_numpy and extract_numpy in float64.

Integration against the definition (scene A, all five views, with colour).  The bands come from the reference side alone
(tsdf_cases.reference): the largest differences in u, v and Qz between integrate_numpy in float64 and the same chain in numpy float32
on the float32-rounded matrices, times four (the kernel's chain may contract to FMAs, order its operations differently and use a 1-ulp
reciprocal, each of the order of one more float32 rounding of the same chain).  A voxel is left out when, for some view, u or v is
within its band of a half-integer near the image, Qz within its band of 0, sdf + trunc within Qz's band of 0, or the two numpy chains
disagree; at most 1 % of the voxels may be left out.  On all others weight equals the float64 chain's bit for bit, tsdf is within four
times the F gap of the two numpy chains, and color within the same band relative to the colour range.

Measured (gaps, bands and excluded shares from the two numpy chains alone; the kernel's columns on an MI355X):
    case                 gap u, v [px]       gap F     excluded  kernel: weight diffs  max |F - f64|  (band)     max |C - f64| / range
    37x53                1.35e-05, 9.15e-06  1.75e-06  0.41 %    0                     1.99e-06       (7.01e-06) 2.01e-08
    96x131               3.62e-05, 2.84e-05  3.20e-06  0.35 %    0                     4.96e-06       (1.28e-05) 2.36e-08
    37x53  masks         1.35e-05, 9.15e-06  1.75e-06  0.41 %    0                     1.99e-06       (7.01e-06) 2.01e-08
    37x53  max_weight    1.35e-05, 9.15e-06  1.75e-06  0.41 %    0                     1.99e-06       (7.01e-06) 6.47e-08
    37x53  holes         1.35e-05, 9.15e-06  1.75e-06  0.41 %    0                     1.99e-06       (7.01e-06) 2.01e-08
    37x53  facing_away   1.27e-05, 9.15e-06  1.75e-06  0.40 %    0                     1.99e-06       (7.01e-06) 2.01e-08
Without a variant 74-77 % of the voxels are observed and 9-16 % of those are inside (56 % and 18 % with the masks as weights).

Extraction on an MI355X: M, T and the triangles equal in every case; the largest deviation of a vertex from the float64 form (band):
    sphere 18^3          M 1502   T 3000    5.16e-07 (2.06e-06)
    half-observed        M 746    T 1418    6.03e-07 (2.41e-06)
    integrated 37x53     M 2870   T 5270    2.91e-07 (1.16e-06)   colours 2.59e-04 (1.04e-03) of 0..4131
    integrated 96x131    M 10868  T 20774   2.87e-07 (1.15e-06)   colours 2.74e-04 (1.10e-03)
    (19,17,23) random    M 8075   T 7776    3.49e-07 (1.39e-06)   colours 2.66e-05 (1.06e-04) of 0..255
    sphere 41^3          M 11358  T 22712   1.97e-06 (7.87e-06)
    sphere 65^3          M 32992  T 65980   1.96e-06 (7.85e-06)
    min_weight 3         M 2440   T 4352    2.91e-07 (1.16e-06)
End to end on the plane: M 2367, T 4528 on the device and on the host, the same verdicts in every voxel; the largest distance of a
vertex from the plane is 2.608e-03 on both (voxel 0.1).

Extraction is compared with extract_numpy run on the device's own downloaded volume: the observed and inside verdicts are exact
comparisons of the same float32 numbers, so nothing is left out: M, T and the triangle array are equal, and the vertices and colours are
within four times the float64-float32 gap of extract_numpy on that volume.
"""
import functools

import numpy as np
import pytest
import torch

import fusion_cases as FC
import tsdf_cases as TC
from robustmvd_amd import cloud_eval as CE
from robustmvd_amd import depth_fusion as DF
from robustmvd_amd import ops
from robustmvd_amd import tsdf as TS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL, LARGE = FC.SIZES


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def down(vol):
    return (vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), None if vol.color is None else vol.color.cpu().numpy())


@functools.lru_cache(maxsize=None)
def integrated(H, W, variant=None):
    """Scene A's five views in a volume with colour on the device (built once: read-only)."""
    inp = TC.inputs("A", H, W, variant)
    voxel, dims, trunc = TC.volume_of(H, W)
    vol = TS.TSDFVolume(TC.ORIGIN, voxel, dims, trunc, inp["max_weight"], color=True, device=DEV)
    vol.integrate([up(d) for d in inp["depths"]], inp["Ks"], inp["Ts"],
                  None if inp["weights"] is None else [up(w) for w in inp["weights"]], [up(im) for im in inp["images"]])
    return vol


CASES = [(SMALL, None), (LARGE, None)] + [(SMALL, v) for v in TC.VARIANTS[1:]]


@pytest.mark.parametrize("size,variant", CASES, ids=[f"{s[0]}x{s[1]}" + (f"-{v}" if v else "") for s, v in CASES])
def test_integrate_against_the_definition(size, variant):
    ref = TC.reference("A", *size, variant)
    F, W, C = down(integrated(*size, variant))
    keep = ~ref["excluded"]
    w_diffs = int((W[keep] != ref["W"][keep].astype(np.float32)).sum())
    f_gap = float(np.abs(F - ref["F"])[keep].max())
    c_gap = float(np.abs(C - ref["C"])[:, keep].max()) / ref["span"]
    print(f"\n{size[0]}x{size[1]} {variant}: gap u {ref['gap']['u']:.2e}, v {ref['gap']['v']:.2e}, Qz {ref['gap']['qz']:.2e}, F "
          f"{ref['gap']['F']:.2e}, C {ref['gap']['C']:.2e}; excluded {100 * ref['share']:.2f} %; observed {100 * ref['observed']:.0f} %, "
          f"inside {100 * ref['inside']:.0f} %; kernel: weight diffs {w_diffs}, max |F - f64| {f_gap:.2e} (band {ref['band']['F']:.2e}), "
          f"max |C - f64| / range {c_gap:.2e}")
    assert ref["share"] <= TC.MAX_EXCLUDED_SHARE and ref["w_equal"]
    assert w_diffs == 0
    assert f_gap <= ref["band"]["F"]
    assert c_gap <= ref["band"]["F"]
    assert W.max() == ref["W"].max() and np.isfinite(F).all() and np.isfinite(C).all()


def launches(groups, inp, size, max_weight=None, color=True):
    """ops.tsdf_integrate once per group of view indices on a zero volume -> the downloaded (tsdf, weight, color)"""
    voxel, dims, trunc = TC.volume_of(*size)
    F, W, C = (None if a is None else up(a) for a in TC.zeros(dims, color))
    depths, images = [up(d) for d in inp["depths"]], [up(im) for im in inp["images"]]
    mats = up(np.stack([TS.compose_matrix(K, T, TC.ORIGIN, voxel) for K, T in zip(inp["Ks"], inp["Ts"])]).astype(np.float32))
    for g in groups:
        ops.tsdf_integrate(F, W, C, [depths[i % 5] for i in g], mats[[i % 5 for i in g]], trunc, max_weight, None,
                           [images[i % 5] for i in g] if color else None)
    return [None if a is None else a.cpu().numpy() for a in (F, W, C)]


def same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_batched_equals_sequential():
    inp = TC.inputs("A", *SMALL)
    assert same_bits(launches([range(5)], inp, SMALL), launches([[i] for i in range(5)], inp, SMALL))
    many = launches([range(32)], inp, SMALL, max_weight=8.0)
    assert same_bits(many, launches([[i] for i in range(32)], inp, SMALL, max_weight=8.0))
    assert many[1].max() == 8.0
    # 33 views through the volume: a launch of 32 and a launch of one
    voxel, dims, trunc = TC.volume_of(*SMALL)
    vol = TS.TSDFVolume(TC.ORIGIN, voxel, dims, color=True, device=DEV)
    rep = lambda xs: [xs[i % 5] for i in range(33)]
    vol.integrate(rep(inp["depths"]), rep(inp["Ks"]), rep(inp["Ts"]), images=rep(inp["images"]))  # host maps: uploaded
    assert same_bits(down(vol), launches([range(32), [32]], inp, SMALL))
    with pytest.raises(ValueError, match="33 views"):
        launches([range(33)], inp, SMALL)


def test_untouched_voxels_keep_their_bits():
    """One view into a volume moved so that part of it is outside the view's image, over a state of arbitrary bits."""
    sc = FC.scene("A", *SMALL)
    voxel, dims, trunc = TC.volume_of(*SMALL)
    origin = (TC.ORIGIN[0] - 1.0, TC.ORIGIN[1], TC.ORIGIN[2])
    view = ([sc["depths"][2]], [sc["Ks"][2]], [sc["Ts"][2]])
    skipped = np.ones(dims[::-1], dtype=bool)
    for dtype in (np.float64, np.float32):
        det = TS.integrate_numpy(*TC.zeros(dims), *view, origin, voxel, trunc, images=[sc["images"][2]], dtype=dtype, details=True)[3]
        skipped &= ~det["updated"][0]
        assert 0.1 < det["inb"].mean() < 0.9
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 32, (5,) + dims[::-1], dtype=np.uint64).astype(np.uint32)
    bits[(bits >> 23) & 0xff == 0xff] &= np.uint32(0xbfffffff)  # no NaN and no inf
    before = bits.view(np.float32)
    F, W, C = up(before[0]), up(before[1]), up(before[2:])
    ops.tsdf_integrate(F, W, C, [up(view[0][0])], up(TS.compose_matrix(view[1][0], view[2][0], origin, voxel).astype(np.float32)[None]),
                       trunc, None, None, [up(sc["images"][2])])
    after = np.concatenate([F.cpu().numpy()[None], W.cpu().numpy()[None], C.cpu().numpy()]).view(np.uint32)
    assert 0.2 < skipped.mean() < 0.95
    assert np.array_equal(after[:, skipped], bits[:, skipped])
    assert (after[1] != bits[1]).mean() > 0.5 * (~skipped).mean()  # and the others were updated


def check_extraction(vol, min_weight=1.0):
    """The device mesh against extract_numpy on the device's own downloaded volume -> the mesh as numpy arrays"""
    mesh = vol.extract_mesh(min_weight)
    assert mesh.vertices.dtype == torch.float32 and mesh.triangles.dtype == torch.int32 and mesh.vertices.is_cuda
    v, t = mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy()
    F, W, C = down(vol)
    v64, c64, t64, vband, cband = TC.extract_reference(F, W, C, vol.origin, vol.voxel, min_weight)
    assert v.shape == v64.shape and t.shape == t64.shape
    assert np.array_equal(t, t64)
    v_gap = float(np.abs(v - v64).max()) if len(v) else 0.0
    print(f"\n{vol.dims} min_weight {min_weight}: M {len(v)}, T {len(t)}, max |v - f64| {v_gap:.2e} (band {vband:.2e})", end="")
    assert v_gap <= vband
    if C is None:
        assert mesh.colors is None
    else:
        c = mesh.colors.cpu().numpy()
        c_gap = float(np.abs(c - c64).max()) if len(c) else 0.0
        print(f", max |c - f64| {c_gap:.2e} (band {cband:.2e})", end="")
        assert c.shape == c64.shape and c_gap <= cband
    return v, t


def random_volume(dims, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    F = (np.sin(0.7 * i + 0.3 * k) + np.cos(0.5 * j - 0.2 * k) + 0.2 * rng.normal(size=i.shape)).astype(np.float32)
    F[rng.random(F.shape) < 0.02] = 0.0  # zeros count as outside
    W = rng.integers(0, 4, F.shape).astype(np.float32)
    W[rng.random(F.shape) < 0.6] = 2.0
    return F, W, rng.uniform(0, 255, (3,) + F.shape).astype(np.float32)


EXTRACTIONS = {
    "sphere": lambda: TS.TSDFVolume.from_arrays(*map(up, TC.sphere_volume())),
    "half-sphere": lambda: TS.TSDFVolume.from_arrays(*map(up, TC.sphere_volume(observed_below_i=9)), origin=(0.5, -2.0, 1.0), voxel=0.3),
    "integrated-37x53": lambda: integrated(*SMALL),
    "integrated-96x131": lambda: integrated(*LARGE),
    "19x17x23": lambda: TS.TSDFVolume.from_arrays(*map(up, random_volume((19, 17, 23), 5)), origin=(-0.4, 0.1, 3.0), voxel=0.07),
    "empty": lambda: TS.TSDFVolume((0, 0, 0), 0.1, (29, 21, 25), color=True, device=DEV),
    # 270 chunks: one block of the two-level scan, its lanes own up to four counts, the last ones none
    "sphere-41": lambda: TS.TSDFVolume.from_arrays(*map(up, TC.sphere_volume(41, (20.3, 19.6, 20.9), 14.2))),
    # 1073 chunks: two blocks, the second of 49 chunks, and two block sums for compact_scan_kernel
    "sphere-65": lambda: TS.TSDFVolume.from_arrays(*map(up, TC.sphere_volume(65, (31.3, 32.6, 30.9), 24.2))),
    "one-voxel": lambda: TS.TSDFVolume.from_arrays(up(-np.ones((1, 1, 1), np.float32)), up(np.ones((1, 1, 1), np.float32))),
}


@pytest.mark.parametrize("case", list(EXTRACTIONS))
def test_extraction_against_the_definition(case):
    v, t = check_extraction(EXTRACTIONS[case]())
    if case in ("empty", "one-voxel"):
        assert len(v) == 0 and len(t) == 0
    else:
        assert len(t) > 100
    if case == "sphere":
        assert (len(v), len(t)) == (1502, 3000)
    if case == "half-sphere":
        assert (len(v), len(t)) == (746, 1418)


def test_extraction_with_a_minimum_weight():
    full = integrated(*SMALL).extract_mesh()
    v, t = check_extraction(integrated(*SMALL), min_weight=3.0)
    assert 0 < len(t) < len(full.triangles)


def test_topology_of_the_device_mesh():
    mesh = EXTRACTIONS["sphere"]().extract_mesh()
    TC.check_closed_surface(mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy(), TC.SPHERE[1])


def test_two_runs_give_the_same_bits():
    runs = []
    for _ in range(2):
        inp = TC.inputs("A", *LARGE)
        voxel, dims, trunc = TC.volume_of(*LARGE)
        vol = TS.TSDFVolume(TC.ORIGIN, voxel, dims, color=True, device=DEV)
        vol.integrate([up(d) for d in inp["depths"]], inp["Ks"], inp["Ts"], images=[up(im) for im in inp["images"]])
        mesh = vol.extract_mesh()
        runs.append([a.cpu().numpy() for a in (vol.tsdf, vol.weight, vol.color, mesh.vertices, mesh.colors)] + [mesh.triangles.cpu().numpy()])
    assert same_bits(runs[0][:5], runs[1][:5]) and np.array_equal(runs[0][5], runs[1][5]) and len(runs[0][5]) > 1000


def test_end_to_end_on_the_plane():
    """Scene B (the plane, noise-free): DepthFusion on the device, its fused depths and masks into a volume, the mesh."""
    H, W = SMALL
    sc = FC.scene("B", H, W)
    voxel, dims, _ = TC.volume_of(H, W)
    fusion = DF.DepthFusion()([up(d) for d in sc["depths"]], sc["Ks"], sc["Ts"], images=[up(im) for im in sc["images"]])
    assert fusion.points.is_cuda
    vol = TS.TSDFVolume(TC.ORIGIN, voxel, dims, color=True, device=DEV)
    vol.integrate_fusion(fusion, sc["Ks"], sc["Ts"], images=[up(im) for im in sc["images"]])
    v, t = check_extraction(vol)
    host_fusion = DF.DepthFusion()(sc["depths"], sc["Ks"], sc["Ts"], images=sc["images"])
    host = TS.TSDFVolume(TC.ORIGIN, voxel, dims, color=True).integrate_fusion(host_fusion, sc["Ks"], sc["Ts"], images=sc["images"])
    host_mesh = host.extract_mesh()
    F, Wt, _ = down(vol)
    same_verdicts = np.array_equal(F < 0, host.tsdf < 0) and np.array_equal(Wt >= 1, host.weight >= 1)
    residual, host_residual = (FC.on_plane_residual(m) * FC.PLANE_D for m in (v, host_mesh.vertices))
    print(f"\nplane: M {len(v)}, T {len(t)}; host M {len(host_mesh.vertices)}, T {len(host_mesh.triangles)}; the same verdicts in every "
          f"voxel: {same_verdicts}; max residual device {residual.max():.3e}, host {host_residual.max():.3e} (voxel {voxel})")
    if same_verdicts:  # else the comparison on the downloaded volume above stands alone
        assert np.array_equal(t, host_mesh.triangles) and np.abs(v - host_mesh.vertices).max() < 1e-4 * voxel
    assert len(t) > 500 and residual.max() < voxel
    mesh = vol.extract_mesh()
    score = CE.PointCloudEvaluation((voxel,))(mesh.vertices, fusion.points)
    assert score is not None


def test_wrapper_errors_on_the_device():
    voxel, dims, trunc = TC.volume_of(*SMALL)
    sc = FC.scene("A", *SMALL)
    F, W, C = (up(a) for a in TC.zeros(dims))
    d, m = up(sc["depths"][0]), up(np.zeros((1, 12), np.float32))
    with pytest.raises(ValueError, match="tsdf: dtype torch.float64"):
        ops.tsdf_integrate(F.double(), W, C, [d], m, trunc)
    with pytest.raises(ValueError, match=r"weight: shape \(24, 21, 29\)"):
        ops.tsdf_integrate(F, W[1:], C, [d], m, trunc)
    with pytest.raises(ValueError, match=r"color: shape \(2, 25, 21, 29\)"):
        ops.tsdf_integrate(F, W, C[:2], [d], m, trunc)
    with pytest.raises(ValueError, match="contiguous"):
        ops.tsdf_integrate(F.transpose(1, 2).contiguous().transpose(1, 2), W, None, [d], m, trunc)
    with pytest.raises(ValueError, match=r"depths\[1\]: shape \(36, 53\)"):
        ops.tsdf_integrate(F, W, C, [d, d[1:]], up(np.zeros((2, 12), np.float32)), trunc)
    with pytest.raises(ValueError, match=r"matrices: shape \(2, 12\)"):
        ops.tsdf_integrate(F, W, C, [d], up(np.zeros((2, 12), np.float32)), trunc)
    with pytest.raises(ValueError, match=r"weights\[0\]: shape \(53, 37\)"):
        ops.tsdf_integrate(F, W, C, [d], m, trunc, weights=[d.t()])
    with pytest.raises(ValueError, match=r"images\[0\]: shape \(1, 37, 53\)"):
        ops.tsdf_integrate(F, W, C, [d], m, trunc, images=[d[None]])
    with pytest.raises(ValueError, match="trunc"):
        ops.tsdf_integrate(F, W, C, [d], m, 0.0)
    with pytest.raises(ValueError, match="tsdf must be"):
        ops.tsdf_extract(F[0], W[0])
    with pytest.raises(ValueError, match="cuda"):
        ops.tsdf_integrate(F, W, C, [d.cpu()], m, trunc)
    assert not F.any() and not W.any()
    # maps on another device than the volume
    with pytest.raises(ValueError, match=r"depths\[0\] is on cuda:0, the volume on host"):
        TS.TSDFVolume(TC.ORIGIN, voxel, dims).integrate([d], sc["Ks"][:1], sc["Ts"][:1])
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match=r"depths\[0\] is on cuda:0, the volume on cuda:1"):
            TS.TSDFVolume(TC.ORIGIN, voxel, dims, device="cuda:1").integrate([d], sc["Ks"][:1], sc["Ts"][:1])
    with pytest.raises(ValueError, match="different places"):
        TS.TSDFVolume.from_arrays(F, W.cpu())
    held = torch.cuda.memory_allocated(DEV)
    with pytest.raises(ValueError, match="below 2\\^31"):
        TS.TSDFVolume((0, 0, 0), 0.01, (2048, 1024, 1024), device=DEV)
    assert torch.cuda.memory_allocated(DEV) == held
