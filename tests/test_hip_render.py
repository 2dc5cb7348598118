"""GPU checks of the mesh-rendering kernels (csrc/mesh_render.hip), of ops.mesh_render and of render_mesh / Mesh.render /
TSDFVolume.render on a GPU, on the cases of render_cases.py.  The reference project has no counterpart: the yardstick is render_numpy
in float64.

The bands come from the reference side alone (render_cases.reference_of): four times the largest gap between render_numpy in float64
and the same chain in numpy float32 on the float32-rounded projection matrices, in the projected x, y (pixels) and in relative z
(projected vertices and rendered depth).  A pixel is left out when some triangle that covers or nearly covers it, with z no more than
the winner's z (1 + zband), has an edge line within the xy band of the pixel, or when the two numpy chains disagree on its winner; at
most 1 % of the pixels may be left out.  On all others the triangle map is equal, depth is within the z band, and bary, colors and
normals are within four times their own float64-float32 numpy gap.

Measured (gaps and excluded shares from the two numpy chains alone; the device columns on an MI355X).  The kernel performs the
float32 numpy chain's operations in its order with correctly rounded divisions, so its deviations from float64 equal that chain's gaps:
    case                          gap xy [px]  gap z     excluded  device: triangle diffs  max rel |z - f64| (band)  bary (band)          normals (band)
    sphere 37x53                  9.64e-06     1.20e-06  0.000 %   0                       1.20e-06 (4.82e-06)       8.39e-05 (3.36e-04)  2.18e-07 (8.72e-07)
    sphere 96x131                 1.86e-05     2.57e-06  0.003 %   0                       2.57e-06 (1.03e-05)       1.47e-04 (5.88e-04)  2.21e-06 (8.85e-06)
    sphere+plane 37x53            2.62e-05     1.20e-06  0.000 %   0                       1.20e-06 (4.82e-06)       8.39e-05 (3.36e-04)  2.18e-07 (8.72e-07)
    sphere+plane 96x131           3.34e-05     2.57e-06  0.005 %   0                       2.57e-06 (1.03e-05)       1.47e-04 (5.88e-04)  2.21e-06 (8.85e-06)
    sphere+plane 36x52            3.02e-05     2.47e-06  0.000 %   0                       2.47e-06 (9.88e-06)       1.30e-04 (5.22e-04)  4.20e-07 (1.68e-06)
    37x53 cull back               2.62e-05     1.20e-06  0.000 %   0                       1.20e-06 (4.82e-06)       8.39e-05 (3.36e-04)  2.18e-07 (8.72e-07)
    37x53 cull front              2.62e-05     9.29e-07  0.017 %   0                       9.29e-07 (3.72e-06)       1.13e-04 (4.53e-04)  4.46e-07 (1.78e-06)
    37x53 near 3                  2.62e-05     9.29e-07  0.017 %   0                       9.29e-07 (3.72e-06)       1.13e-04 (4.53e-04)  4.46e-07 (1.78e-06)
    37x53 cull back, near 3       2.62e-05     2.40e-07  0.000 %   0                       2.40e-07 (9.61e-07)       3.76e-06 (1.51e-05)  2.78e-08 (1.11e-07)
    TSDFVolume.render 37x53       1.21e-05     8.68e-07  0.031 %   0                       8.68e-07 (3.47e-06)       -                    3.90e-07 (1.56e-06)
Colours, relative to their range: 9.2e-08 to 2.4e-06, bands four times that.  The two numpy chains agree on every pixel's winner.
"""
import functools

import numpy as np
import pytest
import torch

import fusion_cases as FC
import render_cases as RC
import tsdf_cases as TC
from robustmvd_amd import Mesh, TSDFVolume, ops, render_mesh, render_numpy
from robustmvd_amd import render as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL, LARGE = FC.SIZES
MAPS = ("depth", "triangle", "bary", "colors", "normals")


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def device_mesh(name):
    return tuple(up(a) for a in RC.mesh(name))


def matrices(Ks, Ts):
    return up(np.stack([R.compose_projection(K, T) for K, T in zip(Ks, Ts)]).astype(np.float32))


def launch(name, size, V=RC.NUM_VIEWS, views=None, colors=True, **kw):
    """ops.mesh_render of a case's mesh into the given views (default: the first V cameras) -> dict of numpy arrays (V, ...)"""
    v, t, c = device_mesh(name)
    Ks, Ts = RC.cameras(*size, V=V if views is None else max(views) + 1)
    if views is not None:
        Ks, Ts = [Ks[i] for i in views], [Ts[i] for i in views]
    out = ops.mesh_render(v, t, matrices(Ks, Ts), size, c if colors else None, **kw)
    return {k: None if a is None else a.cpu().numpy() for k, a in out.items()}


def same_bits(a, b):
    for k in MAPS:
        if (a[k] is None) != (b[k] is None):
            return False
        if a[k] is not None and not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)):
            return False
    return True


CASES = [(n, s) for n in ("sphere", "sphere+plane") for s in FC.SIZES]


@pytest.mark.parametrize("name,size", CASES, ids=[f"{n}-{s[0]}x{s[1]}" for n, s in CASES])
def test_render_against_the_definition(name, size):
    ref = RC.reference(name, *size)
    got = launch(name, size, normals=True, bary=True)
    RC.check_against_reference(ref, got, f"{name} {size[0]}x{size[1]}")
    for n in range(RC.NUM_VIEWS):  # the empty pixels of every map
        empty = got["triangle"][n] < 0
        assert (got["depth"][n][empty] == 0).all()
        for k in ("bary", "colors", "normals"):
            assert (got[k][n][:, empty] == 0).all()


@pytest.mark.parametrize("cull,near", [("back", 0.0), ("front", 0.0), (None, 3.0), ("back", 3.0)])
def test_cull_and_near_against_the_definition(cull, near):
    ref = RC.reference("sphere+plane", *SMALL, cull=cull, near=near)
    got = launch("sphere+plane", SMALL, normals=True, bary=True, cull=cull, near=near)
    RC.check_against_reference(ref, got, f"sphere+plane cull {cull} near {near}")


@pytest.mark.parametrize("name,size", CASES, ids=[f"{n}-{s[0]}x{s[1]}" for n, s in CASES])
def test_every_max_small_gives_the_same_bits(name, size):
    """max_small = 0: every triangle on the wave path; the default; H W: every triangle on its lane"""
    default = launch(name, size, normals=True, bary=True)
    assert same_bits(default, launch(name, size, normals=True, bary=True, max_small=0))
    assert same_bits(default, launch(name, size, normals=True, bary=True, max_small=size[0] * size[1]))
    assert same_bits(default, launch(name, size, normals=True, bary=True, max_small=1))
    assert same_bits(default, launch(name, size, normals=True, bary=True, load_first=True))
    assert same_bits(default, launch(name, size, normals=True, bary=True, max_small=0, load_first=True))


@pytest.mark.parametrize("V", [1, 3, 32])
def test_views_in_one_launch_give_the_bits_of_single_launches(V):
    together = launch("sphere+plane", SMALL, V=V, normals=True, bary=True)
    assert together["depth"].shape == (V,) + SMALL and together["bary"].shape == (V, 3) + SMALL
    for i in sorted({0, V // 2, V - 1}):
        alone = launch("sphere+plane", SMALL, views=[i], normals=True, bary=True)
        assert same_bits({k: together[k][i:i + 1] for k in MAPS}, alone), i


def test_two_runs_give_the_same_bits():
    a = launch("sphere+plane", LARGE, normals=True, bary=True)
    b = launch("sphere+plane", LARGE, normals=True, bary=True)
    assert same_bits(a, b)
    assert same_bits(launch("sphere+plane", LARGE, normals=True, bary=True, max_small=0), a)


def test_render_mesh_runs_33_views_in_two_launches():
    v, t, c = device_mesh("sphere+plane")
    Ks, Ts = RC.cameras(*SMALL, V=33)
    r = render_mesh(Mesh(v, t, c), Ks, Ts, SMALL, colors=True, normals=True)
    assert len(r.depth) == len(r.triangle) == len(r.mask) == len(r.colors) == len(r.normals) == 33 and r.bary is None
    assert r.depth[0].is_cuda and r.depth[0].shape == SMALL and r.mask[0].dtype == torch.bool
    first = launch("sphere+plane", SMALL, V=5, normals=True)
    for i in (0, 4, 31, 32):  # the cameras cycle with period 5
        assert np.array_equal(r.depth[i].cpu().numpy().view(np.uint32), first["depth"][i % 5].view(np.uint32))
        assert np.array_equal(r.triangle[i].cpu().numpy(), first["triangle"][i % 5])
        assert np.array_equal(r.colors[i].cpu().numpy().view(np.uint32), first["colors"][i % 5].view(np.uint32))
        assert np.array_equal(r.mask[i].cpu().numpy(), first["triangle"][i % 5] >= 0)
    pair = render_mesh((v, t), Ks[:2], Ts[:2], SMALL)
    assert pair.colors is None and pair.normals is None and torch.equal(pair.triangle[1], r.triangle[1])


@pytest.mark.parametrize("name", sorted(RC.small_cases()))
def test_small_cases(name):
    """Every screen coordinate is an exact integer or half-integer, so the edge values are exact in float32: the triangle map equals
    the float64 chain's everywhere, on every path; depth and bary differ by float32 roundings of a chain of at most 8 operations."""
    v, t = RC.small_cases()[name]
    Ks, Ts = RC.small_views()
    ref = render_numpy(v, t, Ks, Ts, RC.SMALL_SIZE, bary=True, normals=True)
    eps = float(np.finfo(np.float32).eps)
    for max_small in (None, 0, 99):
        out = ops.mesh_render(up(v), up(t), matrices(Ks, Ts), RC.SMALL_SIZE, normals=True, bary=True, max_small=max_small)
        assert np.array_equal(out["triangle"][0].cpu().numpy(), ref.triangle[0])
        assert (np.abs(out["depth"][0].cpu().numpy() - ref.depth[0]) <= 8 * eps * ref.depth[0]).all()
        assert (np.abs(out["bary"][0].cpu().numpy() - ref.bary[0]) <= 8 * eps).all()
        assert (np.abs(out["normals"][0].cpu().numpy() - ref.normals[0]) <= 8 * eps).all()
        assert out["colors"] is None


@pytest.mark.parametrize("colors,normals,bary", [(False, False, False), (True, False, False), (False, True, False), (False, False, True)])
def test_optional_maps_on_and_off(colors, normals, bary):
    everything = launch("sphere+plane", LARGE, normals=True, bary=True)
    got = launch("sphere+plane", LARGE, colors=colors, normals=normals, bary=bary)
    for k, on in (("colors", colors), ("normals", normals), ("bary", bary)):
        assert (got[k] is not None) == on
        if on:
            assert np.array_equal(got[k].view(np.uint32), everything[k].view(np.uint32))
    assert np.array_equal(got["depth"].view(np.uint32), everything["depth"].view(np.uint32))
    assert np.array_equal(got["triangle"], everything["triangle"])


def test_size_with_vector_stores():
    """H W a multiple of four: resolve's 16-byte stores of the three-channel maps; against the definition like the other sizes"""
    size = (36, 52)
    v, t, c = RC.mesh("sphere+plane")
    Ks, Ts = RC.cameras(*size)
    ref = RC.reference_of(v, t, c, Ks, Ts, size)
    got = launch("sphere+plane", size, normals=True, bary=True)
    RC.check_against_reference(ref, got, "sphere+plane 36x52")


def test_volume_on_the_device_renders_like_the_host_path():
    H, W = SMALL
    sc = FC.scene("A", H, W)
    voxel, dims, trunc = TC.volume_of(H, W)
    vol = TSDFVolume(TC.ORIGIN, voxel, dims, trunc, device=DEV)
    vol.integrate([up(d) for d in sc["depths"]], sc["Ks"], sc["Ts"])
    r = vol.render(sc["Ks"], sc["Ts"], (H, W), normals=True)
    mesh = vol.extract_mesh()
    v, t = mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy()
    ref = RC.reference_of(v, t, None, sc["Ks"], sc["Ts"], (H, W))
    got = {"depth": [d.cpu().numpy() for d in r.depth], "triangle": [a.cpu().numpy() for a in r.triangle], "bary": None, "colors": None,
           "normals": [a.cpu().numpy() for a in r.normals]}
    RC.check_against_reference(ref, got, "TSDFVolume.render 37x53")
    assert sum(int(m.sum()) for m in r.mask) > 0


def test_argument_errors():
    v, t, c = device_mesh("sphere")
    Ks, Ts = RC.cameras(*SMALL, V=1)
    mats = matrices(Ks, Ts)
    bad = t.clone()
    bad[7, 2] = len(v)
    with pytest.raises(ValueError, match="indices"):
        ops.mesh_render(v, bad, mats, SMALL)
    with pytest.raises(ValueError, match="indices"):
        render_mesh((v, bad), Ks, Ts, SMALL)
    out = ops.mesh_render(v, bad, mats, SMALL, check_indices=False)  # the kernels skip the triangle
    assert int((out["triangle"] == 7).sum()) == 0
    with pytest.raises(ValueError, match="matrices"):
        ops.mesh_render(v, t, mats.repeat(33, 1), SMALL)
    with pytest.raises(ValueError, match="cull"):
        ops.mesh_render(v, t, mats, SMALL, cull="sideways")
    with pytest.raises(ValueError, match="colors"):
        ops.mesh_render(v, t, mats, SMALL, c[:-1])
    with pytest.raises(ValueError, match="different places"):
        render_mesh((v, t.cpu()), Ks, Ts, SMALL)
    with pytest.raises(ValueError, match="max_small"):
        ops.mesh_render(v, t, mats, SMALL, max_small=-1)
