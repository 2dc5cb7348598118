"""The device's fixed-order float64 sums (csrc/fixed_sums.h and its users) against sum_order.py, the numpy model of their orders,
BIT FOR BIT: the library is built without contraction, so an IEEE double sum in a stated order has one possible result.  The
per-item terms are the definitions' own (float64(dist), cloud_register.pair_terms_numpy, the points themselves,
mesh_clean.triangle_areas_numpy), which the kernels form with the same operations; every term array is built once per module.

Sizes: around a wave (63, 64, 65), around a workgroup's 2048 items, three workgroups, and 257 * 2048 + 3, the smallest size at which
a thread of the final kernel adds two partial records.
"""
import numpy as np
import pytest
import torch

import sum_order as SO
from robustmvd_amd import cloud_register as CR
from robustmvd_amd import mesh_clean as MC
from robustmvd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 63, 64, 65, 2047, 2048, 2049, 2 * 2048 + 1, 257 * 2048 + 3]
NMAX = max(SIZES)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def decades(rng, n, lo, hi):
    return rng.uniform(0.1, 1.0, n) * 10.0 ** rng.uniform(lo, hi, n)


# ---- cloud_scores -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def distances():
    """NMAX distances over six decades, so that another order of the same terms gives other bits"""
    return decades(np.random.default_rng(1), NMAX, -5, 1).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_scores_sum_equals_the_model(distances, n):
    d = distances[:n]
    th = np.array([1e-5, 1e-4, 1e-3, 1e-2, 0.1, 1.0, 3.0, 10.0], dtype=np.float32)
    res = ops.cloud_scores(up(d), torch.zeros(n, dtype=torch.int32, device=DEV), up(th))
    total, valid, counts = ops.cloud_scores_read(res, 8)
    want = SO.fixed_sum(d.astype(np.float64))
    assert bits(total) == bits(want), (total, float(want))
    assert valid == n
    assert counts.tolist() == [int((d < t).sum()) for t in th]


# ---- cloud_pair_sums --------------------------------------------------------------------------------------------------------------------
class Pairs:
    """NMAX source points, each paired with one of 1000 targets, every row finite and every normal non-zero: the terms of the first n
    rows are those of a call on the first n points."""

    def __init__(self):
        rng = np.random.default_rng(2)
        self.target = rng.uniform(-1, 1, (1000, 3)).astype(np.float32)
        self.normals = (rng.normal(size=(1000, 3)) + 0.01).astype(np.float32)
        self.index = rng.integers(0, 1000, NMAX).astype(np.int32)
        self.source = (self.target[self.index] + rng.normal(size=(NMAX, 3)) * decades(rng, NMAX, -4, -1)[:, None]).astype(np.float32)
        w = np.array([0.02, -0.03, 0.01])
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        self.T = np.eye(4)
        self.T[:3, :3] = 1.01 * (np.eye(3) + K + 0.5 * K @ K)
        self.T[:3, 3] = [0.013, -0.007, 0.021]
        self.pivot = [0.11, -0.07, 0.05]
        self.terms = {plane: CR.pair_terms_numpy(self.source, self.T, self.index, self.target, self.pivot, self.normals if plane else None)
                      for plane in (False, True)}
        assert all(len(t) == NMAX for t in self.terms.values())  # every row is a pair

    def device(self, n, plane, index=None):
        idx = self.index[:n] if index is None else index
        res = ops.cloud_pair_sums(up(self.source[:n]), self.T, up(idx), up(self.target), self.pivot, up(self.normals) if plane else None)
        words = res.cpu().numpy()
        N, sums = ops.cloud_pair_sums_read(res, plane)
        assert (words[1 + len(sums):] == 0).all()  # the block's padding
        return N, sums


@pytest.fixture(scope="module")
def pairs():
    return Pairs()


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("n", SIZES)
def test_pair_sums_equal_the_model(pairs, n, plane):
    N, sums = pairs.device(n, plane)
    want = SO.fixed_sum(pairs.terms[plane][:n])
    assert N == n and sums.shape == want.shape == (28 if plane else 18,)
    assert np.array_equal(bits(sums), bits(want)), np.flatnonzero(bits(sums) != bits(want))


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_pair_sums_with_skipped_lanes(pairs, plane):
    """every third index is -1: those lanes add nothing, and the others keep their places in the tree"""
    n = 2 * 2048 + 1
    index = pairs.index[:n].copy()
    index[::3] = -1
    terms = pairs.terms[plane][:n].copy()
    terms[::3] = 0.0
    N, sums = pairs.device(n, plane, index)
    assert N == n - len(index[::3])
    assert np.array_equal(bits(sums), bits(SO.fixed_sum(terms)))


# ---- voxel_downsample -------------------------------------------------------------------------------------------------------------------
VOXEL_POINTS = [1, 63, 64, 65, 129, 4097]


@pytest.fixture(scope="module")
def voxels():
    """Voxel v = [v, v + 1) x [0, 1)^2 holds VOXEL_POINTS[v] points, the cloud shuffled -> (points, colours, per voxel its points'
    indices in the cloud's order, which is the order of the stable sort)"""
    rng = np.random.default_rng(3)
    vox = rng.permutation(np.repeat(np.arange(len(VOXEL_POINTS)), VOXEL_POINTS))
    n = len(vox)
    pts = np.stack([vox + rng.uniform(0.05, 0.95, n), decades(rng, n, -6, 0), decades(rng, n, -3, 0)], axis=1).astype(np.float32)
    col = (rng.uniform(0, 255, (n, 3)) * 10.0 ** rng.uniform(-4, 0, (n, 1))).astype(np.float32)
    return pts, col, [np.flatnonzero(vox == v) for v in range(len(VOXEL_POINTS))]


@pytest.mark.parametrize("colors", [False, True], ids=["xyz", "xyz-rgb"])
def test_voxel_means_equal_the_model(voxels, colors):
    pts, col, members = voxels
    xyz, rgb, counts = ops.voxel_downsample(up(pts), 1.0, up(col) if colors else None, [0.0, 0.0, 0.0])
    assert counts.cpu().tolist() == VOXEL_POINTS
    assert (rgb is not None) == colors
    for got, src in ((xyz, pts), (rgb, col)) if colors else ((xyz, pts),):
        want = np.stack([SO.segment_sum(src[m].astype(np.float64), 0, len(m)) / float(len(m)) for m in members]).astype(np.float32)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- mesh_component_sums ----------------------------------------------------------------------------------------------------------------
# Sorted positions: [0,1) [1,65) [65,100) [100,4496) [4496,4561) [4561,4861) [4861,11305).  The 35 only move the fourth to position 100,
# where it is a head, ONE whole block of 2048 and a tail; the 300 lie inside block 2 (no whole block: first >= last); the last, 3 * 2048
# + 300 from 4861, is a head, two whole blocks and a tail.
COMPONENT_TRIANGLES = [1, 64, 35, 2 * 2048 + 300, 65, 300, 3 * 2048 + 300]


def test_component_areas_equal_the_model():
    rng = np.random.default_rng(4)
    T = sum(COMPONENT_TRIANGLES)
    vtx = (rng.normal(size=(2000, 3)) * decades(rng, 2000, -2, 1)[:, None]).astype(np.float32)
    tri = rng.integers(0, 2000, (T, 3)).astype(np.int32)
    tcomp = rng.permutation(np.repeat(np.arange(len(COMPONENT_TRIANGLES)), COMPONENT_TRIANGLES)).astype(np.int32)
    key, perm = torch.sort(up(tcomp), stable=True)
    nt, area = ops.mesh_component_sums(up(vtx), up(tri), key, perm, len(COMPONENT_TRIANGLES))
    assert nt.cpu().tolist() == COMPONENT_TRIANGLES
    terms = MC.triangle_areas_numpy(vtx, tri)[perm.cpu().numpy()]
    block_sums = SO.block_record_sum(terms)
    seg = np.concatenate([[0], np.cumsum(COMPONENT_TRIANGLES)])
    assert seg[3] == 100
    want = np.array([SO.segment_sum(terms, int(seg[c]), int(seg[c + 1]), block_sums) for c in range(len(COMPONENT_TRIANGLES))])
    assert np.array_equal(bits(area.cpu().numpy()), bits(want)), np.flatnonzero(bits(area.cpu().numpy()) != bits(want))
