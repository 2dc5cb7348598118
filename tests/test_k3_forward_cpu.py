"""CPU pins of tests/k3_forward_cases.py, the references and the case table of tests/test_hip_k3_forward.py: the restatement of K3
forward against the oracle (bit for bit) and the reference's golden vectors, its folded grid against its exact one in float64, the
fmaf chain of the composed transforms, the restated PROBE step (every box holds every sample of its chunk; every case is what its
label says, with the margin a float32 probe on the device needs), and the chunks per march against csrc/warp_variance_tile.hip."""
import os
import re

import numpy as np
import pytest

import k3_forward_cases as K
from conftest import ROOT, load_golden
from oracle import mvd_oracle as O

F32, F64 = np.float32, np.float64
GOLDEN_ATOL = GOLDEN_RTOL = 1e-4  # test_oracle_golden.py
TILE_SOURCE = os.path.join(ROOT, "robustmvd_amd", "csrc", "warp_variance_tile.hip")
K3_SOURCE = os.path.join(ROOT, "robustmvd_amd", "csrc", "warp_variance.hip")


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("name", list(K.CASES))
def test_exact_float32_restatement_equals_oracle(name):
    """the same float32 operations in the same order: every bit (the clamp into the zero border replaces the oracle's in-bounds test
    of each tap and changes no value: a clamped sample has weight 0 on its one tap inside the map)"""
    feats, projs, key_inv, depth = K.case_inputs(name)
    got = K.warp_variance_restated(feats, projs, key_inv, depth, "exact", F32, F32)
    assert got.dtype == F32 and np.array_equal(got, O.warp_variance(feats[0], feats[1:], projs, key_inv, depth))


@pytest.mark.parametrize("name", K.HOMO_WARP_GEOMETRIES)
@pytest.mark.parametrize("C", [4, 32])
def test_exact_float32_homo_warp_restatement_equals_oracle(name, C):
    feats, projs, key_inv, depth = K.case_inputs(name, C)
    got = K.homo_warp_restated(feats[1], projs[0], key_inv, depth, "exact", F32, F32)
    assert np.array_equal(got, O.homo_warp(feats[1], projs[0], key_inv, depth))


@pytest.mark.parametrize("name,V", [("g4_warpvar_a", 1), ("g4_warpvar_b", 2), ("g4_warpvar_c", 2)])
def test_exact_float32_restatement_vs_reference_golden(name, V):
    g = load_golden(name)
    feats = [g[f"feat{i}"] for i in range(V + 1)]
    projs = [g[f"src_proj{v}"] for v in range(V)]
    if "warped0" in g.files:
        w0 = K.homo_warp_restated(feats[1], projs[0], g["key_proj_inv"], g["depth_values"], "exact", F32, F32)
        np.testing.assert_allclose(w0, g["warped0"], atol=GOLDEN_ATOL, rtol=GOLDEN_RTOL)
    var = K.warp_variance_restated(feats, projs, g["key_proj_inv"], g["depth_values"], "exact", F32, F32)
    np.testing.assert_allclose(var, g["variance"], atol=GOLDEN_ATOL, rtol=GOLDEN_RTOL)
    assert np.array_equal(var, O.warp_variance(feats[0], feats[1:], projs, g["key_proj_inv"], g["depth_values"]))


@pytest.mark.parametrize("name", list(K.CASES))
def test_folded_grid_equals_exact_grid_in_float64(name):
    """the two chains are the same function of real numbers; measured at most 2.9e-13 (all_three)"""
    feats, projs, key_inv, depth = K.case_inputs(name)
    a = K.warp_variance_restated(feats, projs, key_inv, depth, "exact", F64, F64)
    b = K.warp_variance_restated(feats, projs, key_inv, depth, "folded", F64, F64)
    assert a.dtype == F64 and np.isfinite(a).all()
    assert np.abs(a - b).max() <= 1e-9
    w0 = K.homo_warp_restated(feats[1], projs[0], key_inv, depth, "exact", F64, F64)
    w1 = K.homo_warp_restated(feats[1], projs[0], key_inv, depth, "folded", F64, F64)
    assert np.abs(w0 - w1).max() <= 1e-9


FLOAT32_RUNS = [(name, 32) for name in K.CASES] + [(name, C) for name in K.OTHER_CHANNEL_GEOMETRIES for C in K.OTHER_CHANNELS]


@pytest.mark.parametrize("name,C", FLOAT32_RUNS, ids=lambda x: str(x))
def test_float32_restatement_sits_inside_the_hard_band(name, C):
    """A condition on the inputs: evaluated in float32 on the CPU (either grid, transforms composed as the kernel composes them), the
    reference itself stays within HALF of the band that test_hip_k3_forward.py asserts against float64 (atol = rtol = 1e-4), so
    that the band has room for a kernel that rounds in another order.  Measured: at most 0.43 of the band (behind, C = 64, folded
    grid; the positions of samples whose Z nearly cancels carry it); the wide-baseline geometry at D = 40 and seed 77 is at 0.85,
    which is one reason why all_three has another seed."""
    feats, projs, key_inv, depth = K.case_inputs(name, C)
    for grid in ("exact", "folded"):
        want = K.warp_variance_restated(feats, projs, key_inv, depth, grid, F64, F64)
        got = K.warp_variance_restated(feats, projs, key_inv, depth, grid, F32, F32, compose="fma")
        assert (np.abs(got - want) / (1e-4 + 1e-4 * np.abs(want))).max() <= 0.5, grid


def test_single_rounding_fma():
    """a product and an addend whose sum is just above a float32 tie: float64 arithmetic rounds it onto the tie and then to even,
    one rounding goes up"""
    a = F32(1 + 2.0 ** -12)
    c = F32(2.0 ** -60)
    assert K._fma32_exact(a, a, c) == F32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert F32(F64(a) * F64(a) + F64(c)) == F32(1 + 2.0 ** -11)
    assert K._fma32_exact(F32(3), F32(5), F32(-15)) == 0 and K._fma32_exact(F32(0.1), F32(3), F32(1)) == F32(F64(F32(0.1)) * 3 + 1)


@pytest.mark.parametrize("name", ["window_ragged", "behind", "v32"])
def test_fma_composed_transforms(name):
    """compose_transforms_kernel's chain: four terms, three roundings after the first product, each at most half an ulp of a partial
    sum that |P| |Q| bounds"""
    _, projs, key_inv, _ = K.case_inputs(name)
    M = K.composed_transforms(projs, key_inv, F32, "fma")
    M64 = K.composed_transforms(projs, key_inv, F64)
    bound = np.stack([np.matmul(np.abs(p).astype(F64), np.abs(key_inv).astype(F64))[:, :3] for p in projs]) * 4 * 2.0 ** -24
    assert M.dtype == F32 and (np.abs(M - M64) <= bound).all() and np.abs(M - M64).max() > 0
    Mm = K.composed_transforms(projs, key_inv, F32, "matmul")
    assert (np.abs(Mm - M64) <= bound).all()


def test_one_hot_views_move_the_reference():
    """the all_three case with every source map but one zeroed: each view alone moves the float64 volume away from the key-only
    variance by far more than any band"""
    feats, projs, key_inv, depth = K.case_inputs("all_three")
    (B, h, w, D, V) = K.CASES["all_three"][0]
    base = K.key_only_variance(feats[0], D, V)
    for v in range(V):
        hot = [feats[0]] + [f if i == v else np.zeros_like(f) for i, f in enumerate(feats[1:])]
        ref = K.warp_variance_restated(hot, projs, key_inv, depth, "folded", F64, F64)
        assert np.abs(ref - base).max() > 1e-2


# ------------------------------------------------------------------------------------------------ probe
@pytest.mark.parametrize("win", [K.WIN_F32, K.WIN_F16])
@pytest.mark.parametrize("name", list(K.CASES))
def test_case_is_what_its_label_says(name, win):
    """at least one chunk of every class the label names and none of a class it does not name, each counted with its margin"""
    names = K.CASES[name][4][win]
    counts = K.case_classes(name, win)
    for cls in ("window", "gather", "behind"):
        if cls in names:
            assert counts[cls] >= 1, (name, win, counts)
        else:
            assert counts[cls] == 0, (name, win, counts)


def test_case_table_counts():
    """the counts the docstring of test_hip_k3_forward.py lists (fp32 window; fp16 window)"""
    want = {"window_ragged": ((24, 0, 0, 0), (24, 0, 0, 0)), "window_smallest": ((1, 0, 0, 0), (1, 0, 0, 0)),
            "gather_only": ((0, 27, 0, 0), (0, 25, 0, 2)), "mixed": ((26, 8, 0, 26), (48, 0, 0, 12)),
            "behind": ((0, 0, 30, 0), (0, 0, 30, 0)), "all_three": ((49, 47, 45, 9), (55, 40, 45, 10)),
            "short_march": ((81, 0, 0, 27), (108, 0, 0, 0)), "v32": ((7, 2, 0, 3), (10, 2, 0, 0)),
            "xcd_8_tiles": ((9, 6, 0, 1), (10, 6, 0, 0)), "xcd_9_tiles": ((16, 0, 0, 2), (18, 0, 0, 0)),
            "batch_march": ((127, 24, 0, 65), (189, 14, 0, 13))}
    for name in K.CASES:
        for win, w in zip((K.WIN_F32, K.WIN_F16), want[name]):
            c = K.case_classes(name, win)
            assert (c["window"], c["gather"], c["behind"], c["marginal"]) == w, (name, win, c)


@pytest.mark.parametrize("name", list(K.CASES))
def test_probe_box_holds_every_sample(name):
    """the 8 corner samples bound the chunk's samples (a homography maps the tile to a convex quadrilateral while Z > 0): in float64
    the first-tap cell of every (pixel, plane) of a unit without a corner behind the camera lies in the unit's box, so `locate`'s
    redo path stays untaken and a window chunk's taps all lie in its window"""
    (B, h, w, D, V), *_ = K.CASES[name]
    _, projs, key_inv, depth = K.case_inputs(name)
    cl = K.classify(projs, key_inv, depth, h, w, K.WIN_F32)
    M = K.composed_transforms(projs, key_inv, F64)
    tx = (w + K.TILE_W - 1) // K.TILE_W
    checked = 0
    for b in range(B):
        for v in range(V):
            cx, cy, _ = K.cells(M[v, b], depth[b], h, w, "folded", F64)
            for t in range(cl["npix"].shape[1]):
                ys, xs = slice((t // tx) * K.TILE_H, (t // tx + 1) * K.TILE_H), slice((t % tx) * K.TILE_W, (t % tx + 1) * K.TILE_W)
                for c in range(cl["npix"].shape[2]):
                    if cl["behind"][b, t, c, v]:
                        continue
                    xmin, xmax, ymin, ymax = cl["box"][b, t, c, v]
                    ux, uy = cx[c * K.PLANES:(c + 1) * K.PLANES, ys, xs], cy[c * K.PLANES:(c + 1) * K.PLANES, ys, xs]
                    assert xmin <= ux.min() and ux.max() <= xmax and ymin <= uy.min() and uy.max() <= ymax, (b, v, t, c)
                    checked += 1
    assert checked > 0 or name == "behind"


def test_classify_on_a_hand_made_unit():
    """identity transform: every sample is its own pixel.  A 9 x 5 map has tiles of 8 x 4, 1 x 4, 8 x 1 and 1 x 1 pixels; the
    folded position of pixel x is x * 9/8 - 0.5"""
    eye = np.eye(4, dtype=F32)[None]
    cl = K.classify([eye], eye, np.array([[1.0, 2.0, 3.0]], F32), 5, 9, K.WIN_F32)
    assert cl["npix"].shape == (1, 4, 1, 1) and not cl["behind"].any() and (cl["zrel"] == 1.0).all()
    # tile 0: ix from -0.5 to 7.375, iy (y * 5/4 - 0.5) from -0.5 to 3.25: cells 0..8 x 0..4, widened and clamped 0..9 x 0..5
    assert tuple(cl["box"][0, 0, 0, 0]) == (0, 9, 0, 5) and cl["npix"][0, 0, 0, 0] == 11 * 7
    # tile 1 (column 8 alone): ix = 8.5, cell 9, widened 8..10; tile 3 (pixel (8, 4)): iy = 4.5, cell 5, widened 4..6
    assert tuple(cl["box"][0, 1, 0, 0]) == (8, 10, 0, 5) and tuple(cl["box"][0, 3, 0, 0]) == (8, 10, 4, 6)
    assert cl["window"].all()
    # a plane behind the camera: the box is the whole zero-bordered map
    flip = eye.copy()
    flip[0, 2, 2] = -1.0
    cl = K.classify([flip], eye, np.array([[1.0]], F32), 5, 9, K.WIN_F32)
    assert cl["behind"].all() and (cl["npix"] == 12 * 8).all() and (cl["zrel"] == -1.0).all()


# ------------------------------------------------------------------------------------------------ launch arithmetic
def _struct_bytes(src, name):
    body = re.search(r"struct %s \{(.*?)\n\};" % name, src, re.S).group(1)
    n = 0
    for decl in re.findall(r"^\s*(?:float|unsigned)\s+([^;]+);", body, re.M):
        for item in decl.split(","):
            m = re.search(r"\[(\d+)\]", item)
            n += 4 * (int(m.group(1)) if m else 1)
    return n


def test_nch_of_against_the_source():
    src = open(TILE_SOURCE).read()
    assert _struct_bytes(src, "ViewRec") == K.SIZEOF_VIEWREC == 64
    assert _struct_bytes(src, "UnitRec") == K.SIZEOF_UNITREC == 32
    flat = " ".join(src.split())
    assert ("return 2 * (size_t)win * (f16 ? 64 : 128) + 2 * 4096 + 2 * 1024 + 512 + 128 + (size_t)V * sizeof(ViewRec) + "
            "(size_t)nch * 32 + (size_t)nch * V * sizeof(UnitRec);") in flat
    assert "const size_t budget = (size_t)160 * 1024 / (sets == 1 ? 4 : 3);" in flat
    assert "while (nch > 1 && tile_lds_bytes(win, f16, p.V, nch) > budget) --nch;" in flat
    assert "constexpr int P = 8, NPX = 32;" in flat
    k3 = " ".join(open(K3_SOURCE).read().split())
    # the product's variants: 8-wide tiles, window, 8 chunks asked for, one tap set
    assert "return launch_warp_tile(p, st, 8, 128, 8, 1, true, false);" in k3
    assert "return launch_warp_tile(p, st, 8, 104, 8, 1, false, p.exact_grid != 0);" in k3
    assert (K.TILE_W, K.TILE_H, K.PLANES, K.WIN_F32, K.WIN_F16) == (8, 4, 8, 104, 128)
    assert [K.nch_of(V, K.WIN_F32, False) for V in range(1, 11)] == [8] * 10
    assert [K.nch_of(V, K.WIN_F32, False) for V in (11, 12, 16, 20, 32)] == [7, 6, 4, 3, 1]
    assert K.tile_lds_bytes(K.WIN_F32, False, 10, 8) == 40 * 1024  # exactly the budget
    assert [K.nch_of(V, K.WIN_F16, True) for V in (1, 11, 20, 32)] == [8, 8, 8, 8]


def test_case_table_structure():
    """what the cases are for, beyond their labels"""
    def tiles(name):
        (B, h, w, D, V), *_ = K.CASES[name]
        return (w + K.TILE_W - 1) // K.TILE_W, (h + K.TILE_H - 1) // K.TILE_H

    (B, h, w, D, V), *_ = K.CASES["window_ragged"]
    assert B == 2 and tiles("window_ragged") == (2, 2) and w % K.TILE_W == 1 and h % K.TILE_H == 1 and D == 2 * K.PLANES + 1
    _, projs, _, depth = K.case_inputs("window_ragged")
    assert not np.array_equal(projs[0][0], projs[0][1]) and not np.array_equal(depth[0], depth[1])
    assert K.CASES["window_smallest"][0] == (1, 2, 2, 1, 1)
    # a shortened march: two chunk groups that interleave; V = 32: one chunk per march
    (B, h, w, D, V), *_ = K.CASES["short_march"]
    assert K.nch_of(V, K.WIN_F32, False) == 7 and K.march_groups(D, V, K.WIN_F32, False) == [5, 4]
    (B, h, w, D, V), *_ = K.CASES["v32"]
    assert K.nch_of(V, K.WIN_F32, False) == 1 and K.march_groups(D, V, K.WIN_F32, False) == [1, 1, 1]
    # 8 tiles fill the eight XCD slots; 9 tiles take two slots per XCD and leave 7 of 16 idle
    for name, ntiles, idle in (("xcd_8_tiles", 8, 0), ("xcd_9_tiles", 9, 7)):
        tx, ty = tiles(name)
        assert tx * ty == ntiles and 8 * ((ntiles + 7) // 8) - ntiles == idle
    # batch_march: batch, tiles per XCD slot and chunk groups all above one, ragged tiles, a last chunk of one plane
    (B, h, w, D, V), *_ = K.CASES["batch_march"]
    tx, ty = tiles("batch_march")
    assert B == 2 and (tx * ty + 7) // 8 == 2 and K.march_groups(D, V, K.WIN_F32, False) == [5, 4] and D % K.PLANES == 1
    assert w % K.TILE_W and h % K.TILE_H
    # the mixed and all_three cases keep window and gather chunks inside one march (one chunk group)
    for name in ("mixed", "all_three"):
        (B, h, w, D, V), *_ = K.CASES[name]
        assert K.march_groups(D, V, K.WIN_F32, False) == [5]
    # the largest volume of the table
    assert max(B * D * h * w for (B, h, w, D, V), *_ in K.CASES.values()) == 24 * 40 * 40
