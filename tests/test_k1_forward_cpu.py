"""CPU pins of tests/k1_forward_cases.py, the case table and the references of tests/test_hip_k1_forward.py: every case is what its
label says (path_stats, the restated steps 2 and 3 of sweep_corr_px_kernel), no sample of a case sits on a decision boundary of
the float32 chain, the restated pixel list is right in itself, and the float64 restatement agrees with the oracle on two of the
new geometries.

Measured (summary(name); per (key pixel, view, pass of 64 planes) unless said; "steps" are steps of 8 list pixels):
  case        passes  most  longest   most   full  >= 48 cells  steps >= 3     npix one cell    owner 1  owner 2   in3  passes    runs across  passes
                     cells     list  steps  lists  >= 16 steps  odd / even     <= 8 64 planes      taps     taps  taps  revisiting  a boundary  all masked
  full_list      34    64    256      32     32        34         2 / 32        0       0          4        4   122       34           0           0
  monotone      102    53    130      17      0         6        25 / 22       49       9       2229      383     0        0          57          60
  chain4        204    63    239      30      0       186       104 / 100       0       0       4387     1069   460      204          26           3
  invisible     324    27     62       8      0         0        74 / 66      166       2       2933      116     0        0         156         207
  behind        216    23     54       7      0         0        44 / 32      113       1       1793      298     0        1          99          60
  far_planes     20     1      4       1      0         0         0 / 0        20      10          0        0     0        0          10           4
  layout        756    10     22       3      0         0        27 / 0       514       9       2347      314     0        0         363         381
  pixel         160    12     34       5      0         0        13 / 2       113       2        345      120    77       32          75          53
  turned         54    17     38       5      0         0        35 / 19        0       0       1156      158     0        0           0           0
  nonfinite     160     8     26       4      0         0        51 / 4        41       0        423       26     0        0           0          67
Per view: the share of samples with the visibility term false for k_inf > 0 / for k_inf < 0, the share inside the map that the
visibility term alone masks, the share with a tap out of bounds, the borders with samples beyond them (l r t b), edge samples with
inb >= 0.9999 / below, samples with den == 0:
  full_list         0.00 / 0.00, 0.000, 0.53, t, 0 / 1163, 0
  monotone          0.00 / 0.00, 0.000, 0.73, l b, 0 / 3229, 0
  chain4            0.00 / 0.00, 0.000, 0.56, r t, 0 / 7364, 0
  invisible view 0  0.00 / 0.00, 0.000, 0.95, l b, 0 / 3592, 0
  invisible view 1  0.17 / 0.00, 0.000, 0.95, r b, 0 / 3583, 0
  invisible view 2  0.58 / 0.00, 0.000, 0.93, l t b, 0 / 3512, 0
  behind view 0     0.74 / 0.00, 0.546, 0.37, l r t b, 0 / 1414, 0
  behind view 1     0.00 / 0.00, 0.000, 0.00, none, 0 / 3, 0
  far_planes        0.00 / 0.00, 0.000, 0.20, none, 0 / 130, 0
  layout view 0     0.00 / 0.00, 0.000, 0.58, l r b, 0 / 5137, 0
  layout view 1     0.00 / 0.00, 0.000, 0.56, l r t b, 0 / 4906, 0
  layout view 2     0.00 / 0.00, 0.000, 0.53, l r t, 1 / 4653, 0
  pixel view 0      0.00 / 0.00, 0.000, 0.39, r t b, 0 / 1040, 0
  pixel view 1      0.00 / 0.00, 0.000, 0.32, r b, 0 / 859, 0
  turned            0.00 / 0.11, 0.000, 0.43, l r t b, 0 / 1498, 0
  nonfinite view 0  0.33 / 0.00, 0.006, 0.88, l r t b, 16 / 618, 80
  nonfinite view 1  0.00 / 0.00, 0.000, 0.71, l, 0 / 510, 0
nonfinite view 0: every key pixel on the plane ds = 2 has den == 0; there u is -inf for x < 14 and +inf above, v is -inf, NaN on the
16 pixels of the row y = 2 (its numerator is 0 as well) and +inf.  In the random-pose cases every invisible sample is out of the
map too, so only `behind` (and six-thousandths of `nonfinite`) has mask entries that the visibility term alone decides: the class
"visibility_decides" is not in the issue's table and was added for that reason.
Non-finite: a finite float32 calibration reaches den == 0 exactly (k1_forward_cases.py says how); an overflow of den needs
|t3 * ds| near 3e38 and is left out.  Every class of the table is met at a small shape."""
import numpy as np
import pytest

import k1_forward_cases as K
from oracle import mvd_oracle as O

f32 = np.float32

# class -> the condition of the issue's table on summary(name) (s), the case's shape and mode
CLASSES = {
    "full_list": lambda s, c: s["full_lists"] >= 2,
    "monotone": lambda s, c: c["mode"] in ("shared", "batched") and s["long_paths"] >= 2,
    "steps_odd_even": lambda s, c: s["odd_steps"] >= 2 and s["even_steps"] >= 2,
    "one_cell": lambda s, c: s["one_step"] >= 2 and s["one_cell"] >= 2,
    "owner2": lambda s, c: s["owner2"] >= 100,
    "chain4": lambda s, c: s["in3"] >= 100,
    "revisits": lambda s, c: s["revisit_passes"] >= 50,
    "boundary": lambda s, c: s["runs_across"] >= 2,
    "tail1": lambda s, c: c["S"] == 65,
    "tail6": lambda s, c: c["S"] == 70,
    "tail2": lambda s, c: c["S"] == 130,
    "four_passes": lambda s, c: c["S"] == 256,
    "invisible_kpos": lambda s, c: any(v["invisible_kpos"] >= 0.05 for v in s["views"]),
    "invisible_kneg": lambda s, c: any(v["invisible_kneg"] >= 0.05 for v in s["views"]),
    "visibility_decides": lambda s, c: any(v["vis_decides"] >= 0.01 for v in s["views"]),
    "masked_pass": lambda s, c: s["masked_passes"] >= 2,
    "borders": lambda s, c: all(any(v[b] for v in s["views"]) for b in ("left", "right", "top", "bottom")),
    "edge_hi": lambda s, c: any(v["edge_hi"] > 0 for v in s["views"]) and any(v["edge_lo"] > 0 for v in s["views"]),
    "nonfinite": lambda s, c: any(v["nonfinite"] > 0 for v in s["views"]),
    "layout": lambda s, c: (c["N"] == 2 and c["mode"] == "batched" and (c["hs"], c["ws"]) != (c["h"], c["w"]) and c["w"] % 16 != 0
                            and (c["h"] * -(-c["w"] // 16) * c["N"] * c["V"]) % 8 != 0),
}


def _case(name):
    (N, C, h, w, hs, ws, S, V), mode, pose, depths, seed, labels = K.CASES[name]
    return dict(N=N, C=C, h=h, w=w, hs=hs, ws=ws, S=S, V=V, mode=mode, labels=labels)


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_is_what_its_label_says(name):
    c, s = _case(name), K.summary(name)
    print(name, {k: v for k, v in s.items() if k != "views"})
    for v in s["views"]:
        print("   ", {k: x for k, x in v.items() if k != "nonfinite_at"})
    assert c["h"] * c["w"] <= 4 * 20 and c["hs"] <= 48 and c["ws"] <= 160 and s["max_npix"] <= K.LIST
    for label in c["labels"]:
        assert CLASSES[label](s, c), label


def test_every_class_is_met():
    claimed = {label for name in K.CASES for label in K.CASES[name][5]}
    assert claimed == set(CLASSES)
    # the channel sweep: sweep_corr_kernel<5 .. 8> sees an odd and an even number of distinct cells (the last step does the same
    # cell twice) and more than one pass; the warp-only runs see the invisible, out-of-the-map, per-pixel and non-finite samples
    sums = [K.summary(name) for name in K.CHANNEL_GEOMETRIES]
    assert any(s["odd_cells"] for s in sums) and any(s["even_cells"] for s in sums)
    assert any(K.case_shape(name)[6] > K.PASS for name in K.CHANNEL_GEOMETRIES)
    assert {"full_list", "chain4"} <= set(K.CHANNEL_GEOMETRIES)
    labels = {label for name in K.WARP_GEOMETRIES for label in K.CASES[name][5]}
    assert {"invisible_kpos", "borders", "nonfinite", "edge_hi"} <= labels and any(K.CASES[n][1] == "pixel" for n in K.WARP_GEOMETRIES)


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_is_off_the_decision_boundaries(name):
    """The conditions of test_sweep_grads_cpu.test_shape_sweep_inputs_are_off_the_decision_boundaries, under which the GPU tests
    demand masks EQUAL to the restated ones.  The samples of the `nonfinite` case with den == 0 are exempt from the condition on
    zs against z_pole: there zs = 1 / 2 and z_pole = 0.5 / 1 are equal in exact float32 arithmetic (no rounding takes part), and
    the sampling mask is 0 for a position of +-1e9 whatever the visibility says.  Its k_inf is exactly 1."""
    st = K.path_stats(name)
    for v, g in enumerate(K.chains(name)):
        edge = ~g["all_in"]
        d_inb = np.abs(g["inb"][edge] - f32(0.9999)).min() if edge.any() else np.inf
        d_k = np.abs(g["k_inf"]).min()
        with np.errstate(all="ignore"):
            rel = np.abs(g["zs"] - g["z_pole"]) / np.abs(g["z_pole"])
        exempt = st["views"][v]["nonfinite_at"]
        if exempt.any():
            assert "nonfinite" in K.CASES[name][5] and (g["mask"][exempt] == 0).all() and (g["k_inf"] == 1).all()
        d_z = rel[~exempt].min()
        print(f"{name} view {v}: |inb - 0.9999| >= {d_inb:.2e}, |k_inf| >= {d_k:.2e}, |zs - z_pole| / |z_pole| >= {d_z:.2e}")
        assert d_inb > 1e-6 and d_k > 1e-6 and d_z > 1e-5
        assert np.abs(g["inb"][g["all_in"]] - 1).max(initial=0) < 1e-5


@pytest.mark.parametrize("name", list(K.CASES))
def test_restated_pixel_list_names_each_cells_own_pixels(name):
    """For every pass: each list place is written exactly once, every index lies inside the list, and the four dot-product indices
    of every plane, looked up through its cell's entry, name the four source pixels of the plane's cell read directly."""
    planes = 0
    for key, cells, W2 in K.passes(name):
        L = K.pass_lists(cells, W2)
        assert 0 < L["npix"] <= K.LIST and (L["written"] == 1).all() and (L["pixlist"] >= 0).all(), key
        assert (L["idx"] >= 0).all() and (L["idx"] < L["npix"]).all(), key
        assert np.array_equal(L["cj"][L["dci"]], np.asarray(cells)), key
        want = np.asarray(cells, np.int64)[:, None] + np.array([0, 1, W2, W2 + 1])[None, :]
        assert np.array_equal(L["pixlist"][L["idx"][L["dci"]]], want), key
        # the owner's places: owner 1 / 2 read what the cell one / two back wrote itself
        for o in (1, 2):
            j, k = np.nonzero(L["owner"] == o)
            assert (j >= o).all() and L["isnew"][j - o, L["opos"][j, k]].all(), key
        planes += len(cells)
    N, _, h, w, _, _, S, V = K.case_shape(name)
    assert planes == N * V * h * w * S


@pytest.mark.parametrize("name", ["full_list", "chain4"])
def test_one_hot_picks(name):
    """the one-hot runs reach what they are for: the chain-of-four case has picks served through owner 1, owner 2, an in3 reload
    and the list's last place; the full-list case, where by construction nearly every cell is new (4 owner-1 and 4 owner-2 taps in
    all, none with a weight that makes a pick), has in3 reloads and the last place of a list of 256"""
    picks = K.one_hot_picks(name)
    kinds = {p[7] for p in picks}
    assert kinds >= ({"owner1", "owner2", "in3", "last"} if name == "chain4" else {"in3", "last"}), kinds
    st = K.path_stats(name)["passes"]
    if name == "full_list":
        assert any(p[7] == "last" and st[p[:5]]["npix"] == K.LIST for p in picks)
    for p in picks:
        n, v, y, x, ps, j, k, kind, (yy, xx), planes = p
        hit = K.readers(name, v, n, yy, xx)
        assert all(hit[n, s, y, x] for s in planes)
        want, e, mask = K.references(name, None, p)[v]
        assert (want[~hit] == 0).all() and max(abs(want[n, s, y, x]) for s in planes) > 1e-3, p


@pytest.mark.parametrize("name", ["invisible", "pixel"])
def test_restatement_matches_oracle(name):
    """the wide-baseline geometry and a per-pixel one: masks equal, values in the band of
    test_sweep_grads_cpu.test_restated_sweep_corr_matches_oracle_backward (the oracle's forward sums in float32)"""
    c = K.case_inputs(name)
    ref_c, ref_m, _ = O.planesweep_correlation(c["fk"], c["Kk"], c["fs"], c["Ts"], c["Ks"], sampling_invdepths=c["inv"])
    for v, (want, e, mask) in enumerate(K.references(name)):
        assert np.array_equal(mask, ref_m[v]) and 0 < mask.mean() < 1
        print(f"{name} view {v}: max |diff| {np.abs(want - ref_c[v]).max():.3e}, e {e:.3e}")
        np.testing.assert_allclose(want, ref_c[v], atol=2e-5, rtol=1e-5)
