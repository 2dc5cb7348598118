"""CPU-side checks of the K3 gather backward: the switches and their validation, the two C symbols, and the window choice.  The
gather searches (2 R + 1)^2 key pixels around each source pixel's centre (R = MVD_K3_GATHER_RADIUS); this file pins that R covers
the benchmark's and the tests' poses with one key pixel to spare, so that a later change of the window cannot quietly push them into
the atomic fallback.  Measured (numpy, float64, tests/k3_gather_geometry.py): sigma_min / radius needed
  bench configs[1] frames 0, 1, 2:  0.700 / 1   0.600 / 2   0.863 / 1        configs[2] frames 0, 1, 2:  0.794 / 1   0.680 / 1   0.866 / 1
  mvs_inputs(2,32,13,21,5,3, seed=5, rot=0.2, trans=0.3):  0.548 / 2         g4 fixtures a, b, c:  0.973 / 1   0.677 / 1   0.406 / 2
"""
import os
import re

import numpy as np
import pytest
import torch

import gen_common as gc
import k3_gather_geometry as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = {1: (448, 640, 2, 128), 2: (768, 1152, 4, 256)}  # bench.py CONFIGS[1], CONFIGS[2]: H, W, sources, planes


def _header():
    return open(os.path.join(ROOT, "include", "mvd.h")).read()


def test_switches_are_validated():
    import robustmvd_amd as R
    from robustmvd_amd import ops
    assert R.MVSNet().sweep_backward == "atomic" and not hasattr(R.MVSNet(), "sweep_backward_fallbacks")
    with pytest.raises(ValueError, match="sweep_backward"):
        R.MVSNet(sweep_backward="x")
    z = torch.zeros(1, 4, 4, 4)
    with pytest.raises(ValueError, match="backward"):
        ops.warp_variance_autograd(z, [z], [torch.eye(4)[None]], torch.eye(4)[None], torch.ones(1, 2), backward="x")
    with pytest.raises(ValueError, match="fallback_count"):
        ops.warp_variance_autograd(z, [z], [torch.eye(4)[None]], torch.eye(4)[None], torch.ones(1, 2), fallback_count=torch.zeros(1))


def test_model_owns_the_fallback_counter_and_create_model_passes_the_switch():
    import robustmvd_amd as R
    m = R.MVSNet(sweep_backward="gather")
    assert m.sweep_backward == "gather"
    c = m.sweep_backward_fallbacks
    assert c.dtype == torch.int32 and c.numel() == 1 and int(c) == 0
    assert "sweep_backward_fallbacks" not in m.state_dict()  # checkpoints are unchanged
    m = R.create_model("mvsnet_train", pretrained=False, train=True, sweep_backward="gather", train_regulariser="engine", num_gpus=0)
    assert m.sweep_backward == "gather" and m.train_regulariser == "engine" and m.training


def test_new_symbols_are_declared_and_bound_with_matching_arity():
    from robustmvd_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("mvd_warp_variance_backward_gather_workspace_bytes", "mvd_warp_variance_backward_gather_f32"):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert m, f"{name} is not declared in include/mvd.h"
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    # the gather entry point = the atomic one's arguments + int* fallback_count
    assert len(_lib.SIGNATURES["mvd_warp_variance_backward_gather_f32"][1]) == len(_lib.SIGNATURES["mvd_warp_variance_backward_f32"][1]) + 1
    assert int(re.search(r"#define\s+MVD_K3_GATHER_RADIUS\s+(\d+)", _header()).group(1)) == _lib.K3_GATHER_RADIUS


def _covered(name, projs, key_inv, depth, h, w):
    from robustmvd_amd import _lib
    sigma, need = G.pose_set_stats(projs, key_inv, depth, h, w)
    print(f"{name}: sigma_min {sigma:.4f}, window radius needed {need}, built {_lib.K3_GATHER_RADIUS}")
    assert need + 1 <= _lib.K3_GATHER_RADIUS, f"{name}: needs radius {need} + 1 spare, the window has {_lib.K3_GATHER_RADIUS}"
    return sigma, need


@pytest.mark.parametrize("cfg", [1, 2])
def test_window_covers_the_bench_poses(cfg):
    """bench.py's synthetic poses (frames 0 and 1) and tools/time_mvsnet_train.py's (frame = the config's index), depth 0.5 .. 10."""
    H, W, V, D = BENCH[cfg]
    depth = np.linspace(0.5, 10.0, D, dtype=np.float32)[None]
    for frame in (0, 1, 2):
        projs, key_inv = G.mvsnet_projections(gc.synthetic_sample(frame, H, W, V))
        _covered(f"configs[{cfg}] frame {frame}", projs, key_inv, depth, H // 4, W // 4)


def test_window_covers_the_test_poses():
    from test_hip_shapes import mvs_inputs
    _, projs, key_inv, depth = mvs_inputs(2, 32, 13, 21, 5, 3, seed=5, rot=0.2, trans=0.3)
    sigma, _ = _covered("ragged", projs, key_inv, depth, 13, 21)
    assert sigma < 1.0
    for n in "abc":
        g4 = np.load(os.path.join(ROOT, "tests", "golden", f"g4_warpvar_{n}.npz"))
        V = len([k for k in g4.files if k.startswith("src_proj")])
        h, w = g4["feat0"].shape[-2:]
        _covered(f"g4_{n}", [g4[f"src_proj{v}"] for v in range(V)], g4["key_proj_inv"], g4["depth_values"], h, w)


def test_sigma_bound_is_sufficient():
    """Wherever sigma_min is above window_sigma_limit(R), the radius needed is at most R (the bound is the sufficient side; the
    kernels decide the rest exactly, per view)."""
    rng = np.random.default_rng(3)
    Ks = gc.synthetic_intrinsics(64, 96).astype(np.float64)
    Ks[:2] *= 0.25
    Kk = np.eye(4)
    Kk[:3, :3] = Ks
    seen = 0
    for _ in range(20):
        T = gc.synthetic_pose(rng, 0.1, 0.2).astype(np.float64)
        for R in (1, 2, 3):
            sigma, need = G.pose_set_stats([(Kk @ T)[None]], np.linalg.inv(Kk)[None], np.array([[1.0, 3.0, 9.0]]), 16, 24)
            if sigma >= G.window_sigma_limit(R):
                seen += 1
                assert need <= R, (sigma, need, R)
    assert seen > 0
