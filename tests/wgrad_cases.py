"""Cases of the weight-gradient kernel conv3d_weight_grad_kernel<COT, CIT, S> (csrc/conv3d_backward.hip) for
tests/test_hip_conv3d_weight_grad.py (device) and tests/test_conv3d_weight_grad_cpu.py (no GPU); no test lives here.

The kernel sees every mode as one reduction over a "small" tensor s (B,Ds,hs,ws,Cs), which it tiles, and a "big" tensor g
(B,S*Ds,S*hs,S*ws,Cg), which it reads with a halo:  gw[cs,cg,k] = sum_{b,o} s[b,o,cs] gpad[b, S*o + k, cg].
  Conv3d stride 1 / 2:  s = gy, g = x, Cs = Cout, Cg = Cin, S = 1 / 2;   ConvTranspose3d:  s = x, g = gy, Cs = Cin, Cg = Cout, S = 2.
COT / CIT are the 16-channel tiles of a 32-channel block of Cs / Cg (2 above 16 channels), and more than 32 channels on a
side give a second block: the table states (COT, CIT, S) and (cs_blocks, cg_blocks) per case as literals; expected_plan derives
them from the rule above and plan() asks the library (mvd_conv3d_weight_grad_plan_field, a host function: no GPU needed).

An element's small tensor is 9 x 9 x (2 TW + 1) voxels (TW = 16 for S = 1, 8 for S = 2): three tile rows of 4, the last with one
live row; three tile columns, the last with one live column; an interior tile with real data in its halo on both sides; depth
chunks 8 + 1 at DZ = 8, i.e. seven march steps with kept ring planes and a second chunk whose first halo plane is real data.
The work items come from the batch: batch element b is element b % 3 of three distinct ones, so the reference is
sum_e count_e gw_e from three small float64 reductions, and a wrong batch offset shows."""
import numpy as np
import torch

from test_hip_conv3d_backward import _layers

STRIDE1, STRIDE2, DECONV = 0, 1, 2   # MVD_CONV3D_STRIDE1, MVD_CONV3D_STRIDE2, MVD_DECONV3D_STRIDE2 (pinned in the CPU test)
ELEMENTS = 3
SMALL_DHW = {1: (9, 9, 33), 2: (9, 9, 17)}   # per S: (Ds, hs, ws) = (9, 9, 2 TW + 1)

# (B, DZ, items, regime): the plan of every case at that batch size (9 tiles per element; 512 partials at most).  If a retune
# of wgrad_plan moves a regime, change B here, not the assertion.
REGIMES = [
    (2, 1, 162, "one item per workgroup"),
    (12, 2, 540, "persistent"),
    (20, 4, 540, "persistent"),
    (29, 8, 522, "persistent, ten workgroups take a second item"),
]
MAX_PARTIALS = 512
MARCH8 = REGIMES[3]

# name -> (mode, Cin, Cout, (COT, CIT, S), (cs_blocks, cg_blocks))
_LAYER_PLANS = {
    "conv0": ((1, 2, 1), (1, 1)), "conv1": ((1, 1, 2), (1, 1)), "conv2": ((1, 1, 1), (1, 1)), "conv3": ((2, 1, 2), (1, 1)),
    "conv4": ((2, 2, 1), (1, 1)), "conv5": ((2, 2, 2), (2, 1)), "conv6": ((2, 2, 1), (2, 2)), "conv7": ((2, 2, 2), (2, 1)),
    "conv9": ((2, 1, 2), (1, 1)), "conv11": ((1, 1, 2), (1, 1)), "prob": ((1, 1, 1), (1, 1)),
}
LAYER_CASES = {name: (mode, cin, cout) + _LAYER_PLANS[name] for name, cin, cout, mode in _layers()}
UNREACHED_CASES = {  # the two instantiations no CostRegNet layer maps to, in every mode that reaches them
    "s1_16to32": (STRIDE1, 16, 32, (2, 1, 1), (1, 1)),
    "s2_32to16": (STRIDE2, 32, 16, (1, 2, 2), (1, 1)),
    "up_16to32": (DECONV, 16, 32, (1, 2, 2), (1, 1)),
}
OFFGRID_CASES = {  # channel counts off the network's grid
    "s1_3to5": (STRIDE1, 3, 5, (1, 1, 1), (1, 1)),      # scalar staging on both sides
    "up_5to3": (DECONV, 5, 3, (1, 1, 2), (1, 1)),       # scalar staging on both sides
    "s2_20to36": (STRIDE2, 20, 36, (2, 2, 2), (2, 1)),  # vector path with the c < C guard; a second Cs block with 4 live channels
    "s1_33to17": (STRIDE1, 33, 17, (2, 2, 1), (1, 2)),  # scalar staging; a second Cg block with 1 live channel
    "up_48to40": (DECONV, 48, 40, (2, 2, 2), (2, 2)),   # both second blocks half-empty
    "s2_64to1": (STRIDE2, 64, 1, (1, 2, 2), (1, 2)),    # Cs = 1
    "s1_1to64": (STRIDE1, 1, 64, (2, 1, 1), (2, 1)),    # Cg = 1
}
CASES = {**LAYER_CASES, **UNREACHED_CASES, **OFFGRID_CASES}
ROUNDING_CASES = list(LAYER_CASES) + list(UNREACHED_CASES)
CONTRACT_CASES = ["conv4", "conv5"]   # one per S: <2,2,1> and <2,2,2> with two Cs blocks

FIELDS = ("DZ", "ITEMS", "PARTIALS", "COT", "CIT", "S", "CS_BLOCKS", "CG_BLOCKS")


def sides(name):
    """(S, Cs, Cg) of a case: the stride of the taps and the channels of the tiled and of the haloed tensor"""
    mode, cin, cout = CASES[name][:3]
    return (2, cin, cout) if mode == DECONV else (1 if mode == STRIDE1 else 2, cout, cin)


def expected_plan(name):
    """((COT, CIT, S), (cs_blocks, cg_blocks)) from the rule in the module docstring"""
    S, Cs, Cg = sides(name)
    tiles = lambda c: (c + 15) // 16
    return (min(tiles(Cs), 2), min(tiles(Cg), 2), S), ((tiles(Cs) + 1) // 2, (tiles(Cg) + 1) // 2)


def input_dhw(name):
    """(Di, hi, wi) of the layer's input x for one element of the case"""
    mode = CASES[name][0]
    S = sides(name)[0]
    d, h, w = SMALL_DHW[S]
    return (2 * d, 2 * h, 2 * w) if mode == STRIDE2 else (d, h, w)


def plan(name, B):
    """The library's plan for the case at batch size B: a dict over FIELDS"""
    from robustmvd_amd import _lib as L
    mode, cin, cout = CASES[name][:3]
    fn = L.load().mvd_conv3d_weight_grad_plan_field
    return {f: int(fn(B, *input_dhw(name), cin, cout, mode, getattr(L, "WGRAD_PLAN_" + f))) for f in FIELDS}


def assert_plan(name, regime):
    """The library runs `name` in `regime` (an entry of REGIMES) on the instantiation and channel blocks the table states."""
    B, DZ, items, what = regime
    inst, blocks = CASES[name][3:]
    pl = plan(name, B)
    where = f"{name} at B={B}: expected the regime '{what}' (DZ={DZ}, {items} items on {min(items, MAX_PARTIALS)} workgroups), the library plans {pl}"
    assert pl["DZ"] == DZ and pl["ITEMS"] == items and pl["PARTIALS"] == min(items, MAX_PARTIALS), where
    assert (pl["ITEMS"] > pl["PARTIALS"]) == (items > MAX_PARTIALS), where
    assert (pl["COT"], pl["CIT"], pl["S"]) == inst and (pl["CS_BLOCKS"], pl["CG_BLOCKS"]) == blocks, where
    return pl


def elements(name, kind):
    """Three distinct elements of the case: (sm (3,Ds,hs,ws,Cs), bg (3,S*Ds,S*hs,S*ws,Cg)) float32, channel-last, on the CPU.
    kind "int": integers in -2..2 (every product and partial sum an integer: fp32 is exact); "gauss": standard normal."""
    S, Cs, Cg = sides(name)
    d, h, w = SMALL_DHW[S]
    g = torch.Generator().manual_seed(4000 + list(CASES).index(name))
    shapes = (ELEMENTS, d, h, w, Cs), (ELEMENTS, S * d, S * h, S * w, Cg)
    if kind == "int":
        return tuple(torch.randint(-2, 3, s, generator=g).float() for s in shapes)
    assert kind == "gauss", kind
    return tuple(torch.randn(s, generator=g) for s in shapes)


def x_gy(name, sm, bg):
    """(x, gy) of the layer from the kernel's (small, big) pair"""
    return (sm, bg) if CASES[name][0] == DECONV else (bg, sm)


def reduction(sm, bg, S):
    """Per element, in float64: gw[e,cs,cg,k] = sum_o sm[e,o,cs] bgpad[e, S*o + k, cg] and the same sum over absolute values.
    (E,Cs,Cg,3,3,3) each: the layer's own weight layout in every mode (include/mvd.h)."""
    E, d, h, w, Cs = sm.shape
    Cg = bg.shape[-1]
    assert tuple(bg.shape[:4]) == (E, S * d, S * h, S * w)
    bp = torch.nn.functional.pad(bg.double(), (0, 0, 1, 1, 1, 1, 1, 1))
    s2 = sm.double().reshape(E, -1, Cs).transpose(1, 2)
    gw = torch.empty((E, Cs, Cg, 3, 3, 3), dtype=torch.float64)
    sa = torch.empty_like(gw)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                sh = bp[:, kd:kd + S * d:S, kh:kh + S * h:S, kw:kw + S * w:S].reshape(E, -1, Cg)
                gw[:, :, :, kd, kh, kw] = s2 @ sh
                sa[:, :, :, kd, kh, kw] = s2.abs() @ sh.abs()
    return gw, sa


def batch_counts(B):
    """how often element e occurs in a batch whose element b is element b % 3"""
    return np.bincount(np.arange(B) % ELEMENTS, minlength=ELEMENTS)


def batch_reference(per_element, B):
    """sum_e count_e t[e] of a per-element float64 tensor"""
    c = torch.from_numpy(batch_counts(B)).double().reshape(-1, *([1] * (per_element.dim() - 1)))
    return (per_element * c).sum(0)
