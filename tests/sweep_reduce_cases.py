"""The generic plane-sweep reduction's forward (csrc/sweep_modes.hip: sweep_reduce_tile_kernel, sweep_reduce_kernel,
sweep_reduce_nhwc_kernel, sweep_groupcorr_nhwc_kernel<0|1|2>) on the CPU: the table of small cases that
tests/test_hip_sweep_reduce_forward.py runs on the device, their inputs, the float64 reference with its error bound, and a
restatement of the host's dispatch that says which kernel and which of its branches a shape reaches.
tests/test_sweep_reduce_cpu.py pins all of it without a GPU; no test lives here.

INPUTS.  `sweep_inputs` is the generator that tests/test_hip_cvp_mvsnet.py and tests/test_hip_vis_mvsnet.py use too: white-noise
float32 features, a source camera with 3 x the key's focal length, baselines of alternating
sign, one plane at negative depth, planes from 1.5 to 20, per-pixel depths spread by +-50 %.  Two edits of the matrices:
  "z0"            view 0's third row is (1/8, 0, -(7 + pix_offset)/8, 0): Z = (fx - 7 - pix_offset) d / 8 is 0 EXACTLY on the column
                  x = 7 (every operand and the fused multiply-add's result are float32 numbers) and negative left of it, so X / Z is
                  +-inf (NaN where X is 0 too) before the clamp.  tests/test_hip_sweep_grads.py::test_plane_behind_the_source_camera
                  sets (0.1, 0, -0.7, 0), which the kernels' fmaf(0.1f, 7, -0.7f) evaluates to 2.2e-8, not 0: there the
                  quotient is large and finite.
  "out_of_frame"  view 1's X translation + 1e6: every tap of that view is on the zero border.

REFERENCE.  test_sweep_grads_cpu.sweep_reduce_restated (imported): positions in float32 by reduce_positions, i.e. the kernels' own
chain operation by operation (fused multiply-adds rounded once, an IEEE division, the clamp with NaN -> -1), tap weights in
float32 like the kernels' (ix - floor, 1 - fraction, one product each), the gather and the reduction in float64.  With
grid_clamp the positions are clamped once more to `host_bounds`, the float32 arithmetic of mvd_sweep_groupcorr_nhwc_f32.

BOUND.  Per output element K 2^-24 A, nothing else (no atol, nothing from a kernel's output).  With u = 2^-24 and
s_abs = the blend of |taps| (the weights are >= 0 and the same float32 numbers in kernel and reference):
  blend     a w00 rounded, then three fmaf: every term passes <= 4 roundings              |s^ - s| <= 4 u s_abs
  variance  N = V + 1, S1abs = |k| (keysq: k^2) + sum s_abs, S2 = k^2 + sum s_abs^2, A = S2 / N + (S1abs / N)^2
            s1: 4 u from the samples (keysq: 1 u on k k, less) + V additions, each <= u S1abs    <= (V + 4) u S1abs
            s2: s^2 carries 2 x 4 u; k k and V fmaf round once each, partial sums <= S2           <= (V + 9) u S2
            finish: inv_nv = 1.0f / N (u), m = s1 inv_nv (u): m carries V + 6; m m twice that + its own rounding = 2 V + 13;
            s2 inv_nv carries V + 10; the last fmaf rounds the result, |result| <= A: u A
            total <= u ((V + 10) S2 / N + (2 V + 13) (S1abs / N)^2 + A) <= (2 V + 14) u A
  groupcorr q = C / G / 4 quads, A = sum over the group's channels of |k| s_abs
            a quad's dot: k.x s.x rounded, three fmaf (4 u) on samples that carry 4 u: 8 u; the first quad is added to 0.0f
            exactly, the other q - 1 additions round once, partial sums <= A                      <= (q + 7) u A
Products of two or more of these errors are below K u times the first-order sum, K u < 2^-17: one more unit of K covers them.
  K_VARIANCE(V) = 2 V + 15        K_GROUPCORR(q) = q + 8
POSITIONS need no allowance: test_sweep_grads_cpu._fma rounds once (its docstring says how), so reduce_positions gives the
kernels' float32 positions bit for bit, +-inf and NaN included.

CASES (B, C, D, h, w, V, G), each with the paths it is meant to reach (`Case.paths`, checked against `predict` by the CPU test):
`predict` restates the dispatch of mvd_sweep_reduce_f32, mvd_sweep_reduce_nhwc_f32 and mvd_sweep_groupcorr_nhwc_f32.  Every shape
is written in this one order and is the reading of its row that reaches the row's path (plane chunks 8 + 1 need D = 9, chunks
8 + 8 + 3 need D = 19, the 2 x 2 map h = w = 2, the Z = 0 column a map 14 wide).  Seeds are chosen so that
test_sweep_reduce_cpu.test_inputs_exercise_the_edges holds (at least 2 % inside; 3 % but for "views32", whose seed also keeps
the bound of its 32 views, K = 79, below 1e-5 of its small outputs), and "smallest" has D = 4 so that some of its 16 samples
touch the map.  In the tile kernel's float4 store path h w % 4 == 0, so a lane's four pixels are all inside or all outside the
map: "vec4-split" is lanes on both sides of its `po < npix`, 15 and 1 in the "vec4" case."""
import collections
import functools

import numpy as np
import torch

import gen_common as gc
import test_sweep_grads_cpu as RS

f32 = np.float32
U = 2.0 ** -24
NHWC_DPB = 8           # planes per workgroup of the two nhwc kernels
NHWC_MAX_C = 64        # the nhwc entries refuse more channels
CONVENTIONS = {"stretch": dict(pix_offset=0.0, stretch=True), "half": dict(pix_offset=0.5, stretch=False)}
DEPTH_FORMS = ("shared", "per_pixel")
MODES = ("variance", "keysq", "groupcorr")
GRID_CLAMP = float(f32(1.1))  # what the entry point receives for Vis-MVSNet's 1.1

Case = collections.namedtuple("Case", "shape seed edit clamp paths")
CASES = {
    # the tile kernel: two batch elements, 63 pixels (h w % 4 != 0: scalar stores), ppw = 64: the one workgroup per element is partial
    "ragged": Case((2, 16, 5, 7, 9, 2, 4), 7, None, True,
                   ("reduce/tile/scalar-store", "reduce/tile/partial-workgroup", "reduce/tile/batch>1", "reduce/tile/groupcorr",
                    "grid-clamp/side<10")),
    # 60 pixels, h w % 4 == 0, ppw = 64: float4 stores, and lanes on either side of the kernel's `po < npix`
    "vec4": Case((1, 16, 3, 6, 10, 2, 4), 8, None, False, ("reduce/tile/vec4-store", "reduce/tile/vec4-split")),
    # the smallest legal map (2 x 2: w / (w - 1) = 2), one quad, one group: the plain kernel in all three modes.  With one view whose
    # focal length is 3 x the key's, 2 or 3 of the 16 samples touch the map (the seed is chosen so that some do in every form)
    "smallest": Case((1, 4, 4, 2, 2, 1, 1), 32, None, True, ("reduce/plain/units=1/variance", "reduce/plain/units=1/groupcorr")),
    # 3 units: not a power of two; 85 pixels x 3 = 255 live threads in the nhwc kernels
    "units3": Case((1, 12, 4, 9, 13, 3, 3), 10, None, True,
                   ("reduce/plain/not-a-power-of-two", "nhwc-variance/idle-threads", "groupcorr/idle-threads", "groupcorr/G=3")),
    "units6": Case((1, 24, 9, 6, 10, 2, 6), 11, None, False,
                   ("nhwc-variance/units=6", "groupcorr/G=6", "nhwc-variance/chunks=8+1", "groupcorr/chunks=8+1")),
    "one_group": Case((1, 48, 4, 6, 7, 1, 1), 12, None, False, ("groupcorr/QPU=0", "nhwc-variance/units=12")),
    "two_quads": Case((1, 64, 5, 8, 8, 3, 8), 13, None, False, ("groupcorr/QPU=2", "nhwc-variance/units=16")),
    "chunks": Case((1, 32, 19, 9, 13, 2, 8), 14, None, False, ("groupcorr/QPU=1", "nhwc-variance/chunks=8+8+3", "groupcorr/chunks=8+8+3")),
    "views32": Case((1, 8, 3, 3, 5, 32, 2), 34, None, False, ("views=32",)),
    # 65 units: the plain kernel; mvd_sweep_reduce_f32 only
    "wide": Case((1, 260, 2, 4, 5, 1, 5), 11, None, False, ("reduce/plain/units>64", "nhwc/refuses-C>64")),
    "z0": Case((1, 16, 3, 9, 14, 2, 2), 9, "z0", False, ("edit/z0",)),
    "out_of_frame": Case((1, 16, 3, 9, 14, 2, 2), 9, "out_of_frame", False, ("edit/out-of-frame",)),
    # both sides >= 10: the second clamp is the identity
    "clamp_identity": Case((1, 16, 2, 10, 11, 1, 4), 10, None, True, ("grid-clamp/sides>=10",)),
}
REQUIRED_PATHS = (
    "reduce/tile/scalar-store", "reduce/tile/vec4-store", "reduce/tile/vec4-split", "reduce/tile/partial-workgroup", "reduce/tile/batch>1",
    "reduce/tile/groupcorr", "reduce/plain/units=1/variance", "reduce/plain/units=1/groupcorr", "reduce/plain/not-a-power-of-two",
    "reduce/plain/units>64", "nhwc-variance/idle-threads", "nhwc-variance/units=6", "nhwc-variance/units=12", "nhwc-variance/units=16",
    "nhwc-variance/chunks=8+1", "nhwc-variance/chunks=8+8+3", "groupcorr/idle-threads", "groupcorr/G=3", "groupcorr/G=6",
    "groupcorr/QPU=0", "groupcorr/QPU=1", "groupcorr/QPU=2", "groupcorr/chunks=8+1", "groupcorr/chunks=8+8+3", "views=32",
    "nhwc/refuses-C>64", "grid-clamp/side<10", "grid-clamp/sides>=10", "edit/z0", "edit/out-of-frame")
CLAMP_CASES = tuple(name for name, c in CASES.items() if c.clamp)
NHWC_CASES = tuple(name for name, c in CASES.items() if c.shape[1] <= NHWC_MAX_C)


def K_VARIANCE(V):
    return 2 * V + 15


def K_GROUPCORR(quads):
    return quads + 8


# ------------------------------------------------------------------------------------------------ inputs
def sweep_inputs_np(B, C, h, w, D, V, seed):
    """features [key, src_0 ..] (B,C,h,w), [R|t] per view (B,3,4), shared planes (B,D) and per-pixel depths (B,D,h,w), float32:
    hypotheses that push samples across every border and behind the camera: planes from a negative depth over depths close to the
    camera (large parallax: samples leave the map on the side the baseline points to) to far ones, where the source camera's 3 x
    longer focal length pushes the map's rim out through all four borders; per pixel spread by +-50 %."""
    rng = np.random.default_rng(seed)
    feats = [rng.standard_normal((B, C, h, w)).astype(f32) for _ in range(V + 1)]
    K = gc.synthetic_intrinsics(h, w).astype(np.float64)
    Ksrc = K.copy()
    Ksrc[0, 0] *= 3.0
    Ksrc[1, 1] *= 3.0
    Ms = []
    for v in range(V):
        m = []
        for b in range(B):
            P = gc.synthetic_pose(rng, 0.1, 0.3).astype(np.float64)
            P[:3, 3] *= np.array([1, -1, 1]) * (-1) ** (v + b)
            m.append((Ksrc @ P[:3, :4] @ np.linalg.inv(np.vstack([np.hstack([K, np.zeros((3, 1))]), [0, 0, 0, 1]])))[:3, :4])
        Ms.append(np.stack(m).astype(f32))
    planes = np.concatenate(([-0.7], np.geomspace(1.5, 20.0, D - 1))) if D > 1 else np.array([1.0])
    shared = np.stack([planes * (1 + 0.1 * b) for b in range(B)]).astype(f32)
    per_pixel = np.ascontiguousarray(shared[:, :, None, None] * (f32(0.5) + rng.random((B, D, h, w)).astype(f32)))
    return feats, Ms, shared, per_pixel


def sweep_inputs(B, C, h, w, D, V, seed, dev):
    """sweep_inputs_np on a device: (feats, Ms, shared, per_pixel) as tensors"""
    feats, Ms, shared, per_pixel = sweep_inputs_np(B, C, h, w, D, V, seed)
    T = lambda x: torch.from_numpy(x).to(dev)
    return [T(f) for f in feats], [T(m) for m in Ms], T(shared), T(per_pixel)


@functools.lru_cache(maxsize=None)
def case_inputs(name, conv):
    """dict(feats, Ms, shared, per_pixel) of read-only float32 arrays; only the "z0" edit depends on the convention"""
    B, C, D, h, w, V, G = CASES[name].shape
    feats, Ms, shared, per_pixel = sweep_inputs_np(B, C, h, w, D, V, CASES[name].seed)
    if CASES[name].edit == "z0":
        Ms[0][:, 2, :] = np.array([0.125, 0.0, -0.125 * (7 + CONVENTIONS[conv]["pix_offset"]), 0.0], f32)
    elif CASES[name].edit == "out_of_frame":
        Ms[1][:, 0, 3] += f32(1e6)
    for a in feats + Ms + [shared, per_pixel]:
        a.setflags(write=False)
    return dict(feats=feats, Ms=Ms, shared=shared, per_pixel=per_pixel)


def dyadic_inputs(name):
    """The case's features with matrices and planes whose positions are exact in float32 AND float64 under the "half" convention
    (X / Z - 0.5 from x + 0.5): M = [[3, 0, -w, tx], [0, 3, -h, ty], [0, 0, 1, 0]] (the 3 x longer focal length about the
    principal point (w / 2, h / 2)), planes 2^-2 .. 2^3, translations multiples of 1/4: position 3 (fx - w / 2) + w / 2 + tx / d - 0.5.
    The rim leaves through all four borders.  -> (feats, Ms, shared)"""
    B, C, D, h, w, V, G = CASES[name].shape
    Ms = []
    for v in range(V):
        m = np.zeros((B, 3, 4), f32)
        for b in range(B):
            sign = (-1) ** (v + b)
            m[b] = [[3, 0, -w, sign * (0.75 + 0.5 * v)], [0, 3, -h, -sign * (1.25 + 0.25 * b)], [0, 0, 1, 0]]
        Ms.append(m)
    shared = np.stack([2.0 ** ((np.arange(D) + b) % 6 - 2) for b in range(B)]).astype(f32)
    return case_inputs(name, "half")["feats"], Ms, shared


def source_depth(M, depth, h, w, pix_offset, row=2):
    """Z (row 0: X, row 1: Y) of sample_position_div in float32 (its fmaf chain): M (B,3,4), depth (B,D) or (B,D,h,w) -> (B,D,h,w)"""
    M = np.asarray(M, f32)
    B = M.shape[0]
    depth = np.asarray(depth, f32)
    if depth.ndim == 2:
        depth = np.broadcast_to(depth[:, :, None, None], (B, depth.shape[1], h, w))
    fx = (np.arange(w, dtype=f32) + f32(pix_offset))[None, None, None, :]
    fy = (np.arange(h, dtype=f32) + f32(pix_offset))[None, None, :, None]
    m = lambda j: M[:, row, j].reshape(B, 1, 1, 1)
    return RS._fma(RS._fma(m(0), fx, RS._fma(m(1), fy, m(2))), depth, m(3))


def host_bounds(h, w, grid_clamp=GRID_CLAMP):
    """(xlo, xhi, ylo, yhi) as mvd_sweep_groupcorr_nhwc_f32 computes them: grid_sample's un-normalisation ((g + 1) size - 1) / 2 of
    g = -+grid_clamp in float32, one rounding per operation, within [-1, w] x [-1, h]"""
    g, one, two = f32(grid_clamp), f32(1), f32(2)
    lo = lambda n: max(f32(-1), ((one - g) * f32(n) - one) / two)
    hi = lambda n: min(f32(n), ((one + g) * f32(n) - one) / two)
    return lo(w), hi(w), lo(h), hi(h)


# ------------------------------------------------------------------------------------------------ reference and bound
def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def evaluate(feats, Ms, depth, mode, G, conv, bounds=None, dtype=np.float64):
    """sweep_reduce_restated with leaves of `dtype` -> float64 array (B,C,D,h,w), or a list of V (B,G,D,h,w)"""
    leaves = [torch.from_numpy(np.array(f, dtype)) for f in feats]
    with torch.no_grad():
        out = RS.sweep_reduce_restated(leaves[0], leaves[1:], Ms, depth, mode, groups=G, bounds=bounds, **CONVENTIONS[conv])
    return [o.numpy().astype(np.float64) for o in out] if mode == "groupcorr" else out.numpy().astype(np.float64)


def magnitude(feats, Ms, depth, mode, G, conv, bounds=None):
    """A of the module docstring: the same reduction on absolute values, in float64, with the blend of |taps|"""
    key = _t64(feats[0]).abs().unsqueeze(2)
    with torch.no_grad():
        sa = [RS.reduce_sample(_t64(s).abs(), M, depth, bounds=bounds, **CONVENTIONS[conv]) for s, M in zip(feats[1:], Ms)]
        if mode == "groupcorr":
            B, C, D, h, w = sa[0].shape
            return [(key * s).view(B, G, C // G, D, h, w).sum(2).numpy() for s in sa]
        N = len(sa) + 1
        s2 = key * key + sum(s * s for s in sa)
        s1 = (key * key if mode == "keysq" else key) + sum(sa)
        return (s2 / N + (s1 / N) ** 2).numpy()


def bound_of(A, mode, C, G, V):
    if mode == "groupcorr":
        return [K_GROUPCORR(C // G // 4) * U * a for a in A]
    return K_VARIANCE(V) * U * A


@functools.lru_cache(maxsize=None)
def reference(name, conv, form, mode, clamp=False):
    """(want, bound) of a case: float64 arrays (B,C,D,h,w), or lists of V (B,G,D,h,w) for the group correlation; clamp: grid_clamp = 1.1"""
    B, C, D, h, w, V, G = CASES[name].shape
    c = case_inputs(name, conv)
    bounds = host_bounds(h, w) if clamp else None
    args = (c["feats"], c["Ms"], c[form], mode, G, conv, bounds)
    return evaluate(*args), bound_of(magnitude(*args), mode, C, G, V)


# ------------------------------------------------------------------------------------------------ the host's dispatch
def _chunks(D):
    return "+".join(str(n) for n in [NHWC_DPB] * (D // NHWC_DPB) + ([D % NHWC_DPB] if D % NHWC_DPB else []))


def reduce_dispatch(B, C, D, h, w, V, G, mode, out_aligned=True):
    """mvd_sweep_reduce_f32: which kernel, units per pixel, and for the tile kernel the pixels per workgroup, whether the last
    workgroup is partial, the store path of the variance modes (vec4: float4 stores turned through LDS) and, for it, how many
    lanes of the last workgroup store a float4 (`po < npix`) and how many lie past the map; tail_stores counts lanes with only
    some of their four pixels inside, which h w % 4 == 0 rules out"""
    units, npix = (G if mode == "groupcorr" else C // 4), h * w
    if 2 <= units <= 64 and units & (units - 1) == 0 and B <= 65535:
        ppw = 256 // units
        d = dict(kernel="tile", units=units, ppw=ppw, workgroups=-(-npix // ppw), partial=npix % ppw != 0, batch=B)
        if mode != "groupcorr":
            d["vec4"] = npix % 4 == 0 and ppw >= 4 and out_aligned
            if d["vec4"]:
                po = (d["workgroups"] - 1) * ppw + np.arange(0, ppw, 4)  # the last workgroup's lanes of one channel
                d["lanes_float4"], d["lanes_else"] = int((po < npix).sum()), int((po >= npix).sum())
                d["tail_stores"] = int(((po < npix) & (po + 3 >= npix)).sum())
        return d
    why = "units=1" if units == 1 else "units>64" if units > 64 else "not-a-power-of-two"
    threads = B * units * npix
    return dict(kernel="plain", units=units, why=why, workgroups=-(-threads // 256), partial=threads % 256 != 0, batch=B)


def nhwc_dispatch(C, D, h, w, G=None):
    """mvd_sweep_reduce_nhwc_f32 (G None) / mvd_sweep_groupcorr_nhwc_f32: units per pixel, pixels per workgroup, idle threads of
    every workgroup, whether the last one is partial, the plane chunks, and the group correlation's template instance"""
    if C > NHWC_MAX_C:
        return dict(refused=True)
    units = G if G else C // 4
    ppw = 256 // units
    d = dict(refused=False, units=units, ppw=ppw, idle=256 - ppw * units, partial=(h * w) % ppw != 0, chunks=_chunks(D))
    if G:
        d["QPU"] = {1: 1, 2: 2}.get(C // G // 4, 0)
    return d


def predict(name):
    """the set of paths (the strings of REQUIRED_PATHS and more) that the case reaches"""
    B, C, D, h, w, V, G = CASES[name].shape
    paths = set()
    for mode in ("variance", "groupcorr"):  # keysq dispatches like variance
        d = reduce_dispatch(B, C, D, h, w, V, G, mode)
        if d["kernel"] == "plain":
            paths.add(f"reduce/plain/{d['why']}" + (f"/{mode}" if d["why"] == "units=1" else ""))
            continue
        paths.add("reduce/tile/groupcorr" if mode == "groupcorr" else "reduce/tile/vec4-store" if d["vec4"] else "reduce/tile/scalar-store")
        if d["partial"]:
            paths.add("reduce/tile/partial-workgroup")
        if B > 1:
            paths.add("reduce/tile/batch>1")
        if d.get("vec4") and d["lanes_float4"] and d["lanes_else"]:
            paths.add("reduce/tile/vec4-split")
    for tag, d in (("nhwc-variance", nhwc_dispatch(C, D, h, w)), ("groupcorr", nhwc_dispatch(C, D, h, w, G))):
        if d["refused"]:
            paths.add("nhwc/refuses-C>64")
            continue
        paths.add(f"{tag}/{'G' if tag == 'groupcorr' else 'units'}={d['units']}")
        paths.add(f"{tag}/chunks={d['chunks']}")
        if d["idle"]:
            paths.add(f"{tag}/idle-threads")
        if d["partial"]:
            paths.add(f"{tag}/partial-workgroup")
        if "QPU" in d:
            paths.add(f"groupcorr/QPU={d['QPU']}")
    paths.add(f"views={V}")
    if CASES[name].clamp:
        paths.add("grid-clamp/side<10" if min(h, w) < 10 else "grid-clamp/sides>=10")
    if CASES[name].edit:
        paths.add("edit/" + CASES[name].edit.replace("_", "-"))
    return paths
