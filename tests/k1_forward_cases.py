"""K1 forward on the CPU: the table of small cases that tests/test_hip_k1_forward.py runs on the device, their inputs, and
`path_stats`, a numpy restatement of steps 2 and 3 of sweep_corr_px_kernel (csrc/sweep_corr.hip) on the cells of
test_sweep_grads_cpu.warp_chain (the float32 chain of csrc/sweep_epipolar.h): which cells a pass of 64 planes visits, which of a
cell's four pixels the one or two cells before it already hold, the pixel list and where every dot product lands in it.
tests/test_k1_forward_cpu.py pins all of it without a GPU and asserts that every case is what its label says; no test lives here.

A case: shape (N, C, h, w, hs, ws, S, V), an inverse-depth mode, a pose, the range of the inverse depths and a seed.  The inputs
are those of test_sweep_grads_cpu.sweep_case (the same intrinsics, white-noise float32 features) with pose and range as parameters.
Inverse-depth modes: "shared" (1,S); "batched" (N,S), the second batch element's range 1.25 times the first's; per key pixel
(N,S,h,w): "pixel" (every entry jittered by 5 %), "interleave" (even places from the upper half of the plane list, odd places from
the lower half, jittered by 1 %: every plane leaves its predecessor's cell), "shuffle" (every pixel's planes in an order of its own).
Poses: ("random", rot, trans) is gen_common.synthetic_pose(rng, rot, trans) per view and batch element; ("axial", tx, tz) is the
identity rotation with translation (tx, 0, tz): then k_inf = 1 at every pixel, exactly, and the plane at inverse depth -1 / tz has
den = k_inf + tz * ds = 0 exactly when -1 / tz is a float32 and on the plane list (tz = -0.5, planes 0.5, 0.75 .. 2.5): u and v
are +-inf there, or NaN where their numerator is 0 too, and replace_nonfinite sends them to +-1e9.  With the view's intrinsics equal
to the key's and hs = h the same pose puts iy within a rounding of y, so the rows y = 0 or h - 1 have a tap out of bounds with a
weight of 0 or 1e-7: inb >= 0.9999 on an edge sample."""
import functools

import numpy as np

import torch

import gen_common as gc
from test_sweep_grads_cpu import sweep_corr_restated, sweep_warp_restated, warp_chain

f32 = np.float32
PASS = 64    # planes per pass of the lane = plane loop
STEP = 8     # pixels per step of the pixel list
LIST = 256   # entries of pixlist

# name: (N, C, h, w, hs, ws, S, V), inverse-depth mode, pose, (lowest, highest inverse depth), seed, classes the case claims
CASES = {
    "full_list":     ((1, 256, 2, 17, 32, 160, 64, 1), "interleave", ("random", 0.03, 0.8), (0.4, 50.0), 0, ("full_list",)),
    "monotone":      ((1, 256, 2, 17, 48, 64, 130, 1), "shared", ("random", 0.03, 0.6), (0.4, 50.0), 1,
                      ("monotone", "steps_odd_even", "one_cell", "owner2", "boundary", "tail2", "masked_pass")),
    "chain4":        ((1, 64, 3, 17, 12, 16, 256, 1), "shuffle", ("random", 0.08, 0.2), (0.4, 100.0), 4,
                      ("owner2", "chain4", "revisits", "four_passes", "steps_odd_even", "boundary", "masked_pass")),
    "invisible":     ((1, 128, 3, 18, 12, 20, 70, 3), "shared", ("random", 0.3, 1.5), (0.4, 50.0), 2,
                      ("invisible_kpos", "borders", "tail6", "boundary", "masked_pass")),
    "behind":        ((1, 128, 3, 18, 12, 20, 70, 2), "shared", ("axial", -0.1, -1.5), (0.4, 50.0), 9,
                      ("invisible_kpos", "visibility_decides", "tail6", "boundary")),
    "far_planes":    ((1, 192, 2, 5, 6, 7, 65, 1), "shared", ("random", 0.02, 0.02), (50.0, 1000.0), 3,
                      ("one_cell", "tail1", "boundary")),
    "layout":        ((2, 64, 3, 21, 5, 9, 70, 3), "batched", ("random", 0.08, 0.2), (0.4, 100.0), 5,
                      ("layout", "borders", "edge_hi", "tail6", "boundary")),
    "pixel":         ((2, 128, 4, 5, 6, 7, 67, 2), "pixel", ("random", 0.08, 0.2), (0.4, 100.0), 6, ("owner2",)),
    "turned":        ((1, 64, 3, 18, 12, 20, 64, 1), "shared", ("yaw", 1.75, 1.5, 1.0), (0.7, 50.0), 8,
                      ("invisible_kneg", "borders")),
    "nonfinite":     ((1, 64, 5, 16, 5, 16, 9, 2), "shared", ("axial", -0.25, -0.5), (0.4, 2.0), 7,
                      ("nonfinite", "edge_hi", "borders")),
}
# the geometries that run at every channel count (sweep_corr_px_kernel<8, 16, 24, 32> and sweep_corr_kernel<1 .. 8>)
CHANNEL_GEOMETRIES = ("full_list", "chain4", "invisible", "behind")
PX_CHANNELS = (64, 128, 192, 256)
CELL_CHANNELS = (320, 384, 448, 512)
WARP_GEOMETRIES = ("invisible", "behind", "pixel", "nonfinite")
WARP_CHANNELS = (1, 5, 64)


def case_shape(name):
    return CASES[name][0]


@functools.lru_cache(maxsize=None)
def _geometry(name):
    (N, _, h, w, hs, ws, S, V), mode, pose, (near, far), seed, _ = CASES[name]
    from oracle import mvd_oracle as O
    rng = np.random.default_rng(seed)
    Kk = np.stack([np.array([[0.72, 0, 0.5], [0, 1.28, 0.5], [0, 0, 1]], f32)] * N)
    Ks = [Kk * np.array([[1.0 + 0.05 * v], [1.0 - 0.03 * v], [1.0]], f32) for v in range(V)]
    if pose[0] == "random":
        Ts = [np.stack([gc.synthetic_pose(rng, pose[1], pose[2]) for _ in range(N)]) for _ in range(V)]
    elif pose[0] == "axial":
        Ts = []
        for v in range(V):  # the second view sits on the other side: every plane is in front of it
            T = np.eye(4, dtype=f32)
            T[0, 3], T[2, 3] = (pose[1], pose[2]) if v == 0 else (4 * pose[1], -pose[2])
            Ts.append(np.stack([T] * N))
    else:  # "yaw": turned about the y axis so far that k_inf changes its sign inside the key map
        T = np.eye(4)
        T[:3, :3] = gc.rot_xyz(0.0, pose[1], 0.0)
        T[:3, 3] = -T[:3, :3] @ np.array([pose[2], 0.0, pose[3]])  # the source camera stands at (pose[2], 0, pose[3]) of the key frame
        Ts = [np.stack([T.astype(f32)] * N)] * V
    n = 1 if mode == "shared" else N
    inv = O.compute_sampling_invdepths(f32(near) * (1.0 + 0.25 * np.arange(n)).astype(f32), np.full(n, far, f32), S)
    if mode == "pixel":
        inv = (inv[:, :, None, None] * (1 + 0.05 * rng.uniform(-1, 1, (N, S, h, w)))).astype(f32)
    elif mode == "interleave":
        order = np.empty(S, np.int64)
        order[0::2], order[1::2] = np.arange(S // 2, S), np.arange(S // 2)
        inv = (inv[:, order, None, None] * (1 + 0.01 * rng.uniform(-1, 1, (N, S, h, w)))).astype(f32)
    elif mode == "shuffle":
        inv = np.ascontiguousarray(rng.permuted(np.broadcast_to(inv[:, :, None, None], (N, S, h, w)), axis=1)).astype(f32)
    for a in [Kk, inv] + Ks + Ts:
        a.setflags(write=False)
    return Kk, Ks, Ts, inv


@functools.lru_cache(maxsize=None)
def case_inputs(name, C=None):
    """The case's inputs as test_sweep_grads_cpu.sweep_case gives them (fk, fs, Kk, Ks, Ts, inv, key_size), read-only; the geometry
    does not depend on the channel count C (default: the case's own)."""
    (N, C0, h, w, hs, ws, S, V), *_, seed, _ = CASES[name]
    C = C or C0
    Kk, Ks, Ts, inv = _geometry(name)
    rng = np.random.default_rng([seed, C])
    fk = rng.standard_normal((N, C, h, w)).astype(f32)
    fs = [rng.standard_normal((N, C, hs, ws)).astype(f32) for _ in range(V)]
    for a in [fk] + fs:
        a.setflags(write=False)
    return dict(fk=fk, fs=fs, Kk=Kk, Ks=Ks, Ts=Ts, inv=inv, key_size=(h, w))


def plane_constant_invdepths(name):
    """(inv (N,S), the same values per key pixel (N,S,h,w)) of a case with per-plane inverse depths"""
    (N, _, h, w, _, _, S, _), mode, *_ = CASES[name]
    inv = _geometry(name)[3]
    assert mode in ("shared", "batched")
    inv = np.ascontiguousarray(np.broadcast_to(inv, (N, S)))
    return inv, np.ascontiguousarray(np.broadcast_to(inv[:, :, None, None], (N, S, h, w)))


@functools.lru_cache(maxsize=None)
def chains(name):
    """warp_chain of every view"""
    (N, _, h, w, hs, ws, S, V), *_ = CASES[name]
    Kk, Ks, Ts, inv = _geometry(name)
    return [warp_chain(Kk, Ks[v], Ts[v], inv, h, w, hs, ws) for v in range(V)]


# ------------------------------------------------------------------------------------------------ steps 2 and 3 of the kernel
def pass_lists(cells, W2):
    """Steps 2 and 3 of sweep_corr_px_kernel for the cells of one pass's live planes (lane order): a dict of
    dci (per plane: the index of its cell among the distinct ones), cj (the distinct cells in ray order), in1 / in2 / in3, isnew,
    owner, opos (per cell and tap k: nw, ne, sw, se), idx (per cell and tap: the place of its dot product), pixlist, npix."""
    cells = np.asarray(cells, np.int64)
    first = np.ones(len(cells), bool)
    first[1:] = cells[1:] != cells[:-1]
    dci = np.cumsum(first) - 1
    cj = cells[first]
    n = len(cj)
    offs = np.array([0, 1, W2, W2 + 1], np.int64)
    q = cj[:, None] + offs[None, :]
    lane = np.arange(n)[:, None]

    def back(o):  # the cell o lanes up; lanes below o never look at it
        c = np.full(n, -(1 << 40), np.int64)
        c[o:] = cj[:n - o]
        return c[:, None]

    in_cell = lambda d: (d == 0) | (d == 1) | (d == W2) | (d == W2 + 1)
    pos_of = lambda d: np.where(d == 0, 0, np.where(d == 1, 1, np.where(d == W2, 2, 3)))
    c1, c2, c3 = back(1), back(2), back(3)
    in1 = (lane >= 1) & in_cell(q - c1)
    in2 = in1 & (lane >= 2) & in_cell(q - c2)
    in3 = in2 & (lane >= 3) & in_cell(q - c3)
    isnew = ~in1 | in3
    owner = np.where(isnew, 0, np.where(in2, 2, 1))
    opos = pos_of(np.where(in2, q - c2, q - c1))
    newcnt = isnew.sum(1)
    incl = np.cumsum(newcnt)
    base = incl - newcnt
    npix = int(incl[-1])
    src = np.maximum(lane - owner, 0)                      # the lane whose list places the tap uses: itself, one or two up
    op = np.where(owner == 0, np.arange(4)[None, :], opos)
    below = np.arange(4)[None, None, :] < op[:, :, None]   # (1 << op) - 1
    idx = base[src] + (isnew[src] & below).sum(2)
    pixlist = np.full(npix, -1, np.int64)
    written = np.zeros(npix, np.int64)
    np.add.at(written, idx[isnew], 1)
    pixlist[idx[isnew]] = q[isnew]
    return dict(dci=dci, cj=cj, in1=in1, in2=in2, in3=in3, isnew=isnew, owner=owner, opos=opos, idx=idx, pixlist=pixlist,
                written=written, npix=npix, q=q)


def passes(name):
    """every (n, view, y, x, pass) of a case with the cells of its live planes and the zero-bordered map's width W2"""
    (N, _, h, w, hs, ws, S, V), *_ = CASES[name]
    W2 = ws + 3
    for v, g in enumerate(chains(name)):
        cell = g["cell_y"] * W2 + g["cell_x"]
        for n in range(N):
            for y in range(h):
                for x in range(w):
                    for p, s0 in enumerate(range(0, S, PASS)):
                        yield (n, v, y, x, p), cell[n, s0:s0 + PASS, y, x], W2


@functools.lru_cache(maxsize=None)
def path_stats(name):
    """What the kernel does on a case.  "passes": per (n, view, y, x, pass) a dict of ncell, npix, nsteps, live (planes), new,
    owner1, owner2, in3 (taps of each kind), revisits (cells equal to an earlier, non-adjacent cell of the pass), run_across
    (the pass's first plane has the cell of the plane before it) and masked (no live sample).  Per view: the share of samples
    whose visibility is false, split by the sign of k_inf; the share inside the map that only the visibility term masks; the share with a tap out of bounds; whether samples lie beyond each
    border (their cell is clamped to the zero border); edge samples either side of inb = 0.9999; samples replaced as non-finite."""
    (N, _, h, w, hs, ws, S, V), *_ = CASES[name]
    Kk, Ks, Ts, inv = _geometry(name)
    out = {}
    for key, cells, W2 in passes(name):
        L = pass_lists(cells, W2)
        n, v, y, x, p = key
        g = chains(name)[v]
        s0 = p * PASS
        live = (g["mask"] * g["visible"])[n, s0:s0 + PASS, y, x]
        out[key] = dict(ncell=len(L["cj"]), npix=L["npix"], nsteps=-(-L["npix"] // STEP), live=len(cells),
                        new=int(L["isnew"].sum()), owner1=int((L["owner"] == 1).sum()), owner2=int((L["owner"] == 2).sum()),
                        in3=int(L["in3"].sum()), revisits=int(sum(c in L["cj"][:j] for j, c in enumerate(L["cj"]))),
                        run_across=bool(p > 0 and cells[0] == g["cell_y"][n, s0 - 1, y, x] * W2 + g["cell_x"][n, s0 - 1, y, x]),
                        masked=not live.any())
    views = []
    for v, g in enumerate(chains(name)):
        kpos = np.broadcast_to(g["k_inf"] > 0, g["visible"].shape)
        inv_b = inv if inv.ndim == 4 else np.broadcast_to(inv, (N, S))[:, :, None, None]
        with np.errstate(all="ignore"):
            den = (g["k_inf"] + Ts[v][:, 2, 3].reshape(N, 1, 1, 1) * inv_b).astype(f32)
        edge = ~g["all_in"]
        y_in = (g["cell_y"] >= 1) & (g["cell_y"] <= hs - 1)
        x_in = (g["cell_x"] >= 1) & (g["cell_x"] <= ws - 1)
        gone = g["inb"] == 0
        views.append(dict(
            invisible_kpos=float((~g["visible"] & kpos).mean()), invisible_kneg=float((~g["visible"] & ~kpos).mean()),
            vis_decides=float(((g["mask"] == 1) & ~g["visible"]).mean()), oob=float(edge.mean()), mask_mean=float((g["mask"] * g["visible"]).mean()), warp_mask_mean=float(g["mask"].mean()),
            left=bool((gone & y_in & (g["cell_x"] == 0)).any()), right=bool((gone & y_in & (g["cell_x"] == ws)).any()),
            top=bool((gone & x_in & (g["cell_y"] == 0)).any()), bottom=bool((gone & x_in & (g["cell_y"] == hs)).any()),
            edge_hi=int((edge & (g["inb"] >= f32(0.9999))).sum()), edge_lo=int((edge & (g["inb"] < f32(0.9999))).sum()),
            nonfinite=int(((den == 0) | ~np.isfinite(den)).sum()), nonfinite_at=(den == 0) | ~np.isfinite(den)))
    return dict(passes=out, views=views)


def summary(name):
    """the counts that the classes are decided on (tests/test_k1_forward_cpu.py prints and asserts them)"""
    st = path_stats(name)
    P = list(st["passes"].values())
    full = [p for p in P if p["live"] == PASS]
    return dict(
        max_cells=max(p["ncell"] for p in P), max_npix=max(p["npix"] for p in P), max_steps=max(p["nsteps"] for p in P),
        full_lists=sum(p["ncell"] == PASS and p["npix"] == LIST for p in P),
        long_paths=sum(p["ncell"] >= 48 and p["nsteps"] >= 16 for p in P),
        odd_steps=sum(p["nsteps"] >= 3 and p["nsteps"] % 2 == 1 for p in P),
        even_steps=sum(p["nsteps"] >= 3 and p["nsteps"] % 2 == 0 for p in P),
        one_step=sum(p["npix"] <= STEP for p in P), one_cell=sum(p["ncell"] == 1 for p in full),
        owner1=sum(p["owner1"] for p in P), owner2=sum(p["owner2"] for p in P), in3=sum(p["in3"] for p in P),
        revisit_passes=sum(p["revisits"] > 0 for p in P), runs_across=sum(p["run_across"] for p in P),
        masked_passes=sum(p["masked"] for p in P), odd_cells=sum(p["ncell"] % 2 == 1 for p in P),
        even_cells=sum(p["ncell"] % 2 == 0 for p in P), passes=len(P), views=st["views"])


# ------------------------------------------------------------------------------------------------ one-hot sources
def one_hot_picks(name, per_kind=3):
    """Source pixels for the one-hot runs, from the restated lists: per kind ("owner1", "owner2": the dot product is looked up in
    the list places of the cell one / two back; "in3": reloaded at the end of a chain of four; "last": the list's last place) up
    to per_kind picks (n, view, y, x, pass, cell index, tap, kind, (yy, xx) source pixel, planes that read it through that cell),
    each from a pass of its own with the most cells.  A pick lies inside the source map and at least one of its planes is live with a
    weight above 0.1 on the tap, so that the reference output there is of the size of a dot product."""
    (N, _, h, w, hs, ws, S, V), *_ = CASES[name]
    found = {"owner1": [], "owner2": [], "in3": [], "last": []}
    for (n, v, y, x, p), cells, W2 in passes(name):
        L = pass_lists(cells, W2)
        g = chains(name)[v]
        s0 = p * PASS
        live = (g["mask"] * g["visible"])[n, s0:s0 + PASS, y, x] > 0
        kinds = {"owner1": (L["owner"] == 1), "owner2": (L["owner"] == 2), "in3": L["in3"],
                 "last": L["isnew"] & (L["idx"] == L["npix"] - 1)}
        for kind, sel in kinds.items():
            for j, k in zip(*np.nonzero(sel)):
                yy, xx = int(L["q"][j, k]) // W2 - 1, int(L["q"][j, k]) % W2 - 1
                planes = s0 + np.nonzero(L["dci"] == j)[0]
                strong = live[planes - s0] & (g["wts"][k][n, planes, y, x] > 0.1)
                if 0 <= yy < hs and 0 <= xx < ws and strong.any():
                    found[kind].append((L["npix"], (n, v, y, x, p, int(j), int(k), kind, (yy, xx), tuple(int(s) for s in planes[strong]))))
                    break
    picks = []
    for kind, lst in found.items():
        lst.sort(key=lambda t: -t[0])
        picks += [t[1] for t in lst[:per_kind]]
    return picks


def readers(name, view, n, yy, xx):
    """(N,S,h,w) bool: the samples of the view with a tap on source pixel (yy, xx) of batch element n"""
    (N, _, h, w, hs, ws, S, V), *_ = CASES[name]
    g = chains(name)[view]
    hit = np.zeros((N, S, h, w), bool)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        hit[n] |= (g["cell_y"][n] - 1 + dy == yy) & (g["cell_x"][n] - 1 + dx == xx)
    return hit


def one_hot_sources(name, C, pick):
    """the case's source maps, zero except at the pick's pixel (all channels) of its view and batch element"""
    n, v, *_, (yy, xx), _ = pick
    c = case_inputs(name, C)
    fs = [np.zeros_like(f) for f in c["fs"]]
    fs[v][n, :, yy, xx] = c["fs"][v][n, :, yy, xx]
    return fs


# ------------------------------------------------------------------------------------------------ references
def corr_scale(C):
    """1 / sqrt(C) as the kernel receives it: rounded to float32"""
    return float(f32(1.0 / float(C) ** 0.5))


def _tensor(a, dt):
    return torch.from_numpy(np.array(a, dt))


@functools.lru_cache(maxsize=None)
def references(name, C=None, pick=None):
    """sweep_corr_restated of the case (float32 positions; blend and sum in the leaves' dtype) -> per view (want, e, mask): the
    float64 evaluation, the largest deviation of the float32 evaluation from it, and the 0/1 mask.  pick: a one-hot run."""
    c = case_inputs(name, C)
    fs = c["fs"] if pick is None else one_hot_sources(name, C, pick)
    outs = {}
    for dt in (np.float64, f32):
        with torch.no_grad():
            corrs, masks = sweep_corr_restated(_tensor(c["fk"], dt), [_tensor(f, dt) for f in fs], c["Kk"], c["Ks"], c["Ts"], c["inv"],
                                               corr_scale(c["fk"].shape[1]))
        outs[dt] = [x.numpy().astype(np.float64) for x in corrs]
    return [(w64, float(np.abs(w32 - w64).max()), m) for w64, w32, m in zip(outs[np.float64], outs[f32], masks)]


@functools.lru_cache(maxsize=None)
def warp_references(name, C, normalize_after):
    """the same for sweep_warp_restated on the case's geometry with C-channel source maps: per view (want (N,S,C,h,w), e, mask)"""
    c = case_inputs(name, C)
    outs = {}
    for dt in (np.float64, f32):
        with torch.no_grad():
            warped, masks = sweep_warp_restated([_tensor(f, dt) for f in c["fs"]], c["Kk"], c["Ks"], c["Ts"], c["inv"], c["key_size"],
                                                bool(normalize_after))
        outs[dt] = [x.numpy().astype(np.float64) for x in warped]
    return [(w64, float(np.abs(w32 - w64).max()), m) for w64, w32, m in zip(outs[np.float64], outs[f32], masks)]
