"""Shared pieces of the merge-mode and normals tests (test_depth_merge_cpu.py, test_hip_depth_merge.py) on fusion_cases' analytic scenes:
the two numpy chains and the bands derived from them alone, and the replay that checks one view's claims against float64 (u,v).
Everything is built once and shared (treat the arrays as read-only)."""
import functools

import numpy as np

import fusion_cases as FC
from robustmvd_amd import depth_fusion as DF

N_VIEWS = len(FC.CAMERAS)
SOURCES = DF.default_sources(N_VIEWS)
ANALYTIC_NORMAL_BOUND = 1e-4  # sin(angle) to scene B's plane normal: 1.1e-5 measured at 96x131, room for float32 depth rounding
MAX_AMBIGUOUS_SHARE = 0.005


def plane_normal():
    """Scene B's normal towards the cameras (all of them are on the origin's side of the plane n.X = 4)."""
    return -FC.PLANE_N / np.linalg.norm(FC.PLANE_N)


def sin_angle(a, b):
    """|a x b| of two (3,...) fields of unit vectors, in float64"""
    return np.linalg.norm(np.cross(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), axis=0), axis=0)


def valid_normal(n):
    return (np.asarray(n) != 0).any(0)


def bit(bits, s):
    return ((bits >> np.uint32(s)) & np.uint32(1)).astype(bool)


@functools.lru_cache(maxsize=None)
def reference(name, H, W):
    """merge_numpy in float64 and in float32 on scene `name`, the per-view fuse_numpy details of fusion_cases.reference, and what the
    device test derives from the two numpy chains alone: the largest gap in (u,v) over the pairs valid in both, the largest
    sin(angle) between the two chains' per-view normals over the pixels valid in both, the bands (four times the gaps, the practice
    of fusion_cases.reference), and whether the normals' validity ever differed."""
    sc = FC.scene(name, H, W)
    kw = dict(images=sc["images"], normals=True, details=True)
    m64 = DF.merge_numpy(sc["depths"], sc["Ks"], sc["Ts"], **kw)
    m32 = DF.merge_numpy(sc["depths"], sc["Ks"], sc["Ts"], dtype=np.float32, **kw)
    views = [FC.reference(name, H, W, i) for i in range(N_VIEWS)]
    gap_uv = gap_n = 0.0
    same_validity = True
    for i, ref in enumerate(views):
        both = ref["f64"]["valid"] & ref["f32"]["valid"]
        for k in ("u", "v"):
            gap_uv = max(gap_uv, float(np.abs(ref["f64"][k] - ref["f32"][k])[both].max()))
        ok64, ok32 = valid_normal(m64["normals"][i]), valid_normal(m32["normals"][i])
        same_validity &= np.array_equal(ok64, ok32)
        ok = ok64 & ok32
        gap_n = max(gap_n, float(sin_angle(m64["normals"][i], m32["normals"][i])[ok].max()))
    return {"scene": sc, "f64": m64, "f32": m32, "views": views, "gap": {"uv": gap_uv, "normal": gap_n},
            "band": {"uv": 4.0 * gap_uv, "normal": 4.0 * gap_n}, "same_normal_validity": bool(same_validity)}


def members(src, bits, mask, u, v, band):
    """The consistent pairs of the emitted pixels of one view: per source s (view src[s]) a dict of py, px (the key pixels), tx, ty
    (the float64 targets, rint: half to even) and `certain`, true where both fractional parts of (u,v) are farther than `band` from
    0.5, so that a chain within the band of the float64 one rounds to the same pixel."""
    ys, xs = np.nonzero(mask)
    out = []
    for s in range(len(src)):
        sel = bit(bits[ys, xs], s)
        py, px = ys[sel], xs[sel]
        uu, vv = u[s][py, px], v[s][py, px]
        amb_u, amb_v = np.abs(uu - np.floor(uu) - 0.5) <= band, np.abs(vv - np.floor(vv) - 0.5) <= band
        out.append({"py": py, "px": px, "u": uu, "v": vv, "tx": np.rint(uu).astype(np.int64), "ty": np.rint(vv).astype(np.int64),
                    "amb_u": amb_u, "amb_v": amb_v, "certain": ~(amb_u | amb_v)})
    return out


def candidates(m, k, H, W):
    """The two or four pixels the k-th pair of members()' entry m may round to"""
    cx = [int(np.floor(m["u"][k])), int(np.floor(m["u"][k])) + 1] if m["amb_u"][k] else [int(m["tx"][k])]
    cy = [int(np.floor(m["v"][k])), int(np.floor(m["v"][k])) + 1] if m["amb_v"][k] else [int(m["ty"][k])]
    return [(y, x) for y in cy for x in cx if 0 <= y < H and 0 <= x < W]


def check_claims(src, bits, mask, u, v, band, before, after):
    """One view's claims against float64 (u,v).  bits, mask: the implementation's own; before, after: dicts view -> claimed map around
    the view's run.  Every certain target is set afterwards, every ambiguous target has one of its two or four candidate pixels set,
    nothing is ever cleared, and no byte outside before | certain | candidates is set.  -> (targets, ambiguous targets)."""
    H, W = mask.shape
    allowed = {j: before[j].astype(bool) for j in set(src)}
    total = ambiguous = 0
    for s, m in enumerate(members(src, bits, mask, u, v, band)):
        j, c = src[s], m["certain"]
        assert after[j][m["ty"][c], m["tx"][c]].all(), f"source {s}: a certain target is not claimed"
        allowed[j][m["ty"][c], m["tx"][c]] = True
        for k in np.nonzero(~c)[0]:
            cands = candidates(m, k, H, W)
            assert any(after[j][y, x] for y, x in cands), f"source {s}: no candidate of an ambiguous target is claimed"
            for y, x in cands:
                allowed[j][y, x] = True
        total += len(c)
        ambiguous += int((~c).sum())
    for j in allowed:
        assert not (before[j].astype(bool) & ~after[j].astype(bool)).any(), f"view {j}: a claim was cleared"
        assert not (after[j].astype(bool) & ~allowed[j]).any(), f"view {j}: a byte outside before | certain | candidates is set"
        assert set(np.unique(after[j])) <= {0, 1}
    return total, ambiguous


def member_means(src, bits, mask, u, v, band, count, key_image, images, key_normal, normals):
    """float64 merged colour and normal over the implementation's own members at their float64 targets -> (rgb (3,H,W), normal
    (3,H,W), clean (H,W)): clean = emitted pixels none of whose targets is ambiguous; the maps are meaningful there only."""
    rgb = np.where(mask.astype(bool), np.asarray(key_image, dtype=np.float64), 0.0)
    nsum = np.where(mask.astype(bool), np.asarray(key_normal, dtype=np.float64), 0.0)
    clean = mask.astype(bool).copy()
    for s, m in enumerate(members(src, bits, mask, u, v, band)):
        j = src[s]
        rgb[:, m["py"], m["px"]] += np.asarray(images[j], dtype=np.float64)[:, m["ty"], m["tx"]]
        nsum[:, m["py"], m["px"]] += np.asarray(normals[j], dtype=np.float64)[:, m["ty"], m["tx"]]
        clean[m["py"][~m["certain"]], m["px"][~m["certain"]]] = False
    rgb /= count.astype(np.float64) + 1.0
    with np.errstate(all="ignore"):
        length = np.linalg.norm(nsum, axis=0)
        nsum = np.where(length > 0, nsum / length, 0.0)
    return rgb, nsum, clean


def check_result(sources, bits, masks, counts, claimed, details, band, min_views=3):
    """check_claims' replay for a whole result that keeps only the final claimed maps.  Per view the claimed map before its run lies
    between `low` (the certain targets of the earlier views) and `high` (those and the ambiguous ones' candidates): no pixel of low is
    emitted, every pixel with enough consistent views outside high is, and the final maps lie between the final low and high.
    bits, masks, counts: the implementation's own, per view; details[i]: float64 fuse_numpy(details=True) of view i.
    -> (targets, ambiguous targets)."""
    H, W = masks[0].shape
    low = [np.zeros((H, W), dtype=bool) for _ in sources]
    high = [np.zeros((H, W), dtype=bool) for _ in sources]
    total = ambiguous = 0
    for i, src in enumerate(sources):
        mask, enough = masks[i].astype(bool), counts[i] >= min_views
        assert not (mask & low[i]).any(), f"view {i}: a pixel claimed by an earlier view is emitted"
        assert not (enough & ~high[i] & ~mask).any(), f"view {i}: an unclaimed pixel with enough consistent views is not emitted"
        assert not (mask & ~enough).any()
        for s, m in enumerate(members(src, bits[i], masks[i], details[i]["u"], details[i]["v"], band)):
            j, c = src[s], m["certain"]
            low[j][m["ty"][c], m["tx"][c]] = True
            high[j][m["ty"][c], m["tx"][c]] = True
            for k in np.nonzero(~c)[0]:
                for y, x in candidates(m, k, H, W):
                    high[j][y, x] = True
            total += len(c)
            ambiguous += int((~c).sum())
    for j in range(len(sources)):
        got = np.asarray(claimed[j]).astype(bool)
        assert not (low[j] & ~got).any(), f"view {j}: a certain target is not claimed at the end"
        assert not (got & ~high[j]).any(), f"view {j}: a byte that is no view's target is set"
    return total, ambiguous
