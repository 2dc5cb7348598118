"""CPU geometry of the K3 gather backward (numpy, float64): the per-plane homography of homo_warp's sampling positions, the smallest
singular value of its Jacobian over the key pixels whose sample lands inside the source map, and the window radius the gather
needs to find every contribution.  Shared by tests/test_k3_backward_gather_cpu.py and tests/test_hip_k3_backward_gather.py; no
test lives here."""
import numpy as np


def composed(src_proj, key_proj_inv):
    """(3,4) rows of src_proj @ key_proj_inv: (X,Y,Z) = M[:, :3] (x,y,1) d + M[:, 3]."""
    return (np.asarray(src_proj, np.float64) @ np.asarray(key_proj_inv, np.float64))[:3]


def plane_homography(M, d, h, w):
    """3x3 H with (ix, iy, 1) ~ H (x, y, 1): ix = X/Z * w/(w-1) - 0.5 (blocks/utils.py homo_warp's index formula)."""
    Hd = np.array([[M[0, 0] * d, M[0, 1] * d, M[0, 2] * d + M[0, 3]],
                   [M[1, 0] * d, M[1, 1] * d, M[1, 2] * d + M[1, 3]],
                   [M[2, 0] * d, M[2, 1] * d, M[2, 2] * d + M[2, 3]]])
    S = np.array([[w / (w - 1.0), 0, -0.5], [0, h / (h - 1.0), -0.5], [0, 0, 1.0]])
    return S @ Hd


def plane_stats(H, h, w):
    """For one plane: (sigma_min of d(ix,iy)/d(x,y) over the key pixels whose sample lies in (-1,w) x (-1,h), the largest
    |p - round(centre(q))| over every key pixel p and each interior tap q of its sample, number of such pixels).  The centre of q
    is H^-1 q, which is what the gather kernel inverts; (inf, 0, 0) when no sample lands inside."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    X = H[0, 0] * xs + H[0, 1] * ys + H[0, 2]
    Y = H[1, 0] * xs + H[1, 1] * ys + H[1, 2]
    Z = H[2, 0] * xs + H[2, 1] * ys + H[2, 2]
    with np.errstate(all="ignore"):
        ix, iy = X / Z, Y / Z
        inside = np.isfinite(ix) & np.isfinite(iy) & (ix > -1) & (ix < w) & (iy > -1) & (iy < h)
        if not inside.any():
            return np.inf, 0, 0
        # Jacobian of the projective map, analytically
        a = (H[0, 0] - ix * H[2, 0]) / Z
        b = (H[0, 1] - ix * H[2, 1]) / Z
        c = (H[1, 0] - iy * H[2, 0]) / Z
        e = (H[1, 1] - iy * H[2, 1]) / Z
        s1 = a * a + b * b + c * c + e * e
        det = a * e - b * c
        smin = np.sqrt(np.maximum((s1 - np.sqrt(np.maximum(s1 * s1 - 4 * det * det, 0))) / 2, 0))
        sigma = float(smin[inside].min())
        Hi = np.linalg.inv(H)
        need = 0
        xf, yf = np.floor(ix), np.floor(iy)
        for dy in (0, 1):
            for dx in (0, 1):
                qx, qy = xf + dx, yf + dy
                wgt = (1 - np.abs(ix - qx)) * (1 - np.abs(iy - qy))
                ok = inside & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & (wgt > 0)
                if not ok.any():
                    continue
                px = Hi[0, 0] * qx + Hi[0, 1] * qy + Hi[0, 2]
                py = Hi[1, 0] * qx + Hi[1, 1] * qy + Hi[1, 2]
                pz = Hi[2, 0] * qx + Hi[2, 1] * qy + Hi[2, 2]
                ex = np.abs(xs - np.rint(px / pz))[ok].max()
                ey = np.abs(ys - np.rint(py / pz))[ok].max()
                need = max(need, int(ex), int(ey))
    return sigma, need, int(inside.sum())


def pose_set_stats(src_projs, key_proj_inv, depth_values, h, w):
    """src_projs V x (B,4,4), key_proj_inv (B,4,4), depth_values (B,D) -> (sigma_min, radius needed) over all b, views, planes."""
    sigma, need = np.inf, 0
    depth_values = np.asarray(depth_values)
    for P in src_projs:
        for b in range(depth_values.shape[0]):
            M = composed(P[b], key_proj_inv[b])
            for d in depth_values[b]:
                s, n, _ = plane_stats(plane_homography(M, float(d), h, w), h, w)
                sigma, need = min(sigma, s), max(need, n)
    return sigma, need


def window_sigma_limit(radius):
    """The smallest sigma_min a (2 radius + 1)^2 window provably covers: a contribution needs |f(p) - q|_inf < 1, hence
    |p - centre|_inf <= |p - centre|_2 < sqrt(2) / sigma_min, and rounding the centre to a pixel costs another half pixel."""
    return np.sqrt(2.0) / (radius - 0.5)


def mvsnet_projections(sample, h_scale=0.25):
    """bench.py's calibration as MVSNet.projection_matrices makes it: K[:2] *= 0.25, P[:3,:4] = K @ pose[:3,:4], key inverted."""
    out = []
    for K, T in zip(sample["intrinsics"], sample["poses"]):
        Ks = np.asarray(K, np.float64).copy()
        Ks[:2] *= h_scale
        P = np.asarray(T, np.float64).copy()
        P[:3, :4] = Ks @ P[:3, :4]
        out.append(P)
    k = sample["keyview_idx"]
    key_inv = np.linalg.inv(out[k])
    return [p[None] for i, p in enumerate(out) if i != k], key_inv[None]
