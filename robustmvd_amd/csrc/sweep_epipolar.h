// The K1 family's sampling geometry (inverse-depth plane sweep along a key pixel's epipolar line), defined ONCE for the forward
// kernels (sweep_corr.hip: sweep_corr_kernel, sweep_corr_px_kernel, sweep_warp_kernel) and their VJPs (backward.hip:
// sweep_corr_backward_kernel, sweep_warp_backward_kernel).  These float chains decide which taps a sample touches and whether a
// mask entry is 0 or 1: a VJP scatters into exactly the taps its forward gathered because both call the functions below.
// One rounding per operation (the library is built with -ffp-contract=off): keep every expression in the shape it has here.
// Structs travel BY VALUE: passed by reference they reach the register allocator in another order and the K1 kernels come out
// with up to 3 more VGPRs (sweep_corr_px_kernel<8> loses a wave); by value the code equals the hand-inlined form.
#pragma once
#include "mvd_common.h"

namespace mvd {

// EpipolarCoeffs.from_calib (planesweep_corr.py:262-291): 12 scalars per (view, batch element)
struct Epi {
    float a, b, c, e, f, g, h, i, j, k, l, m;
};

__device__ __forceinline__ Epi epipolar(const float* __restrict__ Kk, const float* __restrict__ Ks,
                                        const float* __restrict__ T, int h, int w, int hs, int ws) {
    const float fx = Kk[0] * (float)w, fy = Kk[4] * (float)h, cx = Kk[2] * (float)w, cy = Kk[5] * (float)h;
    const float fxo = Ks[0] * (float)ws, fyo = Ks[4] * (float)hs, cxo = Ks[2] * (float)ws, cyo = Ks[5] * (float)hs;
    const float r11 = T[0], r12 = T[1], r13 = T[2], t1 = T[3];
    const float r21 = T[4], r22 = T[5], r23 = T[6], t2 = T[7];
    const float r31 = T[8], r32 = T[9], r33 = T[10], t3 = T[11];
    Epi E;
    const float A = fxo * r11 + cxo * r31, B = fxo * r12 + cxo * r32;
    E.a = A / fx;
    E.b = B / fy;
    E.c = -(cx * A / fx) - (cy * B / fy) + (fxo * r13 + cxo * r33);
    E.e = fxo * t1 + cxo * t3;
    const float F = fyo * r21 + cyo * r31, G = fyo * r22 + cyo * r32;
    E.f = F / fx;
    E.g = G / fy;
    E.h = -(cx * F / fx) - (cy * G / fy) + (fyo * r23 + cyo * r33);
    E.i = fyo * t2 + cyo * t3;
    E.j = r31 / fx;
    E.k = r32 / fy;
    E.l = -cx * r31 / fx - cy * r32 / fy + r33;
    E.m = t3;
    return E;
}

__device__ __forceinline__ float replace_nonfinite(float v) {
    // us[isinf] = 1e9*sign(us); us[isnan] = 1e9 (planesweep_corr.py:336-338)
    if (isinf(v)) return v > 0.f ? 1e9f : -1e9f;
    if (isnan(v)) return 1e9f;
    return v;
}

// What the ray of key pixel centre (xc, yc) = (x + 0.5, y + 0.5) needs in one source view: u_infs_h = a*x + b*y + c etc.
// (planesweep_corr.py:277-290) and the depth of the pole (:330).
struct SweepRay {
    float u_inf, v_inf, k_inf, z_pole;
};
__device__ __forceinline__ SweepRay sweep_ray(const Epi E, float xc, float yc) {
    SweepRay R;
    R.u_inf = (E.a * xc + E.b * yc) + E.c;
    R.v_inf = (E.f * xc + E.g * yc) + E.h;
    R.k_inf = (E.j * xc + E.k * yc) + E.l;
    R.z_pole = -(E.m / R.k_inf);
    return R;
}

// The sample of a ray on the plane at inverse depth ds: bilinear taps (weights 0 on out-of-image taps), the index of its 2x2
// cell's top-left tap in the zero-bordered source copy (W2 = ws + 3 pixels wide, pixel (yy, xx) at (yy+1, xx+1)) and visibility.
struct SweepSample {
    Taps t;
    int cell;
    bool visible;
};
__device__ __forceinline__ SweepSample sweep_sample(const Epi E, const SweepRay R, float ds, int hs, int ws, int W2) {
    const float fws = (float)ws, fhs = (float)hs;
    const float den = R.k_inf + E.m * ds;
    const float us = replace_nonfinite((R.u_inf + E.e * ds) / den);  // :334
    const float vs = replace_nonfinite((R.v_inf + E.i * ds) / den);  // :343
    const float zs = 1.0f / ds;                                        // :492
    SweepSample G;
    G.visible = (zs > 0.f) && (((R.k_inf > 0.f) && (zs > R.z_pole)) || ((R.k_inf < 0.f) && (zs < R.z_pole)) ||
                               ((R.k_inf == 0.f) && (E.m > 0.f)));  // :499-506
    // warp(): grid = 2*u/w_x - 1 (:87-88), then grid_sample's unnormalisation
    const float ix = unnormalize_coord(2.0f * us / fws - 1.0f, fws);
    const float iy = unnormalize_coord(2.0f * vs / fhs - 1.0f, fhs);
    G.t = bilinear_taps(ix, iy, hs, ws);
    // a cell entirely outside the image has all-zero weights, so which (valid) cell stands in for it does not matter
    const int cx = (int)fminf(fmaxf(floorf(ix), -1.0f), (float)(ws - 1)) + 1;
    const int cy = (int)fminf(fmaxf(floorf(iy), -1.0f), (float)(hs - 1)) + 1;
    G.cell = cy * W2 + cx;
    return G;
}

// Warp-only mask: the sampling mask alone, mask[mask < 0.9999] = 0; mask[mask > 0] = 1 (planesweep_corr.py:101-102).
// WarpOnlyCorr does not take the visibility mask (its forward is called with grids only, :131-133).
__device__ __forceinline__ float sweep_warp_mask(const SweepSample G) { return G.t.inb < 0.9999f ? 0.f : 1.f; }
// Correlation mask: the sampling mask times the visibility mask (:191-193).
__device__ __forceinline__ float sweep_corr_mask(const SweepSample G) { return (G.t.inb < 0.9999f || !G.visible) ? 0.f : 1.f; }

}  // namespace mvd
