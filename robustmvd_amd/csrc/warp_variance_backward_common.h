// What the two K3 backward implementations share: the scatter kernel (backward.hip, float atomics) and the gather kernels
// (warp_variance_backward_gather.hip, fixed summation order).  One definition of the sampling position, so that both compute the
// same floats: the bilinear weights of a key pixel's sample are bit-identical in the two paths, and so is the key gradient.
#pragma once
#include "mvd_common.h"

namespace mvd {

struct WarpBwdParams {
    ViewPtrs src;            // V x (B,h+3,w+3,C) zero-bordered channel-last source features
    ViewOutPtrs gsrc;        // V x (B,h+3,w+3,C) zero-initialised gradient maps (border entries receive the padding's share)
    const float* key;        // (B,h+3,w+3,C)
    float* gkey;             // (B,h+3,w+3,C), interior written (not accumulated)
    const float* M;          // (V,B,12) composed transforms
    const float* depth;      // (B,D)
    const float* gvar;       // (B,D,h,w,C) channel-last
    int B, C, D, h, w, V;
    // the gather path's fallback launch only: (B,V) flags, non-zero = this view of this batch element is scattered; the number of
    // such (b, view) is added to *fallback_count (may be NULL)
    const int* flags;
    int* fallback_count;
};

// backward.hip: M[v][b] = rows 0..2 of src_proj[v][b] @ key_proj_inv[b], the forward's fmaf chain
void launch_compose_transforms_bwd(const ViewPtrs& proj, const float* key_proj_inv, int B, int V, float* M, hipStream_t st);
// backward.hip: the scatter kernel over the flagged (b, view) only; adds into gsrc, leaves gkey alone
void launch_warp_variance_backward_flagged(const WarpBwdParams& p, hipStream_t st);

// Sampling position of key pixel (fx, fy) on the plane at `depth` in a source view with composed transform M (12 floats): the folded
// form of the forward kernel, clamped to [-1, w] x [-1, h] (xhi = w, yhi = h).  A clamped coordinate gives weight 0 to every
// interior tap, like the reference's zero padding.
struct BwdPos { float ix, iy; };
__device__ __forceinline__ BwdPos bwd_position(const float* __restrict__ M, float fx, float fy, float depth, float sx, float sy,
                                               float xhi, float yhi) {
    const float ax = fmaf(M[0], fx, fmaf(M[1], fy, M[2])), ay = fmaf(M[4], fx, fmaf(M[5], fy, M[6]));
    const float az = fmaf(M[8], fx, fmaf(M[9], fy, M[10]));
    const float X = fmaf(ax, depth, M[3]), Y = fmaf(ay, depth, M[7]), Z = fmaf(az, depth, M[11]);
    const float rz = __builtin_amdgcn_rcpf(Z);
    float ix = fmaf(X * rz, sx, -0.5f), iy = fmaf(Y * rz, sy, -0.5f);
    BwdPos P;
    P.ix = __builtin_amdgcn_fmed3f(ix, -1.0f, xhi);
    P.iy = __builtin_amdgcn_fmed3f(iy, -1.0f, yhi);
    return P;
}

// The 2 x 2 cell of a position: offset of its top-left tap (channel quad q) in the bordered map and the four bilinear weights.
struct BwdLoc { size_t o; float w00, w10, w01, w11; };
__device__ __forceinline__ BwdLoc bwd_cell(BwdPos P, int W2, int C, int q) {
    const float xf = floorf(P.ix), yf = floorf(P.iy);
    const float wx = P.ix - xf, wy = P.iy - yf, ux = 1.0f - wx, uy = 1.0f - wy;
    BwdLoc L;
    L.o = ((size_t)((int)yf + 1) * W2 + ((int)xf + 1)) * C + q * 4;
    L.w00 = ux * uy; L.w10 = wx * uy; L.w01 = ux * wy; L.w11 = wx * wy;
    return L;
}
__device__ __forceinline__ BwdLoc bwd_locate(const float* __restrict__ M, float fx, float fy, float depth, float sx, float sy,
                                             float xhi, float yhi, int W2, int C, int q) {
    return bwd_cell(bwd_position(M, fx, fy, depth, sx, sy, xhi, yhi), W2, C, q);
}
__device__ __forceinline__ float4 bwd_sample(const float* __restrict__ f, const BwdLoc& L, int W2, int C) {
    const float4 a = *reinterpret_cast<const float4*>(f + L.o), bq = *reinterpret_cast<const float4*>(f + L.o + C);
    const float4 c = *reinterpret_cast<const float4*>(f + L.o + (size_t)W2 * C), d = *reinterpret_cast<const float4*>(f + L.o + (size_t)W2 * C + C);
    return make_float4(fmaf(d.x, L.w11, fmaf(c.x, L.w01, fmaf(bq.x, L.w10, a.x * L.w00))),
                       fmaf(d.y, L.w11, fmaf(c.y, L.w01, fmaf(bq.y, L.w10, a.y * L.w00))),
                       fmaf(d.z, L.w11, fmaf(c.z, L.w01, fmaf(bq.z, L.w10, a.z * L.w00))),
                       fmaf(d.w, L.w11, fmaf(c.w, L.w01, fmaf(bq.w, L.w10, a.w * L.w00))));
}

// four no-return float atomics (global_atomic_add_f32) on consecutive addresses: the scatter kernels' flush
__device__ __forceinline__ void atomic_add4(float* p, float4 v) {
    unsafeAtomicAdd(p + 0, v.x); unsafeAtomicAdd(p + 1, v.y); unsafeAtomicAdd(p + 2, v.z); unsafeAtomicAdd(p + 3, v.w);
}

}  // namespace mvd
