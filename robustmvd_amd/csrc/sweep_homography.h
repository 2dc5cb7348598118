// The plane-homography family's sampling, defined ONCE: where a key pixel's sample on a depth plane lands in a source view, the
// 2 x 2 cell and bilinear weights of that position, the 4-tap blend, the pending-cell scatter of the VJPs and the running
// variance.  Users: the K3 backward (backward.hip scatter, warp_variance_backward_gather.hip gather), the generic sweep
// reduction (sweep_modes.hip, all three kernels) and its backward (sweep_modes_backward.hip).  A VJP scatters into exactly
// the taps its forward gathered, and the scatter and gather forms of one VJP agree bit for bit, because they call the functions
// below.  Source maps are zero-bordered channel-last copies (h+3, w+3, C), pixel (y, x) at (y+1, x+1), W2 = w + 3.
// (K1's epipolar sweep has its own, different float chains: sweep_epipolar.h.)
#pragma once
#include "mvd_common.h"

namespace mvd {

// Sampling position of key pixel (fx, fy) on the plane at `depth` in a source view with [R | t] = M (12 floats):
// (X,Y,Z) = R (fx, fy, 1)^T depth + t, clamped to [-1, w] x [-1, h] (xhi = w, yhi = h).  A clamped coordinate (NaN -> -1) puts
// every tap on the zero border (weight 0 on every interior tap), like the reference's zero padding.
struct SamplePos { float ix, iy; };

// K3's form, index = X * rcp(Z) * sx - 0.5: the folded arithmetic of the tuned forward tile kernel (warp_variance_tile.hip,
// v_rcp_f32, 1 ulp), which K3's backward must reproduce to hit the forward's taps.
__device__ __forceinline__ SamplePos sample_position_rcp(const float* __restrict__ M, float fx, float fy, float depth, float sx,
                                                         float sy, float xhi, float yhi) {
    const float ax = fmaf(M[0], fx, fmaf(M[1], fy, M[2])), ay = fmaf(M[4], fx, fmaf(M[5], fy, M[6]));
    const float az = fmaf(M[8], fx, fmaf(M[9], fy, M[10]));
    const float X = fmaf(ax, depth, M[3]), Y = fmaf(ay, depth, M[7]), Z = fmaf(az, depth, M[11]);
    const float rz = __builtin_amdgcn_rcpf(Z);
    float ix = fmaf(X * rz, sx, -0.5f), iy = fmaf(Y * rz, sy, -0.5f);
    SamplePos P;
    P.ix = __builtin_amdgcn_fmed3f(ix, -1.0f, xhi);
    P.iy = __builtin_amdgcn_fmed3f(iy, -1.0f, yhi);
    return P;
}

// The generic reduction's form, index = X / Z * scale + bias: a correctly rounded division and the caller's pixel-centre
// convention (scale, bias), because its consumers are checked against references that divide (sweep_modes.hip's header).
__device__ __forceinline__ SamplePos sample_position_div(const float* __restrict__ M, float fx, float fy, float depth, float scale_x,
                                                         float scale_y, float bias, float xhi, float yhi) {
    const float ax = fmaf(M[0], fx, fmaf(M[1], fy, M[2])), ay = fmaf(M[4], fx, fmaf(M[5], fy, M[6]));
    const float az = fmaf(M[8], fx, fmaf(M[9], fy, M[10]));
    const float X = fmaf(ax, depth, M[3]), Y = fmaf(ay, depth, M[7]), Z = fmaf(az, depth, M[11]);
    float ix = fmaf(X / Z, scale_x, bias), iy = fmaf(Y / Z, scale_y, bias);
    SamplePos P;
    P.ix = __builtin_amdgcn_fmed3f(ix, -1.0f, xhi);
    P.iy = __builtin_amdgcn_fmed3f(iy, -1.0f, yhi);
    return P;
}

// The 2 x 2 cell of a position: offset of its top-left tap (channels c0 .. c0+3) in the bordered map and the four bilinear weights.
struct SampleCell { size_t o; float w00, w10, w01, w11; };
__device__ __forceinline__ SampleCell sample_cell(SamplePos P, int W2, int C, int c0) {
    const float xf = floorf(P.ix), yf = floorf(P.iy);
    const float wx = P.ix - xf, wy = P.iy - yf, ux = 1.0f - wx, uy = 1.0f - wy;
    SampleCell L;
    L.o = ((size_t)((int)yf + 1) * W2 + ((int)xf + 1)) * C + c0;
    L.w00 = ux * uy; L.w10 = wx * uy; L.w01 = ux * wy; L.w11 = wx * wy;
    return L;
}
// bilinear blend of the cell's four taps, 4 channels
__device__ __forceinline__ float4 sample_blend(const float* __restrict__ f, const SampleCell L, int W2, int C) {
    const float4 a = *reinterpret_cast<const float4*>(f + L.o), bq = *reinterpret_cast<const float4*>(f + L.o + C);
    const float4 c = *reinterpret_cast<const float4*>(f + L.o + (size_t)W2 * C), d = *reinterpret_cast<const float4*>(f + L.o + (size_t)W2 * C + C);
    return make_float4(fmaf(d.x, L.w11, fmaf(c.x, L.w01, fmaf(bq.x, L.w10, a.x * L.w00))),
                       fmaf(d.y, L.w11, fmaf(c.y, L.w01, fmaf(bq.y, L.w10, a.y * L.w00))),
                       fmaf(d.z, L.w11, fmaf(c.z, L.w01, fmaf(bq.z, L.w10, a.z * L.w00))),
                       fmaf(d.w, L.w11, fmaf(c.w, L.w01, fmaf(bq.w, L.w10, a.w * L.w00))));
}

// four no-return float atomics (global_atomic_add_f32) on consecutive addresses
__device__ __forceinline__ void atomic_add4(float* p, float4 v) {
    unsafeAtomicAdd(p + 0, v.x); unsafeAtomicAdd(p + 1, v.y); unsafeAtomicAdd(p + 2, v.z); unsafeAtomicAdd(p + 3, v.w);
}

// The scatter kernels' ONE pending 2 x 2 cell of tap gradients: consecutive planes of a pixel mostly sample the same source cell
// (the forward kernel's tap reuse), so the four taps' shares are summed in registers and go out as atomics only when the cell
// changes, and at the end of a chunk (flush) — about 2.5x fewer atomics at the headline poses.
struct PendingCell {
    static constexpr size_t NONE = ~(size_t)0;
    int W2, C;
    size_t o = NONE;
    float4 t00 = make_float4(0, 0, 0, 0), t10 = t00, t01 = t00, t11 = t00;
    __device__ __forceinline__ PendingCell(int W2_, int C_) : W2(W2_), C(C_) {}
    __device__ __forceinline__ void flush(float* __restrict__ gmap) const {
        if (o == NONE) return;
        float* go = gmap + o;
        atomic_add4(go, t00);
        atomic_add4(go + C, t10);
        atomic_add4(go + (size_t)W2 * C, t01);
        atomic_add4(go + (size_t)W2 * C + C, t11);
    }
    // adds the sample's gradient gx, times its four weights, to cell L of gradient map gmap.  (The zero start of the four taps and L
    // by reference are what the hand-written form had: with them the K3 scatter compiles to the same code, without them to a
    // shorter kernel that measured 2.4 % slower, profiles/sweep_geometry_refactor.txt.)
    __device__ __forceinline__ void add(float* __restrict__ gmap, const SampleCell& L, float4 gx) {
        if (L.o != o) {
            flush(gmap);
            o = L.o;
            t00 = make_float4(gx.x * L.w00, gx.y * L.w00, gx.z * L.w00, gx.w * L.w00);
            t10 = make_float4(gx.x * L.w10, gx.y * L.w10, gx.z * L.w10, gx.w * L.w10);
            t01 = make_float4(gx.x * L.w01, gx.y * L.w01, gx.z * L.w01, gx.w * L.w01);
            t11 = make_float4(gx.x * L.w11, gx.y * L.w11, gx.z * L.w11, gx.w * L.w11);
        } else {
            t00.x = fmaf(gx.x, L.w00, t00.x); t00.y = fmaf(gx.y, L.w00, t00.y); t00.z = fmaf(gx.z, L.w00, t00.z); t00.w = fmaf(gx.w, L.w00, t00.w);
            t10.x = fmaf(gx.x, L.w10, t10.x); t10.y = fmaf(gx.y, L.w10, t10.y); t10.z = fmaf(gx.z, L.w10, t10.z); t10.w = fmaf(gx.w, L.w10, t10.w);
            t01.x = fmaf(gx.x, L.w01, t01.x); t01.y = fmaf(gx.y, L.w01, t01.y); t01.z = fmaf(gx.z, L.w01, t01.z); t01.w = fmaf(gx.w, L.w01, t01.w);
            t11.x = fmaf(gx.x, L.w11, t11.x); t11.y = fmaf(gx.y, L.w11, t11.y); t11.z = fmaf(gx.z, L.w11, t11.z); t11.w = fmaf(gx.w, L.w11, t11.w);
        }
    }
};

// Running variance over key + V sources (mvsnet.py:124-135), 4 channels: s1 = sum, s2 = sum of squares.  keysq: the reference's
// aliasing in CVP-MVSNet (MVD_REDUCE_VARIANCE_KEYSQ), where both sums start from key^2.
struct VarianceSums {
    float4 s1, s2;
    __device__ __forceinline__ VarianceSums(float4 k, bool keysq) {
        s2 = make_float4(k.x * k.x, k.y * k.y, k.z * k.z, k.w * k.w);
        s1 = make_float4(keysq ? s2.x : k.x, keysq ? s2.y : k.y, keysq ? s2.z : k.z, keysq ? s2.w : k.w);  // (a select of values, not of objects)
    }
    __device__ __forceinline__ void add(float4 sv) {
        s1.x += sv.x; s1.y += sv.y; s1.z += sv.z; s1.w += sv.w;
        s2.x = fmaf(sv.x, sv.x, s2.x); s2.y = fmaf(sv.y, sv.y, s2.y);
        s2.z = fmaf(sv.z, sv.z, s2.z); s2.w = fmaf(sv.w, sv.w, s2.w);
    }
    __device__ __forceinline__ float4 finish(float inv_nv) const {  // inv_nv = 1 / (V + 1)
        const float mx = s1.x * inv_nv, my = s1.y * inv_nv, mz = s1.z * inv_nv, mw = s1.w * inv_nv;
        return make_float4(fmaf(s2.x, inv_nv, -mx * mx), fmaf(s2.y, inv_nv, -my * my), fmaf(s2.z, inv_nv, -mz * mz),
                           fmaf(s2.w, inv_nv, -mw * mw));
    }
};

}  // namespace mvd
