// The plane-homography family's sampling, defined ONCE: where a key pixel's sample on a depth plane lands in a source view, the
// 2 x 2 cell and bilinear weights of that position, the 4-tap blend, the pending-cell scatter of the VJPs and the running
// variance.  Users: the K3 forward (warp_variance*.hip through warp_variance_common.h: position, cell weights, variance), the K3
// backward (backward.hip scatter, warp_variance_backward_gather.hip gather), the generic sweep reduction (sweep_modes.hip, all
// three kernels) and its backward (sweep_modes_backward.hip).  A VJP scatters into exactly the taps its forward gathered, and
// the scatter and gather forms of one VJP agree bit for bit, because they call the functions below.  Source maps are zero-bordered channel-last copies (h+3, w+3, C), pixel (y, x) at (y+1, x+1), W2 = w + 3.
// (K1's epipolar sweep has its own, different float chains: sweep_epipolar.h.)
#pragma once
#include "mvd_common.h"

namespace mvd {

// Sampling position of key pixel (fx, fy) on the plane at `depth` in a source view with [R | t] = M (12 floats):
// (X,Y,Z) = R (fx, fy, 1)^T depth + t, clamped to [-1, w] x [-1, h] (xhi = w, yhi = h).  A clamped coordinate (NaN -> -1) puts
// every tap on the zero border (weight 0 on every interior tap), like the reference's zero padding.
struct SamplePos { float ix, iy, Z; };  // Z: the sample's depth in the source view (the tile kernel's probe tests its sign)

// K3's two grid scales for a map n pixels a side: folded n/(n-1), EXACT the reference's divisor (n-1)/2.  Callers compute them once.
template <bool EXACT>
__device__ __forceinline__ float grid_scale(int n) {
    return EXACT ? (float)(n - 1) / 2.0f : (float)n / (float)(n - 1);
}

// K3's form, forward and backward (sx = grid_scale<EXACT>(w), sy likewise of h).  Folded: index = X * rcp(Z) * sx - 0.5, i.e.
// homo_warp's normalisation /((W-1)/2) - 1 followed by grid_sample's ((g+1)*W-1)/2 (utils.py:256-264) with 1/Z from v_rcp_f32
// (1 ulp; within 1e-4 px of the exact chain) -- the tuned forward's arithmetic, which K3's backward calls too (<false>), so a
// VJP hits the forward's taps.  EXACT (a template parameter: as a run-time branch its operands stay live through the callers'
// loops, 16+ VGPRs): the reference's own chain, one rounding per step: R @ (x*d, y*d, d) + T (utils.py:246-250), IEEE
// perspective divide, /((W-1)/2) - 1 (:256-257), then grid_sample's unnormalisation.
template <bool EXACT>
__device__ __forceinline__ SamplePos sample_position(const float* __restrict__ M, float fx, float fy, float depth, float sx, float sy,
                                                     float xhi, float yhi) {
    float ix, iy;
    SamplePos P;
    if constexpr (EXACT) {
        const float gx = fx * depth, gy = fy * depth;
        const float X = ((M[0] * gx + M[1] * gy) + M[2] * depth) + M[3];
        const float Y = ((M[4] * gx + M[5] * gy) + M[6] * depth) + M[7];
        P.Z = ((M[8] * gx + M[9] * gy) + M[10] * depth) + M[11];
        ix = unnormalize_coord((X / P.Z) / sx - 1.0f, xhi);
        iy = unnormalize_coord((Y / P.Z) / sy - 1.0f, yhi);
    } else {
        const float ax = fmaf(M[0], fx, fmaf(M[1], fy, M[2])), ay = fmaf(M[4], fx, fmaf(M[5], fy, M[6]));
        const float az = fmaf(M[8], fx, fmaf(M[9], fy, M[10]));
        const float X = fmaf(ax, depth, M[3]), Y = fmaf(ay, depth, M[7]);
        P.Z = fmaf(az, depth, M[11]);
        const float rz = __builtin_amdgcn_rcpf(P.Z);
        ix = fmaf(X * rz, sx, -0.5f);
        iy = fmaf(Y * rz, sy, -0.5f);
    }
    // v_med3_f32: one instruction; with a NaN operand it returns the minimum of the others, i.e. -1 like fminf(fmaxf(NaN, -1), hi)
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
    P.Z = Z;
    P.ix = __builtin_amdgcn_fmed3f(ix, -1.0f, xhi);
    P.iy = __builtin_amdgcn_fmed3f(iy, -1.0f, yhi);
    return P;
}

// Floor, fractions and the four bilinear weights (taps nw, ne, sw, se) of a clamped position; (xf, yf) + 1 is the first tap in the
// bordered map.  Every K3 kernel and sample_cell take them from here; what each makes of (xf, yf) as an offset stays with the
// kernel.  (The products are member functions, not fields, so that a caller's offset arithmetic can stand between the fractions
// and the products as it did when each kernel wrote this out: the backward and sweep kernels compile to the same code as before.)
struct CellWeights {
    float xf, yf, wx, wy, ux, uy;
    __device__ __forceinline__ float w00() const { return ux * uy; }
    __device__ __forceinline__ float w10() const { return wx * uy; }
    __device__ __forceinline__ float w01() const { return ux * wy; }
    __device__ __forceinline__ float w11() const { return wx * wy; }
    __device__ __forceinline__ float4 all() const { return make_float4(ux * uy, wx * uy, ux * wy, wx * wy); }
};
__device__ __forceinline__ CellWeights cell_weights(float ix, float iy) {
    CellWeights c;
    c.xf = floorf(ix); c.yf = floorf(iy);
    c.wx = ix - c.xf; c.wy = iy - c.yf; c.ux = 1.0f - c.wx; c.uy = 1.0f - c.wy;
    return c;
}

// The 2 x 2 cell of a position: offset of its top-left tap (channels c0 .. c0+3) in the bordered map and the four bilinear weights.
struct SampleCell { size_t o; float w00, w10, w01, w11; };
__device__ __forceinline__ SampleCell sample_cell(SamplePos P, int W2, int C, int c0) {
    const CellWeights c = cell_weights(P.ix, P.iy);
    SampleCell L;
    L.o = ((size_t)((int)c.yf + 1) * W2 + ((int)c.xf + 1)) * C + c0;
    L.w00 = c.w00(); L.w10 = c.w10(); L.w01 = c.w01(); L.w11 = c.w11();
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

// variance of key + V sources from their sum s1 and sum of squares s2 (mvsnet.py:135), 4 channels; inv_nv = 1 / (V + 1)
__device__ __forceinline__ float4 variance_finish(float4 s1, float4 s2, float inv_nv) {
    const float mx = s1.x * inv_nv, my = s1.y * inv_nv, mz = s1.z * inv_nv, mw = s1.w * inv_nv;
    return make_float4(fmaf(s2.x, inv_nv, -mx * mx), fmaf(s2.y, inv_nv, -my * my), fmaf(s2.z, inv_nv, -mz * mz),
                       fmaf(s2.w, inv_nv, -mw * mw));
}

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
    __device__ __forceinline__ float4 finish(float inv_nv) const { return variance_finish(s1, s2, inv_nv); }
};

}  // namespace mvd
