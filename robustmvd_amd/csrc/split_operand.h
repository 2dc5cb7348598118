// The arithmetic contract of the split-operand fp16-MFMA kernels (conv3d_split.hip, conv2d_split.hip, deconv3d_split.hip), in
// one place: every fp32 operand is multiplied by an exact power of two and then written as two fp16 terms.
//   activations  a 2^-e   = a_hi + a_lo / f,  e   = exponent(max |x| over the whole input) - 14: the largest magnitude lands in
//                                                   [2^14, 2^15)                                          (split_xscale, split2)
//   weights      w 2^-k_c = w_hi + w_lo / f,  k_c = exponent(max finite |w_c| of output channel c) - 10: [2^10, 2^11), 2^0 for an
//                                                   all-zero channel                    (split_wscale_kernel, split_weight)
// hi = fp16(v), lo = fp16((v - hi) f); v - hi is exact in fp32.  f is the kernel's lo-term factor: 1 where the lo terms stay in
// fp16's range as they are (the implicit-GEMM kernels), 2^11 where the kernel rescales them (conv0_split_kernel).  The epilogues
// multiply by 2^(e + k_c); max |y| over the finite outputs (finite_abs_or_zero) reaches the next layer through raise_absmax
// (mvd_common.h).  Below them, what the two implicit-GEMM files build their kernels from: the vector types, the store of a staged
// item's two terms (split8_store), the hi / lo weight fragment pair (split_wpair) and the three-MFMA product (split_mfma3).
#pragma once
#include "mvd_common.h"

namespace mvd {

// activation scale 2^-e and its inverse, e = exponent(max |x|) - 14 clamped to what a normal fp32 power of two can express
__device__ __forceinline__ void split_xscale_of(unsigned max_bits, float& xsc, float& xsc_inv) {  // max_bits: the bits of max |x|
    const int ex = (int)((max_bits >> 23) & 0xffu) - 127;
    const int e = max(-125, min(125, ex - 14));
    xsc = __uint_as_float((unsigned)(127 - e) << 23);
    xsc_inv = __uint_as_float((unsigned)(127 + e) << 23);
}
// the same from max |x| in device memory, in scalar registers (the main kernels hand xsc to split2 as an SGPR operand)
__device__ __forceinline__ void split_xscale(const float* xamax, float& xsc, float& xsc_inv) {
    split_xscale_of(__builtin_amdgcn_readfirstlane((int)__float_as_uint(*xamax)), xsc, xsc_inv);
}
// two activations -> their packed hi and lo fp16 terms: hi = fp16(a 2^-e) (one rounding: the scaling is exact), t = a 2^-e - hi
// (exact, mixed-precision fma straight from the packed half), lo = fp16(t lo_factor).  5 instructions per pair; the compiler's
// own sequence for the same arithmetic is 10 (it converts every hi twice and back).
__device__ __forceinline__ void split2(float xsc, float a0, float a1, unsigned& hi, unsigned& lo, float lo_factor = 1.0f) {
    unsigned hp, lp;
    float t0, t1;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,0,0]" : "=v"(hp) : "v"(a0), "s"(xsc));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,0,0]" : "+v"(hp) : "v"(a1), "s"(xsc));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(t0) : "v"(a0), "s"(xsc), "v"(hp));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(t1) : "v"(a1), "s"(xsc), "v"(hp));
    asm("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,0,0]" : "=v"(lp) : "v"(t0), "s"(lo_factor));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,0,0]" : "+v"(lp) : "v"(t1), "s"(lo_factor));
    hi = hp;
    lo = lp;
}

// The implicit-GEMM kernels' vectors (conv2d_split.hip, deconv3d_split.hip): an MFMA operand fragment, an accumulator or four
// consecutive floats, 16 bytes of packed halves
typedef _Float16 sph8 __attribute__((ext_vector_type(8)));
typedef float spf4 __attribute__((ext_vector_type(4)));
typedef unsigned int spu4 __attribute__((ext_vector_type(4)));

// the two fp16 terms of eight floats -> the same 16 bytes of a staged patch's hi and lo plane (`plane` bytes apart).  !live: zeros
// instead, for an item outside the volume whose load went out all the same: nothing of what it read gets through, inf and NaN included
__device__ __forceinline__ void split8_store(char* dst, int plane, float xsc, spf4 v0, spf4 v1, bool live = true) {
    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
    split2(xsc, v0[0], v0[1], h0, l0);
    split2(xsc, v0[2], v0[3], h1, l1);
    split2(xsc, v1[0], v1[1], h2, l2);
    split2(xsc, v1[2], v1[3], h3, l3);
    spu4 hv = {h0, h1, h2, h3}, lv = {l0, l1, l2, l3};
    if (!live) { hv = spu4{0, 0, 0, 0}; lv = spu4{0, 0, 0, 0}; }
    *reinterpret_cast<spu4*>(dst) = hv;
    *reinterpret_cast<spu4*>(dst + plane) = lv;
}
// the hi and lo fragment of one K step of the packed weights, w = the lane's 16 bytes of the hi fragment (the lo one follows it)
__device__ __forceinline__ void split_wpair(const char* w, sph8& hi, sph8& lo) {
    hi = *reinterpret_cast<const sph8*>(w);
    lo = *reinterpret_cast<const sph8*>(w + 1024);
}
// acc += w x for a 16 x 16 block and K = 32: w_hi x_hi + w_lo x_hi + w_hi x_lo, in this order, into the one accumulator
__device__ __forceinline__ spf4 split_mfma3(sph8 wh, sph8 wl, sph8 xh, sph8 xl, spf4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl, acc, 0, 0, 0);
}

// the two fp16 terms of a weight already divided by its channel's 2^k_c (the pack kernels)
__device__ __forceinline__ void split_weight(float v, float lo_factor, _Float16& hi, _Float16& lo) {
    hi = (_Float16)v;
    lo = (_Float16)((v - (float)hi) * lo_factor);
}

// wscale[r] = 2^k_c of channel c = r % Cout for the GEMM rows r < rows (several rows may share a channel: the parity classes of a
// transposed layer), 2^0 for the pad rows up to the grid; k_c is clamped to +-100.  w is (Cout, Cin, taps), or (Cin, Cout, taps)
// when transposed.  One workgroup per row.
static __global__ void split_wscale_kernel(const float* __restrict__ w, float* __restrict__ wscale, int Cin, int Cout, int taps, int transposed,
                                           int rows) {
    __shared__ float red[256];
    const int r = blockIdx.x, c = r % Cout;
    float m = 0.f;
    if (r < rows)
        for (int e = threadIdx.x; e < Cin * taps; e += 256) {
            const int ci = e / taps, t = e % taps;
            const float v = fabsf(transposed ? w[((size_t)ci * Cout + c) * taps + t] : w[((size_t)c * Cin + ci) * taps + t]);
            m = (finite_f32(v) && v > m) ? v : m;
        }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int ex = (int)((__float_as_uint(red[0]) >> 23) & 0xffu) - 127;
        const int k = red[0] > 0.f ? max(-100, min(100, ex - 10)) : 0;
        wscale[r] = ldexpf(1.0f, k);
    }
}
// wscale holds rows_padded floats
static inline void split_wscale_launch(const float* w, float* wscale, int Cin, int Cout, int taps, bool transposed, int rows, int rows_padded,
                                       hipStream_t st) {
    hipLaunchKernelGGL(split_wscale_kernel, dim3(rows_padded), dim3(256), 0, st, w, wscale, Cin, Cout, taps, transposed ? 1 : 0, rows);
}

}  // namespace mvd
