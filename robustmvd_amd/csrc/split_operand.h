// The split-operand conversion shared by the implicit-GEMM kernels (conv2d_split.hip, deconv3d_split.hip): the activations'
// power-of-two range scale from max |x| and the two fp16 terms of a scaled fp32 value (a 2^-e = a_hi + a_lo).
#pragma once
#include "mvd_common.h"

namespace mvd {

// activation scale 2^-e and its inverse, e = exponent(max |x|) - 14
__device__ __forceinline__ void c2_xscale(const float* xamax, float& xsc, float& xsc_inv) {
    const unsigned mb = __builtin_amdgcn_readfirstlane((int)__float_as_uint(*xamax));
    const int ex = (int)((mb >> 23) & 0xffu) - 127;
    const int e = max(-125, min(125, ex - 14));
    xsc = __uint_as_float((unsigned)(127 - e) << 23);
    xsc_inv = __uint_as_float((unsigned)(127 + e) << 23);
}
// two activations -> their packed hi and lo fp16 terms
__device__ __forceinline__ void c2_split2(float xsc, float a0, float a1, unsigned& hi, unsigned& lo) {
    const float one = 1.0f;
    unsigned hp, lp;
    float t0, t1;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,0,0]" : "=v"(hp) : "v"(a0), "s"(xsc));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,0,0]" : "+v"(hp) : "v"(a1), "s"(xsc));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(t0) : "v"(a0), "s"(xsc), "v"(hp));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(t1) : "v"(a1), "s"(xsc), "v"(hp));
    asm("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,0,0]" : "=v"(lp) : "v"(t0), "s"(one));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,0,0]" : "+v"(lp) : "v"(t1), "s"(one));
    hi = hp;
    lo = lp;
}

}  // namespace mvd
