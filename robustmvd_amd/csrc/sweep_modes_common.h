// What the generic sweep reduction (sweep_modes.hip) and its backward (sweep_modes_backward.hip) share: ONE definition of the
// sampling position, so that the two compute the same floats and the VJP scatters into exactly the taps the forward gathered.
#pragma once
#include "mvd_common.h"

namespace mvd {

// Sampling position of key pixel (fx, fy) (pixel index + pix_offset) on the plane at `depth` in a source view with [R | t] = M
// (12 floats): (X,Y,Z) = R (fx, fy, 1)^T depth + t, index = X/Z * scale + bias, clamped to [-1, w] x [-1, h] (xhi = w, yhi = h).
// A clamped coordinate puts every tap on the zero border of the staging copy (weight 0 on every interior tap).
struct ReducePos { float ix, iy; };
__device__ __forceinline__ ReducePos reduce_position(const float* __restrict__ M, float fx, float fy, float depth, float scale_x,
                                                     float scale_y, float bias, float xhi, float yhi) {
    const float ax = fmaf(M[0], fx, fmaf(M[1], fy, M[2])), ay = fmaf(M[4], fx, fmaf(M[5], fy, M[6]));
    const float az = fmaf(M[8], fx, fmaf(M[9], fy, M[10]));
    const float X = fmaf(ax, depth, M[3]), Y = fmaf(ay, depth, M[7]), Z = fmaf(az, depth, M[11]);
    float ix = fmaf(X / Z, scale_x, bias), iy = fmaf(Y / Z, scale_y, bias);
    ReducePos P;
    P.ix = __builtin_amdgcn_fmed3f(ix, -1.0f, xhi);  // NaN -> -1: all taps in the zero border
    P.iy = __builtin_amdgcn_fmed3f(iy, -1.0f, yhi);
    return P;
}

}  // namespace mvd
