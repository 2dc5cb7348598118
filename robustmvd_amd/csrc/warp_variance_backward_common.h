// What the two K3 backward implementations share: the scatter kernel (backward.hip, float atomics) and the gather kernels
// (warp_variance_backward_gather.hip, fixed summation order).  Both sample through sweep_homography.h (sample_position<false>,
// sample_cell, sample_blend): the bilinear weights of a key pixel's sample are bit-identical in the two paths, and so is the
// key gradient.
#pragma once
#include "sweep_homography.h"

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

// backward.hip: the scatter kernel over the flagged (b, view) only; adds into gsrc, leaves gkey alone
void launch_warp_variance_backward_flagged(const WarpBwdParams& p, hipStream_t st);

}  // namespace mvd
