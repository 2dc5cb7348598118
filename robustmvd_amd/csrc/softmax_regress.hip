// K5 — softmax over the depth axis + soft-argmin depth + 4-bin confidence (Path B).
// Replaces F.softmax + depth_regression + avg_pool3d/gather of MVSNet.forward
// (rmvd/models/mvsnet.py:139-160, rmvd/models/blocks/utils.py:271-274).
// Lanes along x: every load of a depth plane row is a coalesced 256-B segment.  One sweep over D (chunked online softmax, D split
// over the 4 waves of a workgroup) plus a 4-plane window re-read for the confidence; the cost volume is D*h*w*4 B (57 MB at the
// headline shape).
#include "mvd_common.h"

namespace mvd {

// STATS (the training forward, mvd_softmax_regress_stats_f32): also stores the per-pixel max M and 1 / sum_d exp(c_d - M) that
// the VJP kernel below needs; the depth and confidence arithmetic is the same code either way (bit-identical outputs).
// A workgroup = 64 pixels x 4 waves; wave k sweeps depth planes [k Dq, (k+1) Dq) (Dq = D / 4 rounded up to a multiple of 8) with the
// chunked online softmax, the four partial results are merged through LDS in the fixed order k = 0 .. 3.  (One lane per pixel over
// all D planes left 216 workgroups of latency-bound lanes on 256 CUs at the headline shape: 45 us for a 57 MB read.)
template <bool STATS>
__global__ void __launch_bounds__(256) softmax_regress_kernel(const float* __restrict__ cost,
                                                              const float* __restrict__ depth_values, int D,
                                                              long long hw, float* __restrict__ depth_out,
                                                              float* __restrict__ conf_out, float* __restrict__ stats_out) {
    __shared__ float part[4][4][64];  // [wave][m, se, sd, si][lane]
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long pix = (long long)blockIdx.x * 64 + lane;
    const bool live = pix < hw;
    const float* c = cost + (long long)b * D * hw + (live ? pix : 0);
    const float* dv = depth_values + (long long)b * D;

    constexpr int CH = 8;
    const int Dq = ((D + 3) / 4 + CH - 1) / CH * CH;
    const int dbeg = wv * Dq, dend = min(D, dbeg + Dq);
    float m = -INFINITY, se = 0.f, sd = 0.f, si = 0.f;
    for (int d0 = dbeg; d0 < dend; d0 += CH) {
        float v[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) v[k] = d0 + k < dend ? c[(long long)(d0 + k) * hw] : -INFINITY;
        float cm = v[0];
#pragma unroll
        for (int k = 1; k < CH; ++k) cm = fmaxf(cm, v[k]);
        if (cm > m) {
            const float r = expf(m - cm);  // exp(-inf) = 0 on the first chunk
            se *= r; sd *= r; si *= r;
            m = cm;
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            if (d0 + k < dend) {
                const float e = expf(v[k] - m);
                se += e;
                sd = fmaf(e, dv[d0 + k], sd);
                si = fmaf(e, (float)(d0 + k), si);
            }
        }
    }
    part[wv][0][lane] = m; part[wv][1][lane] = se; part[wv][2][lane] = sd; part[wv][3][lane] = si;
    __syncthreads();
    if (wv != 0 || !live) return;
    // merge: common max, partial sums rescaled to it (a slice without planes has m = -inf and sums 0: exp(-inf) * 0 = 0)
    float M = part[0][0][lane];
#pragma unroll
    for (int k = 1; k < 4; ++k) M = fmaxf(M, part[k][0][lane]);
    se = 0.f; sd = 0.f; si = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float mk = part[k][0][lane];
        const float r = mk == -INFINITY ? 0.f : expf(mk - M);
        se = fmaf(part[k][1][lane], r, se);
        sd = fmaf(part[k][2][lane], r, sd);
        si = fmaf(part[k][3][lane], r, si);
    }
    // depth = sum_d p_d depth_d, expected index = sum_d p_d d (mvsnet.py:140-141,151-154) with p_d = e_d / se
    depth_out[(long long)b * hw + pix] = sd / se;
    if (STATS) {  // (B,2,h,w): plane 0 = M, plane 1 = 1 / se
        stats_out[(long long)b * 2 * hw + pix] = M;
        stats_out[(long long)b * 2 * hw + hw + pix] = 1.f / se;
    }
    if (conf_out) {
        const int idx = (int)(si / se);  // .long(): truncation (mvsnet.py:154)
        float conf = 0.f;
#pragma unroll
        for (int j = -1; j <= 2; ++j) {
            const int dd = idx + j;
            if (dd >= 0 && dd < D) conf += expf(c[(long long)dd * hw] - M) / se;
        }
        conf_out[(long long)b * hw + pix] = conf;
    }
}

// VJP of the soft argmin w.r.t. the cost volume (mvsnet.py:139-141, blocks/utils.py:271-274): with p_d = exp(c_d - M) / se and
// depth = sum_d p_d dv_d,  dL/dc_d = p_d * g * (dv_d - depth).  The confidence is computed under no_grad in the reference and has no
// VJP.  One read of the cost volume, one write of its gradient; the per-pixel terms (M, 1/se, g, depth) are read once per lane.
// Workgroup = 64 pixels (lanes along x: each plane row is a coalesced 256-B segment) x 4 waves; the workgroup covers BWD_DCH
// consecutive planes, wave k the planes d0 + k, d0 + k + 4, ...; grid = (pixel blocks, plane chunks, B) so that even B = 1 at
// D = 128 launches thousands of workgroups.
constexpr int BWD_DCH = 32;

__global__ void __launch_bounds__(256) softmax_regress_backward_kernel(const float* __restrict__ cost,
                                                                       const float* __restrict__ depth_values,
                                                                       const float* __restrict__ depth,
                                                                       const float* __restrict__ stats,
                                                                       const float* __restrict__ g_depth, int D, long long hw,
                                                                       float* __restrict__ g_cost) {
    const int b = blockIdx.z;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long pix = (long long)blockIdx.x * 64 + lane;
    if (pix >= hw) return;
    const int d0 = blockIdx.y * BWD_DCH + wv;
    const int d1 = min(D, (int)(blockIdx.y + 1) * BWD_DCH);
    const long long base = (long long)b * D * hw + pix;
    if (!g_depth) {
        for (int d = d0; d < d1; d += 4) g_cost[base + (long long)d * hw] = 0.f;
        return;
    }
    const long long q = (long long)b * hw + pix;
    const float M = stats[(long long)b * 2 * hw + pix];
    const float inv_se = stats[(long long)b * 2 * hw + hw + pix];
    const float gs = g_depth[q] * inv_se;  // g / se
    const float dep = depth[q];
    const float* dv = depth_values + (long long)b * D;
    constexpr int PER = BWD_DCH / 4;
    float v[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int d = d0 + 4 * k;
        v[k] = d < d1 ? cost[base + (long long)d * hw] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int d = d0 + 4 * k;
        if (d < d1) g_cost[base + (long long)d * hw] = expf(v[k] - M) * gs * (dv[d] - dep);
    }
}

// K5 with PER-PIXEL hypotheses (CVP-MVSNet's refinement levels: F.softmax + depth_regression_refine + the 4-bin confidence,
// rmvd/models/cvp_mvsnet.py:210-236, blocks/cvp_mvsnet_components.py:138-141): cost and depth_hypos both (B,D,h,w).
// One lane per pixel over all D planes, lanes along the pixels (every plane row a coalesced 256-B segment per wave): D is 8 there, a
// lane issues its 16 loads at once and the map has far more pixels than the device has lanes, so K5's split of D over four waves
// (made for D = 128 .. 256 on few pixels) has nothing to hide here.  SMALL (D <= 8): the pixel's planes stay in registers and the
// confidence window is taken from them, one pass over both volumes; otherwise K5's chunked online softmax, same operations and
// conventions, and the four window planes are read again.
template <bool SMALL>
__global__ void __launch_bounds__(256) softmax_regress_pp_kernel(const float* __restrict__ cost, const float* __restrict__ hypos, int D,
                                                                 long long hw, float* __restrict__ depth_out,
                                                                 float* __restrict__ conf_out) {
    const int b = blockIdx.y;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const float* c = cost + (long long)b * D * hw + pix;
    const float* dh = hypos + (long long)b * D * hw + pix;
    constexpr int CH = 8;
    float m = -INFINITY, se = 0.f, sd = 0.f, si = 0.f;
    float v[CH], e[CH];
    for (int d0 = 0; d0 < D; d0 += CH) {
        float q[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const bool in = d0 + k < D;
            v[k] = in ? c[(long long)(d0 + k) * hw] : -INFINITY;
            q[k] = in ? dh[(long long)(d0 + k) * hw] : 0.f;
        }
        float cm = v[0];
#pragma unroll
        for (int k = 1; k < CH; ++k) cm = fmaxf(cm, v[k]);
        if (cm > m) {
            const float r = expf(m - cm);  // exp(-inf) = 0 on the first chunk
            se *= r; sd *= r; si *= r;
            m = cm;
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            e[k] = 0.f;
            if (d0 + k < D) {
                e[k] = expf(v[k] - m);
                se += e[k];
                sd = fmaf(e[k], q[k], sd);
                si = fmaf(e[k], (float)(d0 + k), si);
            }
        }
    }
    depth_out[(long long)b * hw + pix] = sd / se;
    if (!conf_out) return;
    const int idx = (int)(si / se);  // .long(): truncation (cvp_mvsnet.py:228-233)
    float conf = 0.f;
    if (SMALL) {  // one chunk: e[k] = exp(c_k - M) is still in registers
#pragma unroll
        for (int k = 0; k < CH; ++k)
            if (k >= idx - 1 && k <= idx + 2) conf += e[k] / se;  // planes k >= D carry e = 0
    } else {
#pragma unroll
        for (int j = -1; j <= 2; ++j) {
            const int dd = idx + j;
            if (dd >= 0 && dd < D) conf += expf(c[(long long)dd * hw] - m) / se;
        }
    }
    conf_out[(long long)b * hw + pix] = conf;
}

}  // namespace mvd

extern "C" int mvd_softmax_regress_pp_f32(const float* cost, const float* depth_hypos, int B, int D, int h, int w, float* depth_out,
                                          float* conf_out, mvd_stream_t stream) {
    MVD_REQUIRE(cost && depth_hypos && depth_out, "softmax_regress_pp: NULL argument");
    MVD_REQUIRE(B > 0 && D > 0 && h > 0 && w > 0 && B <= 65535, "softmax_regress_pp: bad dimension");
    const long long hw = (long long)h * w;
    MVD_REQUIRE((hw + 255) / 256 <= 0x7fffffffLL, "softmax_regress_pp: h*w too large");
    dim3 grid((unsigned)((hw + 255) / 256), (unsigned)B);
    if (D <= 8)
        hipLaunchKernelGGL(mvd::softmax_regress_pp_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, cost, depth_hypos, D, hw, depth_out,
                           conf_out);
    else
        hipLaunchKernelGGL(mvd::softmax_regress_pp_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, cost, depth_hypos, D, hw, depth_out,
                           conf_out);
    return mvd::launch_status("softmax_regress_pp");
}

extern "C" int mvd_softmax_regress_f32(const float* cost, const float* depth_values, int B, int D, int h, int w,
                                       float* depth_out, float* conf_out, mvd_stream_t stream) {
    MVD_REQUIRE(cost && depth_values && depth_out, "softmax_regress: NULL argument");
    MVD_REQUIRE(B > 0 && D > 0 && h > 0 && w > 0 && B <= 65535, "softmax_regress: bad dimension");
    const long long hw = (long long)h * w;
    dim3 grid((unsigned)((hw + 63) / 64), (unsigned)B);
    hipLaunchKernelGGL(mvd::softmax_regress_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, cost, depth_values, D, hw,
                       depth_out, conf_out, nullptr);
    return mvd::launch_status("softmax_regress");
}

extern "C" int mvd_softmax_regress_stats_f32(const float* cost, const float* depth_values, int B, int D, int h, int w,
                                             float* depth_out, float* conf_out, float* stats_out, mvd_stream_t stream) {
    MVD_REQUIRE(cost && depth_values && depth_out && stats_out, "softmax_regress_stats: NULL argument");
    MVD_REQUIRE(B > 0 && D > 0 && h > 0 && w > 0 && B <= 65535, "softmax_regress_stats: bad dimension");
    const long long hw = (long long)h * w;
    dim3 grid((unsigned)((hw + 63) / 64), (unsigned)B);
    hipLaunchKernelGGL(mvd::softmax_regress_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, cost, depth_values, D, hw,
                       depth_out, conf_out, stats_out);
    return mvd::launch_status("softmax_regress_stats");
}

extern "C" int mvd_softmax_regress_backward_f32(const float* cost, const float* depth_values, const float* depth,
                                                const float* stats, const float* g_depth, int B, int D, int h, int w,
                                                float* g_cost, mvd_stream_t stream) {
    MVD_REQUIRE(cost && depth_values && depth && stats && g_cost, "softmax_regress_backward: NULL argument");
    MVD_REQUIRE(B > 0 && D > 0 && h > 0 && w > 0 && B <= 65535, "softmax_regress_backward: bad dimension");
    const long long hw = (long long)h * w;
    MVD_REQUIRE((hw + 63) / 64 <= 0x7fffffffLL, "softmax_regress_backward: h*w too large");
    dim3 grid((unsigned)((hw + 63) / 64), (unsigned)((D + mvd::BWD_DCH - 1) / mvd::BWD_DCH), (unsigned)B);
    hipLaunchKernelGGL(mvd::softmax_regress_backward_kernel, grid, dim3(256), 0, (hipStream_t)stream, cost, depth_values, depth,
                       stats, g_depth, D, hw, g_cost);
    return mvd::launch_status("softmax_regress_backward");
}
