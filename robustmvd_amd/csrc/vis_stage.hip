// The two per-stage kernels of Vis-MVSNet's SingleStage besides the cost volume and the 3-D convolutions
// (rmvd/models/blocks/vis_mvsnet_singlestage.py:149-348):
//   mvd_soft_argmin_f32   soft_argmin (+ entropy, + the windowed probability), blocks/utils.py:51-68, called at
//                         vis_mvsnet_singlestage.py:254-258 (per pair, with the entropy) and :330-333 (fused, window = 2)
//   mvd_vis_fuse_f32      the "soft" fusion of the pairs' regularised volumes, vis_mvsnet_singlestage.py:263-266,302-303
#include "mvd_common.h"

namespace mvd {

// One lane per pixel, the D planes strided by h w: consecutive lanes read consecutive floats of a plane row.  Three passes over the
// pixel's D scores: the maximum; the sums  se = sum_i exp(c_i - m)  and  si = sum_i i exp(c_i - m)  (index = si / se); then, only
// where an optional output asks for it, the probabilities p_i = exp(c_i - m) / se again for the entropy terms, each with the
// reference's clamp (the closed form log se - ... differs where p_i < 1e-9), and for the window mask |i - index| <= window.
// A workgroup is one wave: the per-pair calls of the coarse stage have few pixels (a 1/8-resolution map per pair), and 64-pixel
// workgroups spread them over four times as many compute units as 256-pixel ones.
__global__ void __launch_bounds__(64) soft_argmin_kernel(const float* __restrict__ score, const float* __restrict__ depth_start,
                                                         int start_per_pixel, const float* __restrict__ depth_interval, float window,
                                                         int D, long long hw, float* __restrict__ depth_out,
                                                         float* __restrict__ entropy_out, float* __restrict__ prob_map_out) {
    const int b = blockIdx.y;
    const long long pix = (long long)blockIdx.x * 64 + threadIdx.x;
    if (pix >= hw) return;
    const float* c = score + (long long)b * D * hw + pix;
    float m = c[0];
    for (int i = 1; i < D; ++i) m = fmaxf(m, c[(long long)i * hw]);
    float se = 0.f, si = 0.f;
    for (int i = 0; i < D; ++i) {
        const float e = expf(c[(long long)i * hw] - m);
        se += e;
        si = fmaf(e, (float)i, si);
    }
    const float index = si / se;
    const long long o = (long long)b * hw + pix;
    const float start = start_per_pixel ? depth_start[o] : depth_start[b];
    depth_out[o] = index * depth_interval[b] + start;  // two roundings, as the reference's mul and add
    if (!entropy_out && !prob_map_out) return;
    float ent = 0.f, prob = 0.f;
    for (int i = 0; i < D; ++i) {
        const float pi = expf(c[(long long)i * hw] - m) / se;
        ent += -pi * logf(fminf(fmaxf(pi, 1e-9f), 1.0f));
        if (fabsf((float)i - index) <= window) prob += pi;
    }
    if (entropy_out) entropy_out[o] = ent;
    if (prob_map_out) prob_map_out[o] = prob;
}

// Thread = one float4 of channels of one voxel; the voxel's pixel gives the V weights exp(-u_v), formed once per float4.
// Both sums run in view order from 0 with separate multiply and add (the library is built without contraction), as the reference's
// `fused = fused + interm * weight` and `weight_sum = weight_sum + weight`, then one division.
__global__ void __launch_bounds__(256) vis_fuse_kernel(ViewPtrs x, ViewPtrs u, int V, int C4, long long hw, long long dhw,
                                                       long long n4, float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n4) return;
    const long long vox = t / C4;
    const long long b = vox / dhw, pix = vox % hw;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float ws = 0.f;
    for (int v = 0; v < V; ++v) {
        const float wv = expf(-u.p[v][b * hw + pix]);
        const float4 xv = reinterpret_cast<const float4*>(x.p[v])[t];
        acc.x = acc.x + xv.x * wv; acc.y = acc.y + xv.y * wv; acc.z = acc.z + xv.z * wv; acc.w = acc.w + xv.w * wv;
        ws = ws + wv;
    }
    reinterpret_cast<float4*>(out)[t] = make_float4(acc.x / ws, acc.y / ws, acc.z / ws, acc.w / ws);
}

}  // namespace mvd

extern "C" int mvd_soft_argmin_f32(const float* score, const float* depth_start, int start_per_pixel, const float* depth_interval,
                                   float window, int B, int D, int h, int w, float* depth_out, float* entropy_out, float* prob_map_out,
                                   mvd_stream_t stream) {
    MVD_REQUIRE(score && depth_start && depth_interval && depth_out, "soft_argmin: NULL argument");
    MVD_REQUIRE(B > 0 && D > 0 && h > 0 && w > 0 && B <= 65535, "soft_argmin: bad dimension");
    const long long hw = (long long)h * w;
    MVD_REQUIRE((hw + 63) / 64 <= 0x7fffffffLL, "soft_argmin: h*w too large");
    hipLaunchKernelGGL(mvd::soft_argmin_kernel, dim3((unsigned)((hw + 63) / 64), (unsigned)B), dim3(64), 0, (hipStream_t)stream, score,
                       depth_start, start_per_pixel, depth_interval, window, D, hw, depth_out, entropy_out, prob_map_out);
    return mvd::launch_status("soft_argmin");
}

extern "C" int mvd_vis_fuse_f32(const float* const* x, const float* const* u, int B, int D, int h, int w, int C, int V, float* out,
                                mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(x && u && out, "vis_fuse: NULL argument");
    MVD_REQUIRE(B > 0 && D > 0 && h > 0 && w > 0 && V >= 1 && V <= MVD_MAX_VIEWS, "vis_fuse: bad dimensions");
    MVD_REQUIRE(C >= 4 && C % 4 == 0, "vis_fuse: C=%d must be a positive multiple of 4", C);
    MVD_REQUIRE(((uintptr_t)out & 15) == 0, "vis_fuse: out must be 16-byte aligned");
    ViewPtrs xs{}, us{};
    for (int v = 0; v < V; ++v) {
        MVD_REQUIRE(x[v] && u[v], "vis_fuse: NULL view %d", v);
        MVD_REQUIRE(((uintptr_t)x[v] & 15) == 0, "vis_fuse: x[%d] must be 16-byte aligned", v);
        xs.p[v] = x[v];
        us.p[v] = u[v];
    }
    const long long hw = (long long)h * w, dhw = (long long)D * hw, n4 = (long long)B * dhw * (C / 4);
    const long long nblk = (n4 + 255) / 256;
    MVD_REQUIRE(nblk <= 0x7fffffffLL, "vis_fuse: grid too large");
    hipLaunchKernelGGL(vis_fuse_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, xs, us, V, C / 4, hw, dhw, n4, out);
    return launch_status("vis_fuse");
}
