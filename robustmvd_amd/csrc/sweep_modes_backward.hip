// Backward (vector-Jacobian product) of the generic sweep reduction (sweep_modes.hip) w.r.t. the FEATURE MAPS: what autograd
// computes through grid_sample in the reference's
//   proj_cost                                   rmvd/models/blocks/cvp_mvsnet_components.py:375-456 (grid detached: :397)
//   homography_warping + groupwise_correlation  rmvd/models/blocks/utils.py:71-89,154-186 (grids carry no gradient: :97,164,181;
//                                               rmvd/models/vis_mvsnet.py:124,150 detach the depths)
// Depth hypotheses and calibration are constants, as there.  With N = V + 1, sv the bilinear sample of view v, k the key feature,
// g the cotangent and m = s1 / N:
//   VARIANCE        s1 = k   + sum sv, s2 = k^2 + sum sv^2, out = s2/N - m^2:  d/dsv = 2 g (sv - m)/N,  d/dk = 2 g (k - m)/N
//   VARIANCE_KEYSQ  s1 = k^2 + sum sv (the reference's alias, :393-394):        d/dsv = 2 g (sv - m)/N,  d/dk = 2 g k (1 - 2m)/N
//   GROUPCORR       out_v[grp,d] = sum_{c in grp} k_c sv_c:                     d/dsv_c = g_v[grp,d] k_c, d/dk_c = sum_v sum_d g_v[grp,d] sv_c
// The source gradient is the transpose of the bilinear gather: the per-sample gradient times the four tap weights, scatter-added
// with no-return float atomics into a zero-bordered channel-last gradient map (the border takes the share of the taps that fell
// on the zero padding and is dropped by the un-padding copy).  Sampling: sweep_homography.h, the forward's own functions.
// A first VJP in the shape of warp_variance_backward_kernel (backward.hip): simple, not tuned; summation order varies from run to
// run for the source gradients, the key gradient is a plain sum per thread (bit-reproducible).
#include "sweep_homography.h"

namespace mvd {
int repack_padded_launch(const float* src, float* dst, int B, int C, int h, int w, hipStream_t st);
size_t padded_slot_bytes_public(int B, int C, int h, int w);

struct ReduceBwdParams {
    ViewPtrs src;        // V x (B,h+3,w+3,C) zero-bordered channel-last
    ViewPtrs M;          // V x (B,3,4)
    ViewPtrs gout;       // variance: gout[0] (B,C,D,h,w); group correlation: gout[v] (B,G,D,h,w)
    ViewOutPtrs gsrc;    // V x (B,h+3,w+3,C), zero-initialised
    const float* key;    // (B,h+3,w+3,C)
    float* gkey;         // (B,C,h,w)
    const float* depth;  // (B,D) or (B,D,h,w)
    int depth_per_pixel;
    float pix_offset, scale_x, scale_y, bias;
    int mode, groups;
    int B, C, D, h, w, V;
};

// Thread = (key pixel, channel quad), quads fastest (a pixel's lanes add into one run of a tap's channels).  Planes in chunks of
// DZ.  Variance modes: pass 1 gathers every view's samples to form the chunk's means, pass 2 gathers again per view (no
// per-view register array) and scatters.  Group correlation needs no mean: one pass per view.  Consecutive planes of a pixel
// mostly sample the same 2 x 2 source cell: their tap gradients are summed in registers and leave as atomics when the cell changes.
template <bool CORR>
__global__ void __launch_bounds__(256) sweep_reduce_backward_kernel(ReduceBwdParams p) {
    const int h = p.h, w = p.w, C = p.C, D = p.D, V = p.V;
    const int lpp = C / 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)p.B * h * w * lpp) return;
    const int q = (int)(t % lpp);
    long long pix = t / lpp;
    const int x = (int)(pix % w); pix /= w;
    const int y = (int)(pix % h);
    const int b = (int)(pix / h);
    const int W2 = w + 3;
    const size_t img = (size_t)(h + 3) * W2 * C;
    const size_t dplane = (size_t)h * w, pin = (size_t)y * w + x;
    const float fx = (float)x + p.pix_offset, fy = (float)y + p.pix_offset, xhi = (float)w, yhi = (float)h;
    const float inv_nv = 1.0f / (float)(V + 1), c2 = 2.0f * inv_nv;
    const bool keysq = p.mode == MVD_REDUCE_VARIANCE_KEYSQ;
    const int c0 = q * 4, grp = CORR ? c0 / (C / p.groups) : 0;
    const float4 k = *reinterpret_cast<const float4*>(p.key + b * img + ((size_t)(y + 1) * W2 + (x + 1)) * C + c0);

    auto locate = [&](int v, float depth) {
        return sample_cell(sample_position_div(p.M.p[v] + (size_t)b * 12, fx, fy, depth, p.scale_x, p.scale_y, p.bias, xhi, yhi), W2, C, c0);
    };
    constexpr int DZ = 8;
    float4 gk = make_float4(0, 0, 0, 0);
    for (int d0 = 0; d0 < D; d0 += DZ) {
        float dep[DZ];
        float4 mean[DZ], gs[DZ];  // gs = g * 2 / (V + 1)
#pragma unroll
        for (int dd = 0; dd < DZ; ++dd) {
            mean[dd] = gs[dd] = make_float4(0, 0, 0, 0);
            dep[dd] = 1.0f;
            const int d = d0 + dd;
            if (d >= D) continue;
            dep[dd] = p.depth_per_pixel ? p.depth[((size_t)b * D + d) * dplane + pin] : p.depth[(size_t)b * D + d];
            if constexpr (!CORR) {
                const float* go = p.gout.p[0] + (((size_t)b * C + c0) * D + d) * dplane + pin;
                const float4 g = make_float4(go[0], go[(size_t)D * dplane], go[2 * (size_t)D * dplane], go[3 * (size_t)D * dplane]);
                float4 s1 = keysq ? make_float4(k.x * k.x, k.y * k.y, k.z * k.z, k.w * k.w) : k;
                for (int v = 0; v < V; ++v) {
                    const float4 sv = sample_blend(p.src.p[v] + b * img, locate(v, dep[dd]), W2, C);
                    s1.x += sv.x; s1.y += sv.y; s1.z += sv.z; s1.w += sv.w;
                }
                const float4 m = make_float4(s1.x * inv_nv, s1.y * inv_nv, s1.z * inv_nv, s1.w * inv_nv);
                mean[dd] = m;
                gs[dd] = make_float4(g.x * c2, g.y * c2, g.z * c2, g.w * c2);
                if (keysq) {  // d/dk = 2 g k (1 - 2 m) / N
                    gk.x += gs[dd].x * k.x * (1.0f - 2.0f * m.x); gk.y += gs[dd].y * k.y * (1.0f - 2.0f * m.y);
                    gk.z += gs[dd].z * k.z * (1.0f - 2.0f * m.z); gk.w += gs[dd].w * k.w * (1.0f - 2.0f * m.w);
                } else {
                    gk.x += gs[dd].x * (k.x - m.x); gk.y += gs[dd].y * (k.y - m.y);
                    gk.z += gs[dd].z * (k.z - m.z); gk.w += gs[dd].w * (k.w - m.w);
                }
            }
        }
        for (int v = 0; v < V; ++v) {
            const float* __restrict__ f = p.src.p[v] + b * img;
            float* __restrict__ gv = p.gsrc.p[v] + b * img;
            PendingCell pend(W2, C);
#pragma unroll
            for (int dd = 0; dd < DZ; ++dd) {
                const int d = d0 + dd;
                if (d >= D) continue;
                const SampleCell L = locate(v, dep[dd]);
                const float4 xv = sample_blend(f, L, W2, C);
                float4 gx;
                if constexpr (CORR) {
                    const float g = p.gout.p[v][(((size_t)b * p.groups + grp) * D + d) * dplane + pin];
                    gx = make_float4(g * k.x, g * k.y, g * k.z, g * k.w);
                    gk.x = fmaf(g, xv.x, gk.x); gk.y = fmaf(g, xv.y, gk.y); gk.z = fmaf(g, xv.z, gk.z); gk.w = fmaf(g, xv.w, gk.w);
                } else {
                    gx = make_float4(gs[dd].x * (xv.x - mean[dd].x), gs[dd].y * (xv.y - mean[dd].y),
                                     gs[dd].z * (xv.z - mean[dd].z), gs[dd].w * (xv.w - mean[dd].w));
                }
                pend.add(gv, L, gx);
            }
            pend.flush(gv);
        }
    }
    float* gko = p.gkey + ((size_t)b * C + c0) * dplane + pin;  // written once per (pixel, channel): no atomics
    gko[0] = gk.x; gko[dplane] = gk.y; gko[2 * dplane] = gk.z; gko[3 * dplane] = gk.w;
}

// (B,h+3,w+3,C) zero-bordered channel-last -> the interior as (B,C,h,w): drops the border's share (padding_mode="zeros")
__global__ void __launch_bounds__(256) unpad_to_nchw_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int C, int h, int w) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)B * C * h * w) return;
    const int x = (int)(e % w), y = (int)((e / w) % h), c = (int)((e / ((long long)w * h)) % C), b = (int)(e / ((long long)w * h * C));
    dst[e] = src[(((size_t)b * (h + 3) + (y + 1)) * (w + 3) + (x + 1)) * C + c];
}

}  // namespace mvd

extern "C" {

size_t mvd_sweep_reduce_backward_workspace_bytes(int B, int C, int h, int w, int V) {
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || V < 0) return 0;
    // zero-bordered channel-last copies of the key and the V sources + V gradient maps of the same shape
    return (size_t)(2 * V + 1) * mvd::padded_slot_bytes_public(B, C, h, w);
}

int mvd_sweep_reduce_backward_f32(const float* key_feat, const float* const* src_feat, const float* const* M, const float* depth,
                                  int depth_per_pixel, float pix_offset, float scale_x, float scale_y, float bias, int mode,
                                  int groups, const float* const* grad_out, int B, int C, int D, int h, int w, int V, float* grad_key,
                                  float* const* grad_src, void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(key_feat && src_feat && M && depth && grad_out && grad_key && grad_src, "sweep_reduce_backward: NULL argument");
    MVD_REQUIRE(B > 0 && D > 0 && h > 1 && w > 1 && V >= 1 && V <= MVD_MAX_VIEWS, "sweep_reduce_backward: bad dimensions");
    MVD_REQUIRE(C >= 4 && C % 4 == 0, "sweep_reduce_backward: C=%d must be a positive multiple of 4", C);
    MVD_REQUIRE(mode == MVD_REDUCE_VARIANCE || mode == MVD_REDUCE_VARIANCE_KEYSQ || mode == MVD_REDUCE_GROUPCORR,
                "sweep_reduce_backward: mode %d", mode);
    if (mode == MVD_REDUCE_GROUPCORR)
        MVD_REQUIRE(groups > 0 && C % groups == 0 && (C / groups) % 4 == 0,
                    "sweep_reduce_backward: C/groups = %d/%d must be a multiple of 4", C, groups);
    const int nout = mode == MVD_REDUCE_GROUPCORR ? V : 1;
    for (int v = 0; v < V; ++v)
        MVD_REQUIRE(src_feat[v] && M[v] && grad_src[v] && (v >= nout || grad_out[v]), "sweep_reduce_backward: NULL view %d", v);
    const long long nthr = (long long)B * h * w * (C / 4), nblk = (nthr + 255) / 256;
    const long long nel = (long long)B * C * h * w;
    MVD_REQUIRE(nblk <= 0x7fffffffLL && (nel + 255) / 256 <= 0x7fffffffLL, "sweep_reduce_backward: grid too large");
    const size_t need = mvd_sweep_reduce_backward_workspace_bytes(B, C, h, w, V);
    if (!workspace || workspace_bytes < need) {
        set_error("sweep_reduce_backward: workspace %zu B < required %zu B", workspace_bytes, need);
        return MVD_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t slot = padded_slot_bytes_public(B, C, h, w);
    char* ws = (char*)workspace;
    ReduceBwdParams p{};
    int rc = repack_padded_launch(key_feat, (float*)ws, B, C, h, w, st);
    if (rc) return rc;
    p.key = (float*)ws;
    ws += slot;
    for (int v = 0; v < V; ++v) {
        rc = repack_padded_launch(src_feat[v], (float*)ws, B, C, h, w, st);
        if (rc) return rc;
        p.src.p[v] = (float*)ws;
        ws += slot;
        p.M.p[v] = M[v];
    }
    for (int v = 0; v < V; ++v) {
        if (hipMemsetAsync(ws, 0, slot, st) != hipSuccess) return launch_status("sweep_reduce_backward: memset");
        p.gsrc.p[v] = (float*)ws;
        ws += slot;
    }
    for (int v = 0; v < nout; ++v) p.gout.p[v] = grad_out[v];
    p.gkey = grad_key;
    p.depth = depth; p.depth_per_pixel = depth_per_pixel;
    p.pix_offset = pix_offset; p.scale_x = scale_x; p.scale_y = scale_y; p.bias = bias;
    p.mode = mode; p.groups = groups;
    p.B = B; p.C = C; p.D = D; p.h = h; p.w = w; p.V = V;
    if (mode == MVD_REDUCE_GROUPCORR)
        hipLaunchKernelGGL(sweep_reduce_backward_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL(sweep_reduce_backward_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, st, p);
    rc = launch_status("sweep_reduce_backward");
    if (rc) return rc;
    for (int v = 0; v < V; ++v)
        hipLaunchKernelGGL(unpad_to_nchw_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, st, p.gsrc.p[v], grad_src[v], B, C, h, w);
    return launch_status("sweep_reduce_backward: unpad");
}
}
