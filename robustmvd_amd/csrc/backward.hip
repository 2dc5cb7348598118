// Backward (vector-Jacobian products) of the sweep operators w.r.t. the FEATURE MAPS — SURVEY.md 8f rank 3:
//   K3  homo_warp + variance          rmvd/models/blocks/utils.py:222-268, rmvd/models/mvsnet.py:124-135
//   K1  PlanesweepCorrelation          rmvd/models/blocks/planesweep_corr.py:152-195 (grids under no_grad: :436,464,489)
//   K2  LearnedFusion view weighting   rmvd/models/blocks/learned_fusion.py:32-48
//   WarpOnlyCorr (warp-only sweep)     rmvd/models/blocks/planesweep_corr.py:107-140
// so that the training loop (rmvd/train/multi_view_depth_training.py:231-246) can back-propagate through the engine.
// The sampling grids depend on calibration only and carry no gradient: the backward of a bilinear gather is a
// scatter-add of the incoming gradient times the same weights, done with no-return float atomics
// (global_atomic_add_f32; MI355X_MICROARCH.md "Global float atomics").  Summation order differs from run to run (atomics).
// Checked against autograd through the reference at one shape per kernel (tests/test_hip_backward.py, tests/golden/g10_grads.npz)
// and against float64 at every instantiation (tests/test_hip_backward_shapes.py: NJ = 1..4, one to four passes of the plane loop,
// tails, the inverse-depth modes, one-hot cotangents): K1, warp-only and K2 stay within 6.5 x the error of the same formula evaluated
// in float32 on the CPU (K1 <= 1.4e-6 on gradients of 2.5), K3 within 1.1e-5 on gradients of 10.  MVSNet trains through K3's
// kernel at full size (profiles/mvsnet_train_step.txt), where the scatter runs at the chip's float-atomic rate and is the largest
// stage of a step; warp_variance_backward_gather.hip is the same VJP as a gather, without atomics and bit-reproducible, and uses
// this file's kernel (FLAGGED) for the views its window cannot cover.  K1's and K2's kernels favour simplicity over speed.
#include "sweep_epipolar.h"
#include "warp_variance_backward_common.h"

namespace mvd {

// ---------------------------------------------------------------------------------------------------------------
// K3 backward.  Thread = (pixel, channel quad); loops over the D planes in chunks of 8.  Per chunk: pass 1 gathers every view's
// samples to form the planes' means, pass 2 gathers again per view (no per-view register array) and scatters
// 2 g (x_v - mean) / (V+1) times the bilinear weights into that view's gradient map, runs of planes that hit the same source
// cell summed in registers first.  Sampling positions: the folded form of the forward kernel.
// FLAGGED (the gather path's fallback): only the (b, view) with a non-zero p.flags entry are scattered, a batch element without
// one leaves at once, and the key gradient (the gather path has written it) is left alone.
template <bool FLAGGED>
__global__ void __launch_bounds__(256) warp_variance_backward_kernel(WarpBwdParams p) {
    const int lpp = p.C / 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long npix = (long long)p.B * p.h * p.w;
    if (t >= npix * lpp) return;
    const int q = (int)(t % lpp);
    long long pix = t / lpp;
    const int x = (int)(pix % p.w); pix /= p.w;
    const int y = (int)(pix % p.h);
    const int b = (int)(pix / p.h);
    const int h = p.h, w = p.w, C = p.C, D = p.D, V = p.V;
    if constexpr (FLAGGED) {
        int n = 0;
        for (int v = 0; v < V; ++v) n += p.flags[b * V + v] != 0;
        if (n == 0) return;
        if (x == 0 && y == 0 && q == 0 && p.fallback_count) atomicAdd(p.fallback_count, n);
    }
    const int W2 = w + 3;
    const size_t img = (size_t)(h + 3) * W2 * C;
    const float sx = (float)w / (float)(w - 1), sy = (float)h / (float)(h - 1);
    const float fx = (float)x, fy = (float)y, xhi = (float)w, yhi = (float)h;
    const float inv_nv = 1.0f / (float)(V + 1);
    const size_t self = ((size_t)(y + 1) * W2 + (x + 1)) * C + q * 4;
    const float4 k = *reinterpret_cast<const float4*>(p.key + b * img + self);

    auto locate = [&](int v, float depth) {
        return sample_cell(sample_position<false>(p.M + ((size_t)v * p.B + b) * 12, fx, fy, depth, sx, sy, xhi, yhi), W2, C, q * 4);
    };

    // Planes in chunks of DZ: the chunk's means stay in registers, then each view walks the chunk with one PendingCell of tap
    // gradients in registers.
    constexpr int DZ = 8;
    const float c2 = 2.0f * inv_nv;
    float4 gk = make_float4(0, 0, 0, 0);
    for (int d0 = 0; d0 < D; d0 += DZ) {
        float4 mean[DZ], gs[DZ];  // gs = g * 2 / (V + 1)
#pragma unroll
        for (int dd = 0; dd < DZ; ++dd) {
            mean[dd] = gs[dd] = make_float4(0, 0, 0, 0);
            const int d = d0 + dd;
            if (d >= D) continue;
            const float depth = p.depth[(size_t)b * D + d];
            const float4 g = *reinterpret_cast<const float4*>(p.gvar + ((((size_t)b * D + d) * h + y) * w + x) * C + q * 4);
            float4 sum = k;
            for (int v = 0; v < V; ++v) {
                const float4 xv = sample_blend(p.src.p[v] + b * img, locate(v, depth), W2, C);
                sum.x += xv.x; sum.y += xv.y; sum.z += xv.z; sum.w += xv.w;
            }
            mean[dd] = make_float4(sum.x * inv_nv, sum.y * inv_nv, sum.z * inv_nv, sum.w * inv_nv);
            gs[dd] = make_float4(g.x * c2, g.y * c2, g.z * c2, g.w * c2);
            gk.x += gs[dd].x * (k.x - mean[dd].x); gk.y += gs[dd].y * (k.y - mean[dd].y);
            gk.z += gs[dd].z * (k.z - mean[dd].z); gk.w += gs[dd].w * (k.w - mean[dd].w);
        }
        for (int v = 0; v < V; ++v) {
            if constexpr (FLAGGED) {
                if (p.flags[b * V + v] == 0) continue;
            }
            const float* __restrict__ f = p.src.p[v] + b * img;
            float* __restrict__ gv = p.gsrc.p[v] + b * img;
            PendingCell pend(W2, C);
#pragma unroll
            for (int dd = 0; dd < DZ; ++dd) {
                const int d = d0 + dd;
                if (d >= D) continue;
                const SampleCell L = locate(v, p.depth[(size_t)b * D + d]);
                const float4 xv = sample_blend(f, L, W2, C);
                pend.add(gv, L, make_float4(gs[dd].x * (xv.x - mean[dd].x), gs[dd].y * (xv.y - mean[dd].y),
                                            gs[dd].z * (xv.z - mean[dd].z), gs[dd].w * (xv.w - mean[dd].w)));
            }
            pend.flush(gv);
        }
    }
    if constexpr (!FLAGGED) *reinterpret_cast<float4*>(p.gkey + b * img + self) = gk;
}

// ---------------------------------------------------------------------------------------------------------------
// K1 backward.  One wave per key pixel, lane = channel slice (C = 64 NJ), loops over views and planes; geometry (the
// forward's own functions, sweep_epipolar.h: they decide the 0/1 mask) is evaluated by lane = plane in passes of 64 and broadcast
// with readlane.  Consecutive planes that share a 2x2 source cell accumulate their tap gradients in registers and
// flush them with atomics when the cell changes (~4x fewer atomics).
struct SweepBwdParams {
    ViewPtrs src;        // V x (N,hs+3,ws+3,C) zero-bordered channel-last source features
    ViewPtrs K_src, T;   // V x (N,3,3), V x (N,4,4)
    ViewPtrs gcorr;      // V x (N,S,h,w)
    ViewOutPtrs gsrc;    // V x (N,hs+3,ws+3,C), zero-initialised
    const float* key;    // (N,h,w,C) channel-last
    float* gkey;         // (N,h,w,C)
    const float* K_key;  // (N,3,3)
    const float* invd;
    int invd_stride;
    int invd_per_pixel;
    float corr_scale;
    int N, h, w, hs, ws, S, V;
};

template <int NJ>
__global__ void __launch_bounds__(256) sweep_corr_backward_kernel(SweepBwdParams p) {
    constexpr int C = 64 * NJ;
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long long)p.N * p.h * p.w) return;  // wave-uniform
    const int x = (int)(wid % p.w), y = (int)((wid / p.w) % p.h), n = (int)(wid / ((long long)p.w * p.h));
    const int h = p.h, w = p.w, hs = p.hs, ws = p.ws, S = p.S, W2 = ws + 3;
    const float inv_sqrt_c = p.corr_scale;
    const float xc = (float)x + 0.5f, yc = (float)y + 0.5f;
    const float* __restrict__ invd = p.invd + (size_t)n * p.invd_stride;
    float kf[NJ], gk[NJ];
    const size_t koff = (((size_t)n * h + y) * w + x) * C + lane * NJ;
#pragma unroll
    for (int j = 0; j < NJ; ++j) { kf[j] = p.key[koff + j]; gk[j] = 0.f; }

    for (int v = 0; v < p.V; ++v) {
        const Epi E = epipolar(p.K_key + n * 9, p.K_src.p[v] + n * 9, p.T.p[v] + n * 16, h, w, hs, ws);
        const SweepRay R = sweep_ray(E, xc, yc);
        const size_t simg = (size_t)n * (hs + 3) * W2 * C;
        const float* __restrict__ src = p.src.p[v] + simg + lane * NJ;
        float* __restrict__ gsrc = p.gsrc.p[v] + simg + lane * NJ;
        const float* __restrict__ gc = p.gcorr.p[v] + (((size_t)n * S) * h + y) * w + x;
        int cur = -1;
        float tap[4][NJ], gt[4][NJ];
        auto flush = [&]() {
            if (cur < 0) return;
            float* g0 = gsrc + (size_t)cur * C;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                unsafeAtomicAdd(g0 + j, gt[0][j]); unsafeAtomicAdd(g0 + C + j, gt[1][j]);
                unsafeAtomicAdd(g0 + (size_t)W2 * C + j, gt[2][j]); unsafeAtomicAdd(g0 + (size_t)W2 * C + C + j, gt[3][j]);
            }
        };
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane;
            const bool live = s < S;
            const int sc = live ? s : S - 1;
            const float ds = p.invd_per_pixel ? p.invd[(((size_t)n * S + sc) * h + y) * w + x] : invd[sc];
            const SweepSample G = sweep_sample(E, R, ds, hs, ws, W2);
            const Taps& t = G.t;
            const float mk = sweep_corr_mask(G);
            const int cell = G.cell;
            const float gcoef = live ? gc[(size_t)s * h * w] * mk * inv_sqrt_c : 0.f;
            const int npl = min(64, S - s0);
            for (int i = 0; i < npl; ++i) {  // wave-uniform
                const float gci = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gcoef), i));
                if (gci == 0.f) continue;
                const int ci = __builtin_amdgcn_readlane(cell, i);
                if (ci != cur) {
                    flush();
                    cur = ci;
                    const float* s00 = src + (size_t)ci * C;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        tap[0][j] = s00[j]; tap[1][j] = s00[C + j];
                        tap[2][j] = s00[(size_t)W2 * C + j]; tap[3][j] = s00[(size_t)W2 * C + C + j];
                        gt[0][j] = gt[1][j] = gt[2][j] = gt[3][j] = 0.f;
                    }
                }
                float wk[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) wk[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t.w[k]), i));
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const float samp = fmaf(tap[3][j], wk[3], fmaf(tap[2][j], wk[2], fmaf(tap[1][j], wk[1], tap[0][j] * wk[0])));
                    gk[j] = fmaf(gci, samp, gk[j]);
                    const float gkf = gci * kf[j];
#pragma unroll
                    for (int k = 0; k < 4; ++k) gt[k][j] = fmaf(gkf, wk[k], gt[k][j]);
                }
            }
        }
        flush();
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) p.gkey[koff + j] = gk[j];
}

// ---------------------------------------------------------------------------------------------------------------
// Warp-only backward: VJP of sweep_warp_kernel (sweep_corr.hip, WarpOnlyCorr planesweep_corr.py:107-140) w.r.t. the source
// features, normalize_after = 0: warped = sample * mask is linear in the features, so the gradient of a source pixel is the sum of
// the cotangents of the samples that touched it times their tap weights; no feature map is read.  K1 backward's shape: one
// wave per key pixel, lane = channel (c = j * 64 + lane), geometry by lane = plane in passes of 64 and broadcast with readlane,
// runs of planes in one 2x2 cell summed in registers.  The mask is the SAMPLING mask alone, as in the forward (WarpOnlyCorr
// does not take the visibility mask).
struct WarpOnlyBwdParams {
    ViewPtrs K_src, T;   // V x (N,3,3), V x (N,4,4)
    ViewPtrs gwarp;      // V x (N,S,C,h,w)
    ViewOutPtrs gsrc;    // V x (N,hs+3,ws+3,C), zero-initialised
    const float* K_key;  // (N,3,3)
    const float* invd;
    int invd_stride, invd_per_pixel;
    int N, C, h, w, hs, ws, S, V;
};

template <int NJ>
__global__ void __launch_bounds__(256) sweep_warp_backward_kernel(WarpOnlyBwdParams p) {
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long long)p.N * p.h * p.w) return;  // wave-uniform
    const int x = (int)(wid % p.w), y = (int)((wid / p.w) % p.h), n = (int)(wid / ((long long)p.w * p.h));
    const int h = p.h, w = p.w, hs = p.hs, ws = p.ws, S = p.S, C = p.C, W2 = ws + 3;
    const size_t hw = (size_t)h * w;
    const float xc = (float)x + 0.5f, yc = (float)y + 0.5f;
    const float* __restrict__ invd = p.invd + (size_t)n * p.invd_stride;

    for (int v = 0; v < p.V; ++v) {
        const Epi E = epipolar(p.K_key + n * 9, p.K_src.p[v] + n * 9, p.T.p[v] + n * 16, h, w, hs, ws);
        const SweepRay R = sweep_ray(E, xc, yc);
        float* __restrict__ gsrc = p.gsrc.p[v] + (size_t)n * (hs + 3) * W2 * C;
        const float* __restrict__ gw = p.gwarp.p[v] + (size_t)n * S * C * hw + (size_t)y * w + x;
        int cur = -1;
        float gt[4][NJ];
        auto flush = [&]() {
            if (cur < 0) return;
            float* g0 = gsrc + (size_t)cur * C;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int c = j * 64 + lane;
                if (c < C) {
                    unsafeAtomicAdd(g0 + c, gt[0][j]); unsafeAtomicAdd(g0 + C + c, gt[1][j]);
                    unsafeAtomicAdd(g0 + (size_t)W2 * C + c, gt[2][j]); unsafeAtomicAdd(g0 + (size_t)W2 * C + C + c, gt[3][j]);
                }
            }
        };
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane;
            const bool live = s < S;
            const int sc = live ? s : S - 1;
            const float ds = p.invd_per_pixel ? p.invd[(((size_t)n * S + sc) * h + y) * w + x] : invd[sc];
            const SweepSample G = sweep_sample(E, R, ds, hs, ws, W2);
            const float mk = live ? sweep_warp_mask(G) : 0.f;
            const int npl = min(64, S - s0);
            for (int i = 0; i < npl; ++i) {  // wave-uniform
                const float mki = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mk), i));
                if (mki == 0.f) continue;
                const int ci = __builtin_amdgcn_readlane(G.cell, i);
                if (ci != cur) {
                    flush();
                    cur = ci;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) gt[0][j] = gt[1][j] = gt[2][j] = gt[3][j] = 0.f;
                }
                float wk[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) wk[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(G.t.w[k]), i));
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int c = j * 64 + lane;
                    const float g = c < C ? gw[((size_t)(s0 + i) * C + c) * hw] : 0.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) gt[k][j] = fmaf(g, wk[k], gt[k][j]);
                }
            }
        }
        flush();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// K2 backward.  One wave per (n, y, x): lanes stride over the S planes; the gradient w.r.t. the per-view score (one value
// per pixel) is the wave-reduced sum over planes pushed through the softmax Jacobian.
struct FuseBwdParams {
    ViewPtrs corr, mask, score, dummy;
    ViewOutPtrs gcorr, gscore;
    const float* gfused;
    int N, S, h, w, V;
};

__global__ void __launch_bounds__(256) fuse_views_backward_kernel(FuseBwdParams p) {
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long hw = (long long)p.h * p.w;
    if (wid >= p.N * hw) return;
    const int n = (int)(wid / hw);
    const long long pix = wid % hw;
    const int V = p.V, S = p.S;
    float pr[MVD_MAX_VIEWS];
    float mx = -3.4e38f;
    for (int v = 0; v < V; ++v) { pr[v] = p.score.p[v][n * hw + pix]; mx = fmaxf(mx, pr[v]); }
    float den = 0.f;
    for (int v = 0; v < V; ++v) { pr[v] = expf(pr[v] - mx); den += pr[v]; }
    for (int v = 0; v < V; ++v) pr[v] /= den;
    float dp[MVD_MAX_VIEWS];
    for (int v = 0; v < V; ++v) dp[v] = 0.f;
    for (int s = lane; s < S; s += 64) {
        const size_t o = ((size_t)n * S + s) * hw + pix;
        float W = 0.f, num = 0.f;
        for (int v = 0; v < V; ++v) {
            const float u = (pr[v] + 1e-9f) * p.mask.p[v][o];
            W += u;
            num = fmaf(p.corr.p[v][o], u, num);
        }
        const float g = (W != 0.f) ? p.gfused[o] : 0.f;
        const float d = W + 1e-9f, q = num / d;
        for (int v = 0; v < V; ++v) {
            const float m = p.mask.p[v][o], u = (pr[v] + 1e-9f) * m;
            p.gcorr.p[v][o] = g * u / d;
            dp[v] = fmaf(g * (p.corr.p[v][o] - q) / d, m, dp[v]);
        }
    }
    float dot = 0.f;
    for (int v = 0; v < V; ++v) {
        float t = dp[v];
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
        dp[v] = t;
        dot = fmaf(pr[v], t, dot);
    }
    if (lane == 0)
        for (int v = 0; v < V; ++v) p.gscore.p[v][n * hw + pix] = pr[v] * (dp[v] - dot);
}

void launch_warp_variance_backward_flagged(const WarpBwdParams& p, hipStream_t st) {
    const long long nthr = (long long)p.B * p.h * p.w * (p.C / 4);
    hipLaunchKernelGGL(warp_variance_backward_kernel<true>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, p);
}

}  // namespace mvd

extern "C" {

size_t mvd_warp_variance_backward_workspace_bytes(int B) {
    return B > 0 ? mvd::align_up((size_t)MVD_MAX_VIEWS * B * 12 * sizeof(float), 256) : 0;
}

int mvd_warp_variance_backward_f32(const float* key_feat, const float* const* src_feat, const float* const* src_proj,
                                   const float* key_proj_inv, const float* depth_values, const float* grad_var, int B, int C,
                                   int D, int h, int w, int V, float* grad_key, float* const* grad_src, void* workspace,
                                   size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(key_feat && src_feat && src_proj && key_proj_inv && depth_values && grad_var && grad_key && grad_src,
                "warp_variance_backward: NULL argument");
    MVD_REQUIRE(B > 0 && D > 0 && h > 1 && w > 1 && V >= 1 && V <= MVD_MAX_VIEWS, "warp_variance_backward: bad dimensions");
    MVD_REQUIRE(C >= 4 && C % 4 == 0, "warp_variance_backward: C=%d must be a positive multiple of 4", C);
    const size_t need = mvd_warp_variance_backward_workspace_bytes(B);
    if (!workspace || workspace_bytes < need) {
        set_error("warp_variance_backward: workspace %zu B < required %zu B", workspace_bytes, need);
        return MVD_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    WarpBwdParams p{};
    ViewPtrs proj{};
    const size_t slot = (size_t)B * (h + 3) * (w + 3) * C * sizeof(float);
    for (int v = 0; v < V; ++v) {
        MVD_REQUIRE(src_feat[v] && src_proj[v] && grad_src[v], "warp_variance_backward: NULL view %d", v);
        p.src.p[v] = src_feat[v];
        p.gsrc.p[v] = grad_src[v];
        proj.p[v] = src_proj[v];
        if (hipMemsetAsync(grad_src[v], 0, slot, st) != hipSuccess) return launch_status("warp_variance_backward: memset");
    }
    if (hipMemsetAsync(grad_key, 0, slot, st) != hipSuccess) return launch_status("warp_variance_backward: memset");
    p.M = (float*)workspace;
    launch_compose_transforms(proj, key_proj_inv, B, V, (float*)workspace, st);
    p.key = key_feat; p.gkey = grad_key; p.depth = depth_values; p.gvar = grad_var;
    p.B = B; p.C = C; p.D = D; p.h = h; p.w = w; p.V = V;
    const long long nthr = (long long)B * h * w * (C / 4), nblk = (nthr + 255) / 256;
    MVD_REQUIRE(nblk <= 0x7fffffffLL, "warp_variance_backward: grid too large");
    hipLaunchKernelGGL(warp_variance_backward_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, st, p);
    return launch_status("warp_variance_backward");
}

int mvd_sweep_corr_backward_f32(const float* feat_key, const float* const* feat_src, const float* K_key,
                                const float* const* K_src, const float* const* T_src2key, const float* invdepths,
                                int invdepth_mode, float corr_scale, const float* const* grad_corr, int N, int C, int h, int w,
                                int hs, int ws, int S, int V, float* grad_key, float* const* grad_src, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(invdepth_mode >= MVD_INVDEPTH_SHARED && invdepth_mode <= MVD_INVDEPTH_PER_PIXEL, "sweep_corr_backward: invdepth_mode %d", invdepth_mode);
    MVD_REQUIRE(feat_key && feat_src && K_key && K_src && T_src2key && invdepths && grad_corr && grad_key && grad_src,
                "sweep_corr_backward: NULL argument");
    MVD_REQUIRE(N > 0 && h > 0 && w > 0 && hs > 0 && ws > 0 && S > 0 && V >= 1 && V <= MVD_MAX_VIEWS, "sweep_corr_backward: bad dimensions");
    MVD_REQUIRE(C == 64 || C == 128 || C == 192 || C == 256, "sweep_corr_backward: C=%d unsupported (64, 128, 192, 256)", C);
    hipStream_t st = (hipStream_t)stream;
    SweepBwdParams p{};
    const size_t slot = (size_t)N * (hs + 3) * (ws + 3) * C * sizeof(float);
    for (int v = 0; v < V; ++v) {
        MVD_REQUIRE(feat_src[v] && K_src[v] && T_src2key[v] && grad_corr[v] && grad_src[v], "sweep_corr_backward: NULL view %d", v);
        p.src.p[v] = feat_src[v]; p.K_src.p[v] = K_src[v]; p.T.p[v] = T_src2key[v]; p.gcorr.p[v] = grad_corr[v];
        p.gsrc.p[v] = grad_src[v];
        if (hipMemsetAsync(grad_src[v], 0, slot, st) != hipSuccess) return launch_status("sweep_corr_backward: memset");
    }
    p.key = feat_key; p.gkey = grad_key; p.K_key = K_key; p.invd = invdepths;
    p.invd_stride = invdepth_mode == MVD_INVDEPTH_BATCHED ? S : 0;
    p.invd_per_pixel = invdepth_mode == MVD_INVDEPTH_PER_PIXEL;
    p.corr_scale = corr_scale;
    p.N = N; p.h = h; p.w = w; p.hs = hs; p.ws = ws; p.S = S; p.V = V;
    const long long nwave = (long long)N * h * w, nblk = (nwave + 3) / 4;
    MVD_REQUIRE(nblk <= 0x7fffffffLL, "sweep_corr_backward: grid too large");
    switch (C / 64) {
        case 1: hipLaunchKernelGGL(sweep_corr_backward_kernel<1>, dim3((unsigned)nblk), dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL(sweep_corr_backward_kernel<2>, dim3((unsigned)nblk), dim3(256), 0, st, p); break;
        case 3: hipLaunchKernelGGL(sweep_corr_backward_kernel<3>, dim3((unsigned)nblk), dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL(sweep_corr_backward_kernel<4>, dim3((unsigned)nblk), dim3(256), 0, st, p); break;
    }
    return launch_status("sweep_corr_backward");
}

int mvd_sweep_warp_backward_f32(const float* K_key, const float* const* K_src, const float* const* T_src2key, const float* invdepths,
                                int invdepth_mode, const float* const* grad_warped, int N, int C, int h, int w, int hs, int ws, int S,
                                int V, float* const* grad_src, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(invdepth_mode >= MVD_INVDEPTH_SHARED && invdepth_mode <= MVD_INVDEPTH_PER_PIXEL, "sweep_warp_backward: invdepth_mode %d", invdepth_mode);
    MVD_REQUIRE(K_key && K_src && T_src2key && invdepths && grad_warped && grad_src, "sweep_warp_backward: NULL argument");
    MVD_REQUIRE(N > 0 && h > 0 && w > 0 && hs > 0 && ws > 0 && S > 0 && V >= 1 && V <= MVD_MAX_VIEWS, "sweep_warp_backward: bad dimensions");
    MVD_REQUIRE(C >= 1 && C <= 256, "sweep_warp_backward: C=%d unsupported (1..256)", C);
    MVD_REQUIRE((long long)(hs + 3) * (ws + 3) < 0x7fffffffLL, "sweep_warp_backward: source map %dx%d too large", hs, ws);
    hipStream_t st = (hipStream_t)stream;
    WarpOnlyBwdParams p{};
    const size_t slot = (size_t)N * (hs + 3) * (ws + 3) * C * sizeof(float);
    for (int v = 0; v < V; ++v)
        MVD_REQUIRE(K_src[v] && T_src2key[v] && grad_warped[v] && grad_src[v], "sweep_warp_backward: NULL view %d", v);
    const long long nwave = (long long)N * h * w, nblk = (nwave + 3) / 4;
    MVD_REQUIRE(nblk <= 0x7fffffffLL, "sweep_warp_backward: grid too large");
    for (int v = 0; v < V; ++v) {
        p.K_src.p[v] = K_src[v]; p.T.p[v] = T_src2key[v]; p.gwarp.p[v] = grad_warped[v]; p.gsrc.p[v] = grad_src[v];
        if (hipMemsetAsync(grad_src[v], 0, slot, st) != hipSuccess) return launch_status("sweep_warp_backward: memset");
    }
    p.K_key = K_key; p.invd = invdepths;
    p.invd_stride = invdepth_mode == MVD_INVDEPTH_BATCHED ? S : 0;
    p.invd_per_pixel = invdepth_mode == MVD_INVDEPTH_PER_PIXEL;
    p.N = N; p.C = C; p.h = h; p.w = w; p.hs = hs; p.ws = ws; p.S = S; p.V = V;
    switch ((C + 63) / 64) {
        case 1: hipLaunchKernelGGL(sweep_warp_backward_kernel<1>, dim3((unsigned)nblk), dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL(sweep_warp_backward_kernel<2>, dim3((unsigned)nblk), dim3(256), 0, st, p); break;
        case 3: hipLaunchKernelGGL(sweep_warp_backward_kernel<3>, dim3((unsigned)nblk), dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL(sweep_warp_backward_kernel<4>, dim3((unsigned)nblk), dim3(256), 0, st, p); break;
    }
    return launch_status("sweep_warp_backward");
}

int mvd_fuse_views_backward_f32(const float* const* corr, const float* const* mask, const float* const* score,
                                const float* grad_fused, int N, int S, int h, int w, int V, float* const* grad_corr,
                                float* const* grad_score, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(corr && mask && score && grad_fused && grad_corr && grad_score, "fuse_views_backward: NULL argument");
    MVD_REQUIRE(N > 0 && S > 0 && h > 0 && w > 0 && V >= 2 && V <= MVD_MAX_VIEWS, "fuse_views_backward: bad dimensions (V >= 2)");
    FuseBwdParams p{};
    for (int v = 0; v < V; ++v) {
        MVD_REQUIRE(corr[v] && mask[v] && score[v] && grad_corr[v] && grad_score[v], "fuse_views_backward: NULL view %d", v);
        p.corr.p[v] = corr[v]; p.mask.p[v] = mask[v]; p.score.p[v] = score[v];
        p.gcorr.p[v] = grad_corr[v]; p.gscore.p[v] = grad_score[v];
    }
    p.gfused = grad_fused; p.N = N; p.S = S; p.h = h; p.w = w; p.V = V;
    const long long nwave = (long long)N * h * w, nblk = (nwave + 3) / 4;
    MVD_REQUIRE(nblk <= 0x7fffffffLL, "fuse_views_backward: grid too large");
    hipLaunchKernelGGL(fuse_views_backward_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, p);
    return launch_status("fuse_views_backward");
}
}
