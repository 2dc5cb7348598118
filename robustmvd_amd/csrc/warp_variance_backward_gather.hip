// K3 backward (VJP of homo_warp + variance w.r.t. the feature maps) as a GATHER: no float atomics, a fixed summation order, so two
// calls on the same inputs give the same bits.  backward.hip's kernel scatters each key voxel's share into the four taps of its
// sample; here every interior source pixel collects its shares itself.
//   stage A  dense over (b, y, x, channel quad), no scatter: warps all V views like the scatter kernel's pass 1, writes the per-voxel
//            mean to a workspace volume (B,D,h,w,C) and the key gradient (the scatter kernel's expression, plane by plane: the same
//            bits).  It also PROVES the gather complete: for every tap of every sample that carries weight it evaluates the centre
//            stage B will search around (bwd_centre, the same floats) and checks that this key pixel lies inside that window.  A miss
//            raises the (b, view)'s flag (integer OR: order-independent).
//   stage B  per view, thread = (interior source pixel q, channel quad), planes in ascending order: the plane's homography inverted
//            at q gives a centre; the (2R+1)^2 key pixels around it are tested in row-major order (the channel quads of a pixel share
//            the tests through a ballot); a key pixel whose sample cell contains q contributes w * 2g/(V+1) * (x_v - mean) with the
//            scatter kernel's own weight w.  One store per output, no accumulation into memory.  A flagged (b, view) gets zeros.
//   fallback backward.hip's scatter kernel over the flagged (b, view) only (leaves at once where none is flagged): always correct,
//            deterministic wherever the window holds.  No host synchronisation anywhere.
// Only interior gradients are produced: the zero border's share (which the scatter kernel writes into the border entries) is dropped.
#include "warp_variance_backward_common.h"

namespace mvd {

constexpr int GR = MVD_K3_GATHER_RADIUS;  // window radius in key pixels
constexpr int GW = 2 * GR + 1;
constexpr int FAR = -(1 << 20);           // a centre no key pixel is near

// Centre of source pixel (qx, qy) on one plane: G = the plane's inverse homography (9 floats, source index -> key pixel).  Both
// stages call this with the same arguments, so they agree on the window bit for bit whatever the rounding of G.
__device__ __forceinline__ void bwd_centre(const float* __restrict__ G, float qx, float qy, float xhi, float yhi, int& cx, int& cy) {
    const float n0 = fmaf(G[0], qx, fmaf(G[1], qy, G[2])), n1 = fmaf(G[3], qx, fmaf(G[4], qy, G[5]));
    const float n2 = fmaf(G[6], qx, fmaf(G[7], qy, G[8]));
    const float r = __builtin_amdgcn_rcpf(n2);
    const float px = n0 * r, py = n1 * r;
    const bool near = px > -(float)(GR + 1) && px < xhi + (float)GR && py > -(float)(GR + 1) && py < yhi + (float)GR;  // false for NaN
    cx = near ? (int)rintf(px) : FAR;
    cy = near ? (int)rintf(py) : FAR;
}

// G[v][b][d] = inverse of the plane's homography (ix, iy, 1) ~ S (A d + t e3^T) (x, y, 1), in double, scaled to unit maximum
__global__ void plane_inverse_kernel(const float* __restrict__ M, const float* __restrict__ depth, int B, int D, int V, int h, int w,
                                     float* __restrict__ G) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= V * B * D) return;
    const int d = e % D, b = (e / D) % B, v = e / (D * B);
    const float* m = M + ((size_t)v * B + b) * 12;
    const double z = depth[(size_t)b * D + d];
    const double sx = (double)w / (double)(w - 1), sy = (double)h / (double)(h - 1);
    double H[9];
    for (int i = 0; i < 3; ++i) {
        H[i * 3 + 0] = m[i * 4 + 0] * z; H[i * 3 + 1] = m[i * 4 + 1] * z; H[i * 3 + 2] = m[i * 4 + 2] * z + m[i * 4 + 3];
    }
    for (int j = 0; j < 3; ++j) {
        H[j] = sx * H[j] - 0.5 * H[6 + j];
        H[3 + j] = sy * H[3 + j] - 0.5 * H[6 + j];
    }
    double A[9] = {H[4] * H[8] - H[5] * H[7], H[2] * H[7] - H[1] * H[8], H[1] * H[5] - H[2] * H[4],
                   H[5] * H[6] - H[3] * H[8], H[0] * H[8] - H[2] * H[6], H[2] * H[3] - H[0] * H[5],
                   H[3] * H[7] - H[4] * H[6], H[1] * H[6] - H[0] * H[7], H[0] * H[4] - H[1] * H[3]};
    double mx = 0.0;
    for (int i = 0; i < 9; ++i) mx = fmax(mx, fabs(A[i]));
    const double s = mx > 0.0 ? 1.0 / mx : 0.0;
    for (int i = 0; i < 9; ++i) G[(size_t)e * 9 + i] = (float)(A[i] * s);
}

struct GatherParams {
    WarpBwdParams w;
    const float* G;  // (V,B,D,9)
    float* mean;     // (B,D,h,w,C)
    int* flags;      // (B,V), zeroed before stage A
};

__global__ void __launch_bounds__(256) warp_variance_gather_stage_a_kernel(GatherParams gp) {
    const WarpBwdParams& p = gp.w;
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
    const int W2 = w + 3;
    const size_t img = (size_t)(h + 3) * W2 * C;
    const float sx = (float)w / (float)(w - 1), sy = (float)h / (float)(h - 1);
    const float fx = (float)x, fy = (float)y, xhi = (float)w, yhi = (float)h;
    const float inv_nv = 1.0f / (float)(V + 1);
    const size_t self = ((size_t)(y + 1) * W2 + (x + 1)) * C + q * 4;
    const float4 k = *reinterpret_cast<const float4*>(p.key + b * img + self);
    const float c2 = 2.0f * inv_nv;
    float4 gk = make_float4(0, 0, 0, 0);
    unsigned missed = 0;  // bit v: a contribution to view v lies outside stage B's window
    for (int d = 0; d < D; ++d) {
        const float depth = p.depth[(size_t)b * D + d];
        const size_t vox = ((((size_t)b * D + d) * h + y) * w + x) * C + q * 4;
        const float4 g = *reinterpret_cast<const float4*>(p.gvar + vox);
        float4 sum = k;
        for (int v = 0; v < V; ++v) {
            const SamplePos P = sample_position<false>(p.M + ((size_t)v * p.B + b) * 12, fx, fy, depth, sx, sy, xhi, yhi);
            const SampleCell L = sample_cell(P, W2, C, q * 4);
            const float4 xv = sample_blend(p.src.p[v] + b * img, L, W2, C);
            sum.x += xv.x; sum.y += xv.y; sum.z += xv.z; sum.w += xv.w;
            // the pixel's channel quads share its four taps between them
            const float* __restrict__ G = gp.G + (((size_t)v * p.B + b) * D + d) * 9;
            const int xf = (int)floorf(P.ix), yf = (int)floorf(P.iy);
            bool miss = !(P.ix == P.ix) || !(P.iy == P.iy);
            for (int tap = q; tap < 4; tap += lpp) {
                const int tx = xf + (tap & 1), ty = yf + (tap >> 1);
                const float wt = (tap & 1) ? ((tap & 2) ? L.w11 : L.w10) : ((tap & 2) ? L.w01 : L.w00);
                if (wt != 0.0f && tx >= 0 && tx < w && ty >= 0 && ty < h) {
                    int cx, cy;
                    bwd_centre(G, (float)tx, (float)ty, xhi, yhi, cx, cy);
                    miss |= abs(x - cx) > GR || abs(y - cy) > GR;
                }
            }
            if (miss) missed |= 1u << v;
        }
        const float4 mean = make_float4(sum.x * inv_nv, sum.y * inv_nv, sum.z * inv_nv, sum.w * inv_nv);
        const float4 gs = make_float4(g.x * c2, g.y * c2, g.z * c2, g.w * c2);
        gk.x += gs.x * (k.x - mean.x); gk.y += gs.y * (k.y - mean.y);
        gk.z += gs.z * (k.z - mean.z); gk.w += gs.w * (k.w - mean.w);
        *reinterpret_cast<float4*>(gp.mean + vox) = mean;
    }
    *reinterpret_cast<float4*>(p.gkey + b * img + self) = gk;
    for (int v = 0; v < V; ++v)
        if ((missed >> v & 1u) && __builtin_nontemporal_load(gp.flags + b * V + v) == 0) atomicOr(gp.flags + b * V + v, 1);
}

// Block = 8 x (256 / LPP / 8) source pixels x LPP channel quads; grid (tiles, V, B).  LPP = C / 4 in {1, 2, 4, 8, 16}: the LPP lanes of a
// pixel are neighbours inside one wave and split the window's GW^2 position tests between them.
template <int LPP>
__global__ void __launch_bounds__(256) warp_variance_gather_stage_b_kernel(GatherParams gp) {
    const WarpBwdParams& p = gp.w;
    constexpr int TX = 8, TY = 256 / LPP / TX;
    const int h = p.h, w = p.w, D = p.D, V = p.V;
    constexpr int C = LPP * 4;
    const int tiles_x = (w + TX - 1) / TX;
    const int sub = threadIdx.x % LPP, pi = threadIdx.x / LPP;
    const int qx = (blockIdx.x % tiles_x) * TX + pi % TX, qy = (blockIdx.x / tiles_x) * TY + pi / TX;
    const int v = blockIdx.y, b = blockIdx.z;
    if (qx >= w || qy >= h) return;  // whole pixels leave: the ballots below see complete groups of LPP lanes
    const int W2 = w + 3;
    const size_t img = (size_t)(h + 3) * W2 * C;
    float* __restrict__ out = p.gsrc.p[v] + b * img + ((size_t)(qy + 1) * W2 + (qx + 1)) * C + sub * 4;
    if (gp.flags[b * V + v] != 0) {  // the window does not hold for this view: the fallback launch adds its gradient to zeros
        *reinterpret_cast<float4*>(out) = make_float4(0, 0, 0, 0);
        return;
    }
    const float sx = (float)w / (float)(w - 1), sy = (float)h / (float)(h - 1);
    const float xhi = (float)w, yhi = (float)h, fqx = (float)qx, fqy = (float)qy;
    const float c2 = 2.0f / (float)(V + 1);
    const float* __restrict__ M = p.M + ((size_t)v * p.B + b) * 12;
    const float* __restrict__ f = p.src.p[v] + b * img;
    const int lane = threadIdx.x & 63, shift = lane - sub;
    constexpr int NT = (GW * GW + LPP - 1) / LPP;  // position tests per lane and plane
    float4 acc = make_float4(0, 0, 0, 0);
    for (int d = 0; d < D; ++d) {
        const float depth = p.depth[(size_t)b * D + d];
        int cx, cy;
        bwd_centre(gp.G + (((size_t)v * p.B + b) * D + d) * 9, fqx, fqy, xhi, yhi, cx, cy);
        unsigned long long hits = 0;  // bit i: window pixel i (row-major) samples a cell that contains q
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int i = j * LPP + sub;
            const int px = cx - GR + i % GW, py = cy - GR + i / GW;
            bool hit = false;
            if (i < GW * GW && px >= 0 && px < w && py >= 0 && py < h) {
                const SamplePos P = sample_position<false>(M, (float)px, (float)py, depth, sx, sy, xhi, yhi);
                const unsigned dx = (unsigned)(qx - (int)floorf(P.ix)), dy = (unsigned)(qy - (int)floorf(P.iy));
                hit = dx < 2u && dy < 2u;
            }
            const unsigned long long votes = __ballot(hit);
            hits |= ((votes >> shift) & ((1ull << LPP) - 1ull)) << (j * LPP);
        }
        const size_t plane = ((size_t)b * D + d) * h;
        while (hits) {  // ascending bit = row-major window order, the same for every lane of the pixel
            const int i = __builtin_ctzll(hits);
            hits &= hits - 1;
            const int px = cx - GR + i % GW, py = cy - GR + i / GW;
            const SamplePos P = sample_position<false>(M, (float)px, (float)py, depth, sx, sy, xhi, yhi);
            const SampleCell L = sample_cell(P, W2, C, sub * 4);
            const bool right = qx != (int)floorf(P.ix), low = qy != (int)floorf(P.iy);
            const float wt = right ? (low ? L.w11 : L.w10) : (low ? L.w01 : L.w00);
            const float4 xv = sample_blend(f, L, W2, C);
            const size_t vox = ((plane + py) * w + px) * C + sub * 4;
            const float4 g = *reinterpret_cast<const float4*>(p.gvar + vox);
            const float4 mean = *reinterpret_cast<const float4*>(gp.mean + vox);
            acc.x = fmaf(g.x * c2 * (xv.x - mean.x), wt, acc.x);
            acc.y = fmaf(g.y * c2 * (xv.y - mean.y), wt, acc.y);
            acc.z = fmaf(g.z * c2 * (xv.z - mean.z), wt, acc.z);
            acc.w = fmaf(g.w * c2 * (xv.w - mean.w), wt, acc.w);
        }
    }
    *reinterpret_cast<float4*>(out) = acc;
}

static size_t gather_m_bytes(int B) { return align_up((size_t)MVD_MAX_VIEWS * B * 12 * sizeof(float), 256); }
static size_t gather_g_bytes(int B, int D, int V) { return align_up((size_t)V * B * D * 9 * sizeof(float), 256); }
static size_t gather_flag_bytes(int B, int V) { return align_up((size_t)B * V * sizeof(int), 256); }

}  // namespace mvd

extern "C" {

size_t mvd_warp_variance_backward_gather_workspace_bytes(int B, int C, int D, int h, int w, int V) {
    if (B <= 0 || C <= 0 || D <= 0 || h <= 0 || w <= 0 || V <= 0 || V > MVD_MAX_VIEWS) return 0;
    return mvd::gather_m_bytes(B) + mvd::gather_g_bytes(B, D, V) + mvd::gather_flag_bytes(B, V) +
           mvd::align_up((size_t)B * D * h * w * C * sizeof(float), 256);
}

int mvd_warp_variance_backward_gather_f32(const float* key_feat, const float* const* src_feat, const float* const* src_proj,
                                          const float* key_proj_inv, const float* depth_values, const float* grad_var, int B, int C,
                                          int D, int h, int w, int V, float* grad_key, float* const* grad_src, int* fallback_count,
                                          void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(key_feat && src_feat && src_proj && key_proj_inv && depth_values && grad_var && grad_key && grad_src,
                "warp_variance_backward_gather: NULL argument");
    MVD_REQUIRE(B > 0 && B <= 65535 && D > 0 && h > 1 && w > 1 && V >= 1 && V <= MVD_MAX_VIEWS,
                "warp_variance_backward_gather: bad dimensions");
    MVD_REQUIRE(C == 4 || C == 8 || C == 16 || C == 32 || C == 64, "warp_variance_backward_gather: C=%d unsupported (4, 8, 16, 32, 64)", C);
    const size_t need = mvd_warp_variance_backward_gather_workspace_bytes(B, C, D, h, w, V);
    if (!workspace || workspace_bytes < need) {
        set_error("warp_variance_backward_gather: workspace %zu B < required %zu B", workspace_bytes, need);
        return MVD_ERR_WORKSPACE;
    }
    MVD_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)key_feat & 15) == 0 && ((uintptr_t)grad_var & 15) == 0 &&
                ((uintptr_t)grad_key & 15) == 0, "warp_variance_backward_gather: pointers must be 16-byte aligned");
    GatherParams gp{};
    WarpBwdParams& p = gp.w;
    ViewPtrs proj{};
    for (int v = 0; v < V; ++v) {
        MVD_REQUIRE(src_feat[v] && src_proj[v] && grad_src[v], "warp_variance_backward_gather: NULL view %d", v);
        MVD_REQUIRE(((uintptr_t)src_feat[v] & 15) == 0 && ((uintptr_t)grad_src[v] & 15) == 0,
                    "warp_variance_backward_gather: view %d must be 16-byte aligned", v);
        p.src.p[v] = src_feat[v];
        p.gsrc.p[v] = grad_src[v];
        proj.p[v] = src_proj[v];
    }
    const long long nthr = (long long)B * h * w * (C / 4), nblk = (nthr + 255) / 256;
    MVD_REQUIRE(nblk <= 0x7fffffffLL, "warp_variance_backward_gather: grid too large");
    char* ws = (char*)workspace;
    float* M = (float*)ws; ws += gather_m_bytes(B);
    float* G = (float*)ws; ws += gather_g_bytes(B, D, V);
    int* flags = (int*)ws; ws += gather_flag_bytes(B, V);
    gp.G = G; gp.flags = flags; gp.mean = (float*)ws;
    p.M = M; p.key = key_feat; p.gkey = grad_key; p.depth = depth_values; p.gvar = grad_var;
    p.B = B; p.C = C; p.D = D; p.h = h; p.w = w; p.V = V;
    p.flags = flags; p.fallback_count = fallback_count;
    hipStream_t st = (hipStream_t)stream;
    timing_begin(st);
    if (hipMemsetAsync(flags, 0, (size_t)B * V * sizeof(int), st) != hipSuccess) {
        timing_end(st);
        return launch_status("warp_variance_backward_gather: memset");
    }
    launch_compose_transforms(proj, key_proj_inv, B, V, M, st);
    hipLaunchKernelGGL(plane_inverse_kernel, dim3((unsigned)((V * B * D + 255) / 256)), dim3(256), 0, st, M, depth_values, B, D, V, h, w, G);
    hipLaunchKernelGGL(warp_variance_gather_stage_a_kernel, dim3((unsigned)nblk), dim3(256), 0, st, gp);
    const int lpp = C / 4, ty = 256 / lpp / 8;
    const dim3 grid((unsigned)(((w + 7) / 8) * ((h + ty - 1) / ty)), (unsigned)V, (unsigned)B);
    switch (lpp) {
        case 1: hipLaunchKernelGGL(warp_variance_gather_stage_b_kernel<1>, grid, dim3(256), 0, st, gp); break;
        case 2: hipLaunchKernelGGL(warp_variance_gather_stage_b_kernel<2>, grid, dim3(256), 0, st, gp); break;
        case 4: hipLaunchKernelGGL(warp_variance_gather_stage_b_kernel<4>, grid, dim3(256), 0, st, gp); break;
        case 8: hipLaunchKernelGGL(warp_variance_gather_stage_b_kernel<8>, grid, dim3(256), 0, st, gp); break;
        default: hipLaunchKernelGGL(warp_variance_gather_stage_b_kernel<16>, grid, dim3(256), 0, st, gp); break;
    }
    launch_warp_variance_backward_flagged(p, st);
    timing_end(st);
    return launch_status("warp_variance_backward_gather");
}
}
