// K3 — fronto-parallel homography warp of V source feature maps into the key frustum at D depth
// hypotheses + variance aggregation with the key features, in one pass (Path B).
// Replaces homo_warp (rmvd/models/blocks/utils.py:222-268) and the sum / sum-of-squares / variance
// arithmetic of MVSNet.forward (rmvd/models/mvsnet.py:124-136).
//
// HBM-bound by construction: the only large tensor is the variance volume, written exactly once
// (algorithmic bytes 4*((V+1)*C*h*w + C*D*h*w) per batch element); the per-view warped volumes of the
// reference are never materialised.  Feature maps are first repacked channel-last with a zero border
// ((h+3,w+3,C), 128 B per pixel at C=32): one bilinear tap of one pixel is a single full cache line shared
// by C/4 lanes, and zero padding costs no in-bounds logic (the clamped sample position lands on zero taps).
//
// This file: the entry points, the repacking and composing prologues, the dispatcher (launch_k3) and the GATHER kernel, which
// takes every call the tile kernel (warp_variance_tile.hip: C = 32 channel-last volumes, maps up to 65,532 px a side) does
// not: NCDHW volumes, C != 32, homo_warp, longer maps.  Thread mapping: C/4 lanes per output pixel (each lane owns 4
// channels = one 16-B load per tap), 256/(C/4) consecutive x pixels per workgroup, one (b, d, y) row segment per
// workgroup.  The earlier forms of K3 live in warp_variance_exp.hip (experiments library).
#include "mvd_common.h"
#include "warp_variance_common.h"

namespace mvd {


// M[v][b] = (src_proj[v][b] @ key_proj_inv[b])[:3,:4] as an fmaf chain over k (what a K=4 sgemm does):
// computed once per call by a one-block prologue kernel; the main kernel reads the 12 floats through the
// scalar cache instead of redoing a uniform 4x4 product in every lane.
__global__ void compose_transforms_kernel(ViewPtrs proj, const float* __restrict__ key_proj_inv, int B, int V,
                                          float* __restrict__ M) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= V * B * 12) return;
    const int j = e % 4, i = (e / 4) % 3, b = (e / 12) % B, v = e / (12 * B);
    const float* P = proj.p[v] + b * 16;
    const float* Q = key_proj_inv + b * 16;
    float acc = P[i * 4 + 0] * Q[0 * 4 + j];
    acc = fmaf(P[i * 4 + 1], Q[1 * 4 + j], acc);
    acc = fmaf(P[i * 4 + 2], Q[2 * 4 + j], acc);
    acc = fmaf(P[i * 4 + 3], Q[3 * 4 + j], acc);
    M[e] = acc;
}
void launch_compose_transforms(const ViewPtrs& proj, const float* key_proj_inv, int B, int V, float* M, hipStream_t st) {
    hipLaunchKernelGGL(compose_transforms_kernel, dim3((unsigned)((V * B * 12 + 255) / 256)), dim3(256), 0, st, proj, key_proj_inv,
                       B, V, M);
}

// (N, C, h, w) -> channel-last with a zero border: (N, h+3, w+3, C), pixel (y, x) at padded (y+1, x+1).
// Rows/cols -1, w and w+1 (h, h+1) stay zero (the buffer is cleared first), so a bilinear sample whose
// position is clamped to [-1, w] x [-1, h] needs no in-bounds logic: out-of-image taps read zeros.
__global__ void __launch_bounds__(256) repack_padded_kernel(const float* __restrict__ src, float* __restrict__ dst, int C,
                                                            int h, int w) {
    __shared__ float tile[32][33];
    const int n = blockIdx.z;
    const long long hw = (long long)h * w;
    const long long p0 = (long long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + ty + 8 * k;
        const long long pix = p0 + tx;
        if (c < C && pix < hw) tile[ty + 8 * k][tx] = src[((long long)n * C + c) * hw + pix];
    }
    __syncthreads();
    const int W2 = w + 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long pix = p0 + ty + 8 * k;
        const int c = c0 + tx;
        if (c < C && pix < hw) {
            const int y = (int)(pix / w), x = (int)(pix - (long long)y * w);
            dst[(((long long)n * (h + 3) + y + 1) * W2 + x + 1) * C + c] = tile[tx][ty + 8 * k];
        }
    }
}


// The 4 planes of a workgroup for one source view when the WAVE's re-gather pattern is MASK (bit i-1: some lane's
// 2x2 cell differs between plane i-1 and plane i).  Planes whose bit is clear reuse the previous plane's registers
// outright — no per-lane select, no exec masking: the texture path charges a gather instruction the same whether 1
// or 64 lanes are active, so re-gathering for the whole wave costs nothing extra, and a pattern known at compile time
// lets every load be issued up front and waited for with exact counts.
template <int MASK>
__device__ __forceinline__ void gather_blend_4planes(float4 (&s1)[4], float4 (&s2)[4], const float (&wt)[4][4],
                                                     const unsigned (&off)[4], __amdgpu_buffer_rsrc_t rsrc, unsigned rowb,
                                                     unsigned pix) {
    u32x4 f[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i == 0 || ((MASK >> (i - 1)) & 1)) gather_cell<RowPitch::in_voffset>(f[i], rsrc, off[i], rowb, pix);
    }
    int src = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i > 0 && ((MASK >> (i - 1)) & 1)) src = i;
        accumulate_cell(s1[i], s2[i], wt[i], f[src]);
    }
}

// Work decomposition (the part that decides where the tap gathers are served from):
//   * a workgroup owns one row segment of PPB key pixels and DPB consecutive depth planes; for each view
//     it computes the DPB sample positions, issues all 4*DPB gathers back to back (buffer loads: SGPR
//     descriptor + one 32-bit offset per sample, the 4 taps at constant strides from it) and only then
//     accumulates, so the gathers of a view overlap each other and consecutive planes touch (nearly) the
//     same source lines;
//   * the 1-D grid is decoded XCD-first (decode_xcd_first): each XCD owns a contiguous band of key rows for ALL planes --
//     with a plane-major grid every XCD streamed all V source images per plane and the gathers were served by the Infinity
//     Cache (measured 2.8 ms at the headline shape, profiles/r01_*).
// Placement only affects speed; results do not depend on it.
template <int LPP, bool WARP_ONLY, int DPB, int MINW, Reuse REUSE = Reuse::none, bool EXACT = false>
__global__ void __launch_bounds__(256, MINW) warp_variance_kernel(WarpParams p) {
    constexpr int PPB = 256 / LPP;  // pixels per block
    constexpr int C = LPP * 4;
    constexpr unsigned PIX = LPP * 16;  // bytes per pixel
    __shared__ float stage[C * (PPB + 1)];

    const int tid = threadIdx.x;
    const int q = tid % LPP;   // channel quad
    const int px = tid / LPP;  // pixel within the block
    const int h = p.h, w = p.w, D = p.D;

    // ---- decode: one row segment of PPB key pixels, DPB planes ----
    const BlockWork blk = decode_xcd_first(blockIdx.x, (D + DPB - 1) / DPB, p.tiles_per_xcd);
    const int b = blk.b;
    if (blk.tile >= p.tiles_x * h) return;  // block-uniform
    const int y = blk.tile / p.tiles_x;
    const int x0 = (blk.tile - y * p.tiles_x) * PPB;
    const int x = x0 + px;
    const int d0 = blk.chunk * DPB;
    const bool active = x < w;
    const int xc = active ? x : w - 1;

    // Path B has no in-bounds mask, so the folded grid's few-ulp difference moves a sample by < 1e-4 px and the output continuously
    const float sx = grid_scale<EXACT>(w), sy = grid_scale<EXACT>(h);
    const float fx = (float)xc, fy = (float)y;
    const float xhi = (float)w, yhi = (float)h;
    const int W2 = w + 3;
    const float W2f = (float)W2;
    const unsigned rowb = (unsigned)W2 * PIX;                    // bytes per padded row
    const unsigned img_bytes = (unsigned)(h + 3) * rowb;         // bytes per padded image
    const unsigned org = rowb + PIX + (unsigned)q * 16;          // padded (1,1) + this lane's channel quad

    // ---- key: both sums start from the key features ----
    float4 s1[DPB], s2[DPB];
    if constexpr (!WARP_ONLY) {
        const float4 k = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.key) + (size_t)b * img_bytes +
                                                          org + (unsigned)y * rowb + (unsigned)xc * PIX);
        const float4 k2 = make_float4(k.x * k.x, k.y * k.y, k.z * k.z, k.w * k.w);
#pragma unroll
        for (int i = 0; i < DPB; ++i) { s1[i] = k; s2[i] = k2; }
    } else {
#pragma unroll
        for (int i = 0; i < DPB; ++i) { s1[i] = make_float4(0, 0, 0, 0); s2[i] = s1[i]; }
    }
    const float* __restrict__ dvals = p.depth + (size_t)b * D;
    float dep[DPB];
#pragma unroll
    for (int i = 0; i < DPB; ++i) dep[i] = dvals[min(d0 + i, D - 1)];
    const float mydep = dvals[min(d0 + (q & 3), D - 1)];  // the plane this lane locates for its quad (DPB == 4)

    // the next view's transform and base pointer are fetched (scalar loads) while the current view is processed
    float Mn[12];
    const char* srcn;
    auto fetch_view = [&](int v) {
        const float* __restrict__ Mv = p.M + ((size_t)v * p.B + b) * 12;  // wave-uniform: scalar loads
#pragma unroll
        for (int k = 0; k < 12; ++k) Mn[k] = Mv[k];
        srcn = reinterpret_cast<const char*>(p.src.p[v]);
    };
    fetch_view(0);
    const int nviews = p.V;
    for (int v = 0; v < nviews; ++v) {
        float M[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) M[k] = Mn[k];
        const char* srcv = srcn;
        fetch_view(min(v + 1, p.V - 1));
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(srcv + (size_t)b * img_bytes), 0, (int)img_bytes,
            0x00020000);
        unsigned off[DPB];
        float wt[DPB][4];  // bilinear weights of the taps nw, ne, sw, se

        // ---- locate: a plane's cell weights; returns the byte offset of (yf, xf), which is (yf+1, xf+1) in the padded image once
        // `org` is added.  With 32 channels the padded map has < 2^24 pixels (checked on the host), so yf*W2 + xf is exact in
        // fp32 and replaces a quarter-rate integer multiply.
        auto locate = [&](float depth, CellWeights& c) {
            const SamplePos P = sample_position<EXACT>(M, fx, fy, depth, sx, sy, xhi, yhi);
            c = cell_weights(P.ix, P.iy);
            if constexpr (LPP == 8) return (unsigned)(int)fmaf(c.yf, W2f, c.xf) * PIX;
            else return (unsigned)((int)c.yf * W2 + (int)c.xf) * PIX;
        };
        if constexpr (DPB == 4 && LPP % 4 == 0) {
            // the LPP lanes of a pixel would each repeat this arithmetic for all 4 planes; instead lane (q & 3) of every
            // quad does plane (q & 3) and the quad exchanges the results with DPP quad_perm broadcasts
            CellWeights m;
            const unsigned mpo = locate(mydep, m);
            if constexpr (REUSE == Reuse::wave_uniform_late) {
                off[0] = org + quad_bcast<0>(mpo); off[1] = org + quad_bcast<1>(mpo);
                off[2] = org + quad_bcast<2>(mpo); off[3] = org + quad_bcast<3>(mpo);
                // four waves per SIMD (128 VGPRs): the weights stay in the locating lane until a plane's arithmetic needs them (4
                // DPP broadcasts right there instead of 16 registers held through the gathers), at most three cells in flight
                dispatch_mask(cell_change_mask(off), [&](auto mask) {
                    gather_blend_4planes_3sets<decltype(mask)::value>(
                        s1, s2, off,
                        [&](auto I) {
                            constexpr int i = decltype(I)::value;
                            return make_float4(quad_bcast<i>(m.w00()), quad_bcast<i>(m.w10()), quad_bcast<i>(m.w01()), quad_bcast<i>(m.w11()));
                        },
                        [&](u32x4 (&f)[4], unsigned o) { gather_cell<RowPitch::in_voffset>(f, rsrc, o, rowb, PIX); });
                });
                continue;
            }
            auto bcast = [&](auto I) {
                constexpr int i = decltype(I)::value;
                wt[i][0] = quad_bcast<i>(m.w00()); wt[i][1] = quad_bcast<i>(m.w10()); wt[i][2] = quad_bcast<i>(m.w01()); wt[i][3] = quad_bcast<i>(m.w11());
                off[i] = org + quad_bcast<i>(mpo);
            };
            bcast(std::integral_constant<int, 0>{}); bcast(std::integral_constant<int, 1>{});
            bcast(std::integral_constant<int, 2>{}); bcast(std::integral_constant<int, 3>{});
        } else {
#pragma unroll
            for (int i = 0; i < DPB; ++i) {
                CellWeights c;
                off[i] = org + locate(dep[i], c);
                wt[i][0] = c.w00(); wt[i][1] = c.w10(); wt[i][2] = c.w01(); wt[i][3] = c.w11();
            }
        }

        // ---- pattern and gather-blend ----
        if constexpr (REUSE == Reuse::wave_uniform && DPB == 4) {
            // (its own switch, not dispatch_mask: through the closure the compiler sinks the eight cases' final adds into one
            // tail block, which changes both product instances throughout and costs the warp-only one 4 VGPRs, 118 -> 122)
            switch (cell_change_mask(off)) {
                case 0: gather_blend_4planes<0>(s1, s2, wt, off, rsrc, rowb, PIX); break;
                case 1: gather_blend_4planes<1>(s1, s2, wt, off, rsrc, rowb, PIX); break;
                case 2: gather_blend_4planes<2>(s1, s2, wt, off, rsrc, rowb, PIX); break;
                case 3: gather_blend_4planes<3>(s1, s2, wt, off, rsrc, rowb, PIX); break;
                case 4: gather_blend_4planes<4>(s1, s2, wt, off, rsrc, rowb, PIX); break;
                case 5: gather_blend_4planes<5>(s1, s2, wt, off, rsrc, rowb, PIX); break;
                case 6: gather_blend_4planes<6>(s1, s2, wt, off, rsrc, rowb, PIX); break;
                default: gather_blend_4planes<7>(s1, s2, wt, off, rsrc, rowb, PIX); break;
            }
            continue;
        }
        u32x4 f[DPB][4];
        if constexpr (REUSE == Reuse::per_lane) {
            // Sweep coherence: from one plane to the next a sample moves a fraction of a pixel, so its 2x2 cell is
            // usually the previous plane's.  Only lanes whose cell moved gather again (exec-masked loads, all issued
            // before the first use); the others take the previous plane's registers.
            bool moved[DPB];
#pragma unroll
            for (int i = 0; i < DPB; ++i) {
                moved[i] = i == 0 || off[i] != off[i - 1];
                if (moved[i]) gather_cell<RowPitch::in_voffset>(f[i], rsrc, off[i], rowb, PIX);
            }
#pragma unroll
            for (int i = 1; i < DPB; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    f[i][k].x = moved[i] ? f[i][k].x : f[i - 1][k].x;
                    f[i][k].y = moved[i] ? f[i][k].y : f[i - 1][k].y;
                    f[i][k].z = moved[i] ? f[i][k].z : f[i - 1][k].z;
                    f[i][k].w = moved[i] ? f[i][k].w : f[i - 1][k].w;
                }
        } else {
#pragma unroll
            for (int i = 0; i < DPB; ++i) gather_cell<RowPitch::in_voffset>(f[i], rsrc, off[i], rowb, PIX);
        }
#pragma unroll
        for (int i = 0; i < DPB; ++i) accumulate_cell(s1[i], s2[i], wt[i], f[i]);
    }

    // ---- finish and store ----
    const float inv_nv = 1.0f / (float)(p.V + 1);  // mvsnet.py:135, V there counts the key view
    const size_t plane = (size_t)h * w;
#pragma unroll
    for (int i = 0; i < DPB; ++i) {
        const int d = d0 + i;
        if (d >= D) break;  // block-uniform
        const float4 r = WARP_ONLY ? s1[i] : variance_finish(s1[i], s2[i], inv_nv);
        if (p.layout == MVD_LAYOUT_NDHWC) {
            if (active)
                *reinterpret_cast<float4*>(p.out + ((((size_t)b * D + d) * h + y) * w + x) * C + q * 4) = r;
            continue;
        }
        // NCDHW: transpose the (pixel, channel) tile through LDS so every channel row is written as
        // PPB consecutive floats.
        __syncthreads();
        stage[(q * 4 + 0) * (PPB + 1) + px] = r.x;
        stage[(q * 4 + 1) * (PPB + 1) + px] = r.y;
        stage[(q * 4 + 2) * (PPB + 1) + px] = r.z;
        stage[(q * 4 + 3) * (PPB + 1) + px] = r.w;
        __syncthreads();
#pragma unroll
        for (int e0 = 0; e0 < C * PPB / 256; ++e0) {
            const int e = tid + e0 * 256;
            const int c = e / PPB, xx = e % PPB;
            if (x0 + xx < w)
                p.out[(((size_t)b * C + c) * D + d) * plane + (size_t)y * w + x0 + xx] = stage[c * (PPB + 1) + xx];
        }
    }
}

static size_t padded_image_floats(int C, int h, int w) { return (size_t)(h + 3) * (w + 3) * C; }
static size_t padded_slot_bytes(int B, int C, int h, int w) {
    return align_up((size_t)B * padded_image_floats(C, h, w) * sizeof(float), 256);
}

// clears the slot and writes the zero-bordered channel-last copy of one (B,C,h,w) feature map into it
static int repack_padded(const float* src, float* dst, int B, int C, int h, int w, hipStream_t st) {
    if (hipMemsetAsync(dst, 0, padded_slot_bytes(B, C, h, w), st) != hipSuccess) return launch_status("repack: memset");
    const long long hw = (long long)h * w;
    dim3 grid((unsigned)((hw + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)B);
    hipLaunchKernelGGL(repack_padded_kernel, grid, dim3(256), 0, st, src, dst, C, h, w);
    return launch_status("repack_padded");
}

int repack_padded_launch(const float* src, float* dst, int B, int C, int h, int w, hipStream_t st) {
    return repack_padded(src, dst, B, C, h, w, st);
}
size_t padded_slot_bytes_public(int B, int C, int h, int w) { return padded_slot_bytes(B, C, h, w); }

// The gather kernel in one compiled form: LPP lanes per pixel, DPB planes per workgroup; the grid is decoded XCD-first (see
// the kernel)
int launch_gather(const WarpParams& p0, int lpp, int dpb, WarpKernel kernel, hipStream_t st) {
    WarpParams p = p0;
    const int ppb = 256 / lpp;
    p.tiles_x = (p.w + ppb - 1) / ppb;
    const long long tiles = (long long)p.tiles_x * p.h;
    p.tiles_per_xcd = (int)((tiles + 7) / 8);
    const long long nblk = 8LL * p.tiles_per_xcd * ((p.D + dpb - 1) / dpb) * p.B;
    if (nblk > 0x7fffffffLL) {
        set_error("warp_variance: %lld workgroups exceed the grid limit", nblk);
        return MVD_ERR_INVALID_ARG;
    }
    timing_begin(st);
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(256), 0, st, p);
    timing_end(st);
    return launch_status("warp_variance");
}

// The product's forms of the gather kernel: 4 planes per workgroup, 3 waves per SIMD (tuned on MI355X); with
// 8 lanes per pixel (C = 32) on the folded grid, a plane's cell is gathered again only where the wave needs it
template <bool WARP_ONLY, bool EXACT>
static WarpKernel gather_kernel(int lpp) {
    switch (lpp) {
        case 1: return warp_variance_kernel<1, WARP_ONLY, 4, 3, Reuse::none, EXACT>;
        case 2: return warp_variance_kernel<2, WARP_ONLY, 4, 3, Reuse::none, EXACT>;
        case 4: return warp_variance_kernel<4, WARP_ONLY, 4, 3, Reuse::none, EXACT>;
        case 8: return warp_variance_kernel<8, WARP_ONLY, 4, 3, EXACT ? Reuse::none : Reuse::wave_uniform, EXACT>;
        default: return warp_variance_kernel<16, WARP_ONLY, 4, 3, Reuse::none, EXACT>;  // C = 64
    }
}

int launch_warp_gather(const WarpParams& p, int C, bool warp_only, hipStream_t st) {  // C = 4, 8, 16, 32 or 64 (checked)
    const int lpp = C / 4;
    WarpKernel k;
    if (!p.exact_grid) {
        k = warp_only ? gather_kernel<true, false>(lpp) : gather_kernel<false, false>(lpp);
    } else if (!warp_only) {
        k = gather_kernel<false, true>(lpp);
    } else {
#ifdef MVD_EXPERIMENTS
        k = gather_kernel<true, true>(lpp);
#else
        // homo_warp has no exact-grid flag (mvd_homo_warp_f32 passes a plain layout): the product does not compile these
        set_error("homo_warp: the exact grid is not compiled into the product library");
        return MVD_ERR_INVALID_ARG;
#endif
    }
    return launch_gather(p, lpp, 4, k, st);
}

// max |x| over the FINITE values of n floats into *absmax (zeroed first): NaN and inf do not take part, so that one bad voxel
// does not set the scale of everything else.  A streaming read: 16 bytes per lane, grid-stride.
__global__ void __launch_bounds__(256) absmax_kernel(const float* __restrict__ x, long long n, unsigned* __restrict__ out) {
    __shared__ float wmax[4];
    const long long n4 = n / 4;
    float m = 0.f;
    auto take = [&m](const float4 v) {
        m = fmaxf(fmaxf(m, fmaxf(finite_abs_or_zero(v.x), finite_abs_or_zero(v.y))), fmaxf(finite_abs_or_zero(v.z), finite_abs_or_zero(v.w)));
    };
    // a contiguous segment per workgroup, eight 16-byte loads in flight per thread (with one load in flight the pass ran at 1.4 TB/s)
    const long long per_blk = ((n4 + gridDim.x - 1) / gridDim.x + 255) / 256 * 256;
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
    long long i = (long long)blockIdx.x * per_blk + threadIdx.x;
    const long long end = min(n4, ((long long)blockIdx.x + 1) * per_blk);
    for (; i + 7 * 256 < end; i += 8 * 256) {
        float4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = x4[i + k * 256];
#pragma unroll
        for (int k = 0; k < 8; ++k) take(v[k]);
    }
    for (; i < end; i += 256) take(x4[i]);
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) m = fmaxf(m, finite_abs_or_zero(x[n4 * 4 + threadIdx.x]));
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    // ONE atomic per workgroup: atomics on a single address serialise at ~10 ns each
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        raise_absmax(reinterpret_cast<float*>(out), m);
    }
}

int absmax_launch(const float* x, long long n, float* absmax, hipStream_t st) {
    if (hipMemsetAsync(absmax, 0, sizeof(float), st) != hipSuccess) return launch_status("absmax: memset");
    if (n <= 0) return MVD_OK;
    // 16 loads of 16 bytes per thread, at most 8 workgroups per CU; a workgroup ends with at most one atomic
    const long long want = (n / 4 + 4095) / 4096;
    const unsigned nblk = (unsigned)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
    hipLaunchKernelGGL(absmax_kernel, dim3(nblk), dim3(256), 0, st, x, n, reinterpret_cast<unsigned*>(absmax));
    return launch_status("absmax");
}

// K3's choice of kernel for run_warp and run_warp_f16.  The tile kernel takes every C = 32 channel-last volume whose maps it
// covers (run_warp_f16 refuses other maps); every other fp32 call runs the gather kernel.  With `absmax`, the tile kernel
// leaves max |volume| behind and sets *absmax_done; after the gather kernel the caller runs a separate pass.
static int launch_k3(const WarpParams& p0, int C, bool warp_only, bool f16, hipStream_t st, float* absmax = nullptr,
                     bool* absmax_done = nullptr) {
    WarpParams p = p0;
#ifdef MVD_EXPERIMENTS
    // experiments library: MVD_K3_CFG selects the kernel (warp_variance_exp.hip).  The gather kernel's other forms
    // (Reuse, planes per workgroup, min waves per SIMD; C = 32 on the folded grid) are instantiated here, with its template.
    if (const char* e = exp_env("MVD_K3_CFG")) {
#define MVD_G(R, DPB, MW) {Reuse::R, DPB, MW, warp_only ? warp_variance_kernel<8, true, DPB, MW, Reuse::R> : warp_variance_kernel<8, false, DPB, MW, Reuse::R>}
        const GatherForm forms[] = {MVD_G(none, 1, 8), MVD_G(none, 2, 4), MVD_G(none, 2, 6), MVD_G(none, 2, 8), MVD_G(none, 4, 2),
                                    MVD_G(none, 4, 3), MVD_G(none, 4, 4), MVD_G(none, 8, 2), MVD_G(none, 8, 3), MVD_G(per_lane, 2, 4),
                                    MVD_G(per_lane, 2, 6), MVD_G(per_lane, 4, 2), MVD_G(per_lane, 4, 3), MVD_G(per_lane, 4, 4),
                                    MVD_G(per_lane, 8, 2), MVD_G(wave_uniform, 4, 2), MVD_G(wave_uniform, 4, 3), MVD_G(wave_uniform, 4, 4),
                                    MVD_G(wave_uniform_late, 4, 2), MVD_G(wave_uniform_late, 4, 3), MVD_G(wave_uniform_late, 4, 4)};
#undef MVD_G
        return warp_variance_experiment(e, p, C, warp_only, f16, st, forms, (int)(sizeof(forms) / sizeof(forms[0])));
    }
#endif
    if (f16) return launch_warp_tile(p, st, 8, 128, 8, 1, true, false);
    if (!warp_only && C == 32 && p.layout == MVD_LAYOUT_NDHWC && warp_tile_supported(p, false)) {
        // LDS-staged footprints, 8x4 key tiles, 8-plane chunks (tools/bench_k3.py)
        if (absmax) {
            if (hipMemsetAsync(absmax, 0, sizeof(float), st) != hipSuccess) return launch_status("warp_variance: memset");
            p.absmax = absmax;
            *absmax_done = true;
        }
        return launch_warp_tile(p, st, 8, 104, 8, 1, false, p.exact_grid != 0);
    }
    return launch_warp_gather(p, C, warp_only, st);
}

// shared by the two entry points: validates, lays out the workspace, repacks, composes, launches
static int run_warp(const float* key_feat, const float* const* src_feat, const float* const* src_proj,
                    const float* key_proj_inv, const float* depth_values, int B, int C, int D, int h, int w, int V,
                    float* out, int layout, void* workspace, size_t workspace_bytes, hipStream_t st, bool warp_only,
                    float* absmax = nullptr, bool* absmax_done = nullptr) {
    const char* who = warp_only ? "homo_warp" : "warp_variance";
    MVD_REQUIRE(B > 0 && D > 0 && h > 1 && w > 1, "%s: non-positive dimension (h, w must be >= 2)", who);
    MVD_REQUIRE(V >= 1 && V <= MVD_MAX_VIEWS, "%s: V=%d outside 1..%d", who, V, MVD_MAX_VIEWS);
    MVD_REQUIRE(C == 4 || C == 8 || C == 16 || C == 32 || C == 64, "%s: C=%d unsupported (need 4, 8, 16, 32 or 64)", who, C);
    MVD_REQUIRE((long long)(h + 3) * (w + 3) * C * 4 < 0x7fffffffLL && h < (1 << 23) && w < (1 << 23),
                "%s: one padded feature map of %dx%dx%d floats exceeds the 2 GiB buffer-offset range", who, h, w, C);
    // MVD_FEAT_NHWC_BORDER: the caller's maps already are zero-bordered channel-last copies (K6 writes them); only the
    // composed transforms need workspace
    const bool staged = (layout & MVD_FEAT_NHWC_BORDER) != 0;
    const size_t need = staged ? align_up((size_t)MVD_MAX_VIEWS * B * 12 * sizeof(float), 256)
                               : mvd_warp_variance_workspace_bytes(B, C, h, w, warp_only ? 0 : V);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu B < required %zu B", who, workspace_bytes, need);
        return MVD_ERR_WORKSPACE;
    }
    const size_t slot = padded_slot_bytes(B, C, h, w);
    char* ws = (char*)workspace;
    WarpParams p{};
    p.M = (float*)ws;
    ws += align_up((size_t)MVD_MAX_VIEWS * B * 12 * sizeof(float), 256);
    int rc;
    if (!warp_only) {
        if (staged) {
            p.key = key_feat;
        } else {
            rc = repack_padded(key_feat, (float*)ws, B, C, h, w, st);
            if (rc) return rc;
            p.key = (float*)ws;
            ws += slot;
        }
    }
    for (int v = 0; v < V; ++v) {
        MVD_REQUIRE(src_feat[v] && src_proj[v], "%s: NULL view %d", who, v);
        if (staged) {
            p.src.p[v] = src_feat[v];
        } else {
            rc = repack_padded(src_feat[v], (float*)ws, B, C, h, w, st);
            if (rc) return rc;
            p.src.p[v] = (float*)ws;
            ws += slot;
        }
        p.proj.p[v] = src_proj[v];
    }
    launch_compose_transforms(p.proj, key_proj_inv, B, V, const_cast<float*>(p.M), st);
    rc = launch_status("compose_transforms");
    if (rc) return rc;
    p.key_proj_inv = key_proj_inv;
    p.depth = depth_values;
    p.out = out;
    p.B = B; p.D = D; p.h = h; p.w = w; p.V = V;
    p.layout = layout & 0xff;
    p.exact_grid = (layout & MVD_GRID_EXACT) ? 1 : 0;
    return launch_k3(p, C, warp_only, false, st, absmax, absmax_done);
}

// fp16-feature variant (BASELINE configs[3]): features arrive as fp16 zero-bordered channel-last maps, the volume
// leaves as fp16 channel-last; everything in between is the fp32 arithmetic of the tile kernel, which must cover the maps
static int run_warp_f16(const void* key_feat, const void* const* src_feat, const float* const* src_proj,
                        const float* key_proj_inv, const float* depth_values, int B, int D, int h, int w, int V, void* out,
                        void* workspace, size_t workspace_bytes, hipStream_t st) {
    const char* who = "warp_variance_f16";
    MVD_REQUIRE(B > 0 && D > 0 && h > 1 && w > 1, "%s: non-positive dimension (h, w must be >= 2)", who);
    MVD_REQUIRE(V >= 1 && V <= MVD_MAX_VIEWS, "%s: V=%d outside 1..%d", who, V, MVD_MAX_VIEWS);
    MVD_REQUIRE((long long)(h + 3) * (w + 3) * 64 < 0x7fffffffLL && h < (1 << 23) && w < (1 << 23),
                "%s: one padded feature map of %dx%dx32 halves exceeds the 2 GiB buffer-offset range", who, h, w);
    const size_t need = align_up((size_t)MVD_MAX_VIEWS * B * 12 * sizeof(float), 256);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu B < required %zu B", who, workspace_bytes, need);
        return MVD_ERR_WORKSPACE;
    }
    WarpParams p{};
    p.M = (float*)workspace;
    p.key = (const float*)key_feat;
    for (int v = 0; v < V; ++v) {
        MVD_REQUIRE(src_feat[v] && src_proj[v], "%s: NULL view %d", who, v);
        p.src.p[v] = (const float*)src_feat[v];
        p.proj.p[v] = src_proj[v];
    }
    p.key_proj_inv = key_proj_inv;
    p.depth = depth_values;
    p.out = (float*)out;
    p.B = B; p.D = D; p.h = h; p.w = w; p.V = V;
    p.layout = MVD_LAYOUT_NDHWC;
    MVD_REQUIRE(warp_tile_supported(p, true), "%s: maps of %dx%d are outside the fp16 kernel's range (h, w <= 65532 and h*w*64 < 2^31)",
                who, h, w);
    launch_compose_transforms(p.proj, key_proj_inv, B, V, const_cast<float*>(p.M), st);
    const int rc = launch_status("compose_transforms");
    if (rc) return rc;
    return launch_k3(p, 32, false, true, st);
}

template <bool TO_HALF>
__global__ void __launch_bounds__(256) convert_kernel(const void* __restrict__ src, void* __restrict__ dst, long long n4) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // 4 elements per thread
    if (i >= n4) return;
    if constexpr (TO_HALF) {
        const float4 v = reinterpret_cast<const float4*>(src)[i];
        const f16x2 lo = {(_Float16)v.x, (_Float16)v.y}, hi = {(_Float16)v.z, (_Float16)v.w};
        reinterpret_cast<u32x2*>(dst)[i] = u32x2{as_u32(lo), as_u32(hi)};
    } else {
        const u32x2 v = reinterpret_cast<const u32x2*>(src)[i];
        const f16x2 lo = as_h2(v.x), hi = as_h2(v.y);
        reinterpret_cast<float4*>(dst)[i] = make_float4((float)lo.x, (float)lo.y, (float)hi.x, (float)hi.y);
    }
}

template <bool TO_HALF>
static int convert(const void* src, void* dst, long long n, hipStream_t st) {
    MVD_REQUIRE(src && dst && n > 0 && n % 4 == 0, "convert: NULL argument or element count not a positive multiple of 4");
    const long long n4 = n / 4, nblk = (n4 + 255) / 256;
    MVD_REQUIRE(nblk <= 0x7fffffffLL, "convert: too many elements");
    hipLaunchKernelGGL(convert_kernel<TO_HALF>, dim3((unsigned)nblk), dim3(256), 0, st, src, dst, n4);
    return launch_status("convert");
}

}  // namespace mvd

extern "C" {

size_t mvd_warp_variance_f16_workspace_bytes(int B) {
    return B > 0 ? mvd::align_up((size_t)MVD_MAX_VIEWS * B * 12 * sizeof(float), 256) : 0;
}

int mvd_warp_variance_f16(const void* key_feat, const void* const* src_feat, const float* const* src_proj,
                          const float* key_proj_inv, const float* depth_values, int B, int D, int h, int w, int V,
                          void* var_out, void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    MVD_REQUIRE(key_feat && src_feat && src_proj && key_proj_inv && depth_values && var_out, "warp_variance_f16: NULL argument");
    return mvd::run_warp_f16(key_feat, src_feat, src_proj, key_proj_inv, depth_values, B, D, h, w, V, var_out, workspace,
                             workspace_bytes, (hipStream_t)stream);
}

int mvd_convert_f32_to_f16(const float* src, void* dst, long long n, mvd_stream_t stream) {
    return mvd::convert<true>(src, dst, n, (hipStream_t)stream);
}
int mvd_convert_f16_to_f32(const void* src, float* dst, long long n, mvd_stream_t stream) {
    return mvd::convert<false>(src, dst, n, (hipStream_t)stream);
}

size_t mvd_warp_variance_workspace_bytes(int B, int C, int h, int w, int V) {
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || V < 0) return 0;
    // transforms + (V + 1) zero-bordered channel-last feature copies (V = 0: homo_warp, one copy)
    return mvd::align_up((size_t)MVD_MAX_VIEWS * B * 12 * sizeof(float), 256) +
           (size_t)(V + 1) * mvd::padded_slot_bytes(B, C, h, w);
}

int mvd_warp_variance_f32(const float* key_feat, const float* const* src_feat, const float* const* src_proj,
                          const float* key_proj_inv, const float* depth_values, int B, int C, int D, int h, int w,
                          int V, float* var_out, int out_layout, void* workspace, size_t workspace_bytes,
                          mvd_stream_t stream) {
    MVD_REQUIRE(key_feat && src_feat && src_proj && key_proj_inv && depth_values && var_out,
                "warp_variance: NULL argument");
    MVD_REQUIRE((out_layout & 0xff) == MVD_LAYOUT_NCDHW || (out_layout & 0xff) == MVD_LAYOUT_NDHWC, "warp_variance: bad layout");
    return mvd::run_warp(key_feat, src_feat, src_proj, key_proj_inv, depth_values, B, C, D, h, w, V, var_out, out_layout,
                         workspace, workspace_bytes, (hipStream_t)stream, false);
}

int mvd_warp_variance_absmax_f32(const float* key_feat, const float* const* src_feat, const float* const* src_proj,
                                 const float* key_proj_inv, const float* depth_values, int B, int C, int D, int h, int w,
                                 int V, float* var_out, float* absmax_out, int out_layout, void* workspace, size_t workspace_bytes,
                                 mvd_stream_t stream) {
    MVD_REQUIRE(key_feat && src_feat && src_proj && key_proj_inv && depth_values && var_out && absmax_out,
                "warp_variance_absmax: NULL argument");
    MVD_REQUIRE((out_layout & 0xff) == MVD_LAYOUT_NCDHW || (out_layout & 0xff) == MVD_LAYOUT_NDHWC, "warp_variance: bad layout");
    bool done = false;
    int rc = mvd::run_warp(key_feat, src_feat, src_proj, key_proj_inv, depth_values, B, C, D, h, w, V, var_out, out_layout,
                           workspace, workspace_bytes, (hipStream_t)stream, false, absmax_out, &done);
    if (rc == MVD_OK && !done) rc = mvd::absmax_launch(var_out, (long long)B * C * D * h * w, absmax_out, (hipStream_t)stream);
    return rc;
}

int mvd_absmax_f32(const float* x, long long n, float* absmax, mvd_stream_t stream) {
    MVD_REQUIRE(x && absmax && n >= 0, "absmax: NULL argument or negative count");
    return mvd::absmax_launch(x, n, absmax, (hipStream_t)stream);
}

int mvd_homo_warp_f32(const float* src_feat, const float* src_proj, const float* key_proj_inv,
                      const float* depth_values, int B, int C, int D, int h, int w, float* warped_out,
                      void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    MVD_REQUIRE(src_feat && src_proj && key_proj_inv && depth_values && warped_out, "homo_warp: NULL argument");
    const float* srcs[1] = {src_feat};
    const float* projs[1] = {src_proj};
    return mvd::run_warp(nullptr, srcs, projs, key_proj_inv, depth_values, B, C, D, h, w, 1, warped_out,
                         MVD_LAYOUT_NCDHW, workspace, workspace_bytes, (hipStream_t)stream, true);
}
}

