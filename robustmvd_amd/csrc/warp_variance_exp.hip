// Experimental and retired forms of K3, all bit-identical to the product kernels (DESIGN.md section 4 records the
// measurements): the round-1 LDS-staged, wave-autonomous and quad-per-pixel forms, the round-2 located and marching kernels
// (the product's K3 before the tile kernel), and warp_variance_experiment(), which reads the MVD_K3_CFG selector.
// NOT part of libmvd_hip.so: compiled only into robustmvd_amd/lib_exp/libmvd_hip_exp.so (`make exp`, -DMVD_EXPERIMENTS),
// which tools/ and tests/test_hip_shapes.py::test_warp_variance_experimental_variants_match_default load explicitly.
#include "warp_variance_common.h"

namespace mvd {

// Footprint copy of the LDS-staged kernel, global -> LDS directly (LDS-DMA, no staging registers): wave r moves box
// rows r, r+4, ...; one instruction writes 64 consecutive float4s (1 KiB) of an LDS row, so rows are pitched to
// LDS_ROWQ float4s and a row tail that overshoots `rowq` lands in the row's own padding.
constexpr int LDS_ROWQ = 128;  // float4s per LDS row = 16 pixels of 32 channels
template <int NROW, int NCOL>
__device__ __forceinline__ void lds_dma_copy(float4* __restrict__ dst, const float4* __restrict__ g, int pitchq, int rowq,
                                             int rh, int wave, int lane) {
#pragma unroll
    for (int r = 0; r < NROW; ++r) {
        const int row = wave + 4 * r;
        if (row < rh) {  // wave-uniform
#pragma unroll
            for (int c = 0; c < NCOL; ++c)
                if (c * 64 < rowq)  // wave-uniform
                    __builtin_amdgcn_global_load_lds(
                        (const __attribute__((address_space(1))) void*)(g + (size_t)row * pitchq + min(lane + 64 * c, rowq - 1)),
                        (__attribute__((address_space(3))) void*)(dst + row * LDS_ROWQ + c * 64), 16, 0, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// LDS-staged form (C = 32, channel-last output): taps come from LDS (256 B/clk/CU) instead of the L1 /
// texture-addresser path (64 B/clk/CU), which is what bounds the direct kernel above (TA 84 % busy).
//
// A workgroup owns an 8x8 key tile for ND consecutive planes.  Per source view it copies the tile's source
// FOOTPRINT — the axis-aligned bounding box of all its samples in the zero-bordered image — into one of two
// LDS buffers with coalesced row loads, and takes every bilinear tap from there with ds_read_b128.  The copy
// of view v+1 is issued (global -> registers) before the taps of view v are computed and written to the other
// buffer afterwards: one barrier per view, the L2 latency of the copy hidden under a view's worth of work.
//
// Footprint bound: for a fixed plane the homography maps the tile to a convex quad, and for a fixed pixel the
// sample moves monotonically along its epipolar line with depth, so — as long as Z > 0 at the 8 corners (tile
// corners x first/last plane), which bounds Z > 0 in between because Z is multilinear in (x, y, d) — every
// (clamped) sample lies in the bounding box of the 8 clamped corner samples.  A box that does not fit the LDS
// buffer, or a corner with Z <= 0, sends that (tile, chunk, view) down the direct-gather path (block-uniform).
// Tap coordinates are clamped into the staged box, so a sample pushed across a box edge by rounding
// (weight < 1e-5) still reads valid LDS.  Results are bit-identical to the direct kernel.
template <int ND>
__global__ void __launch_bounds__(256, 2) warp_variance_lds_kernel(WarpParams p) {
    constexpr int C = 32, Q = 8, TX = 8, TY = 4;
    constexpr unsigned PIX = 128;
    constexpr int RH_MAX = 12, ROWQ_MAX = LDS_ROWQ;  // boxes up to 12 rows x 16 pixels: 24 KiB per buffer
    constexpr int NROW = RH_MAX / 4, NCOL = ROWQ_MAX / 64;
    __shared__ float4 region[2][RH_MAX * LDS_ROWQ];  // 48 KiB -> 3 workgroups per CU

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int q = tid & 7;
    const int slot = tid >> 3;  // 0..31: one pixel of the 4x8 tile per 8 lanes
    const int lx = slot & 7, ly0 = slot >> 3;
    const int h = p.h, w = p.w, D = p.D;

    const BlockWork blk = decode_xcd_first(blockIdx.x, (D + ND - 1) / ND, p.tiles_per_xcd);
    const int b = blk.b, tile = blk.tile;
    if (tile >= p.tiles_x * p.tiles_y) return;  // block-uniform
    const int tyi = tile / p.tiles_x;
    const int x0 = (tile - tyi * p.tiles_x) * TX, y0 = tyi * TY;
    const int d0 = blk.chunk * ND;
    const int dl = min(d0 + ND, D) - 1;

    const float sx = (float)w / (float)(w - 1), sy = (float)h / (float)(h - 1);
    const float xhi = (float)w, yhi = (float)h;
    const int W2 = w + 3;
    const unsigned rowb = (unsigned)W2 * PIX;
    const unsigned img_bytes = (unsigned)(h + 3) * rowb;
    const int xs = min(x0 + lx, w - 1);
    const int ys[1] = {min(y0 + ly0, h - 1)};
    const float fxs = (float)xs;
    const float* __restrict__ dvals = p.depth + (size_t)b * D;
    float dep[ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) dep[i] = dvals[min(d0 + i, D - 1)];
    const float dfirst = dvals[d0], dlast = dvals[dl];
    const float cxs[2] = {(float)x0, (float)min(x0 + TX - 1, w - 1)};
    const float cys[2] = {(float)y0, (float)min(y0 + TY - 1, h - 1)};

    float4 s1[1][ND], s2[1][ND];
#pragma unroll
    for (int pi = 0; pi < 1; ++pi) {
        const float4 k = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.key) + (size_t)b * img_bytes +
                                                          (unsigned)(ys[pi] + 1) * rowb + (unsigned)(xs + 1) * PIX + q * 16);
        const float4 k2 = make_float4(k.x * k.x, k.y * k.y, k.z * k.z, k.w * k.w);
#pragma unroll
        for (int i = 0; i < ND; ++i) { s1[pi][i] = k; s2[pi][i] = k2; }
    }

    // footprint box of one view in PADDED pixel coordinates (x+1, y+1); staged == it fits the LDS buffer
    struct Box { int x0, y0, rw, rh; bool staged; };
    auto footprint = [&](int v) {
        const float* __restrict__ M = p.M + ((size_t)v * p.B + b) * 12;
        float bx0 = 3e38f, bx1 = -3e38f, by0 = 3e38f, by1 = -3e38f, zmin = 3e38f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const SamplePos c = sample_position<false>(M, cxs[a & 1], cys[a >> 1], e ? dlast : dfirst, sx, sy, xhi, yhi);
                bx0 = fminf(bx0, c.ix); bx1 = fmaxf(bx1, c.ix);
                by0 = fminf(by0, c.iy); by1 = fmaxf(by1, c.iy);
                zmin = fminf(zmin, c.Z);
            }
        }
        Box bx;
        bx.x0 = (int)floorf(bx0) + 1;  // padded coordinates: pixel -1 is column 0
        bx.y0 = (int)floorf(by0) + 1;
        bx.rw = (int)floorf(bx1) + 3 - bx.x0;  // floor(bx1)+1 (second tap) +1 (padding shift) - x0 + 1
        bx.rh = (int)floorf(by1) + 3 - bx.y0;
        bx.staged = zmin > 1e-6f && bx.rh <= RH_MAX && bx.rw * Q <= ROWQ_MAX;
        return bx;
    };
    auto src_image = [&](int v) {
        return reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.src.p[v]) + (size_t)b * img_bytes);
    };
    Box cur = footprint(0);
    if (cur.staged) {
        lds_dma_copy<NROW, NCOL>(region[0], src_image(0) + ((size_t)cur.y0 * W2 + cur.x0) * Q, W2 * Q, cur.rw * Q, cur.rh, wave, lane);
    }
    __syncthreads();

    for (int v = 0; v < p.V; ++v) {
        Box nxt = cur;
        const bool has_next = v + 1 < p.V;
        if (has_next) {
            nxt = footprint(v + 1);
            if (nxt.staged)  // streams into the other buffer while this view's taps are computed
                lds_dma_copy<NROW, NCOL>(region[(v + 1) & 1], src_image(v + 1) + ((size_t)nxt.y0 * W2 + nxt.x0) * Q, W2 * Q,
                                         nxt.rw * Q, nxt.rh, wave, lane);
        }
        const float* __restrict__ M = p.M + ((size_t)v * p.B + b) * 12;
        const u32x4* __restrict__ reg = reinterpret_cast<const u32x4*>(region[v & 1]);
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(reinterpret_cast<const char*>(p.src.p[v]) + (size_t)b * img_bytes), 0, (int)img_bytes,
            0x00020000);
#pragma unroll
        for (int pi = 0; pi < 1; ++pi) {
            const float fy = (float)ys[pi];
#pragma unroll
            for (int i = 0; i < ND; ++i) {
                const SamplePos sp = sample_position<false>(M, fxs, fy, dep[i], sx, sy, xhi, yhi);
                const CellWeights cw = cell_weights(sp.ix, sp.iy);
                u32x4 f[4];
                if (cur.staged) {
                    // padded coordinates relative to the staged box, clamped into it
                    const int xi = (int)cw.xf + 1 - cur.x0, yi = (int)cw.yf + 1 - cur.y0;
                    const int xa = min(max(xi, 0), cur.rw - 1), xb = min(max(xi + 1, 0), cur.rw - 1);
                    const int ya = min(max(yi, 0), cur.rh - 1), yb = min(max(yi + 1, 0), cur.rh - 1);
                    const int ra = ya * LDS_ROWQ + q, rb = yb * LDS_ROWQ + q;
                    f[0] = reg[ra + xa * Q];
                    f[1] = reg[ra + xb * Q];
                    f[2] = reg[rb + xa * Q];
                    f[3] = reg[rb + xb * Q];
                } else {
                    gather_cell<RowPitch::in_voffset>(f, rsrc, rowb + PIX + (unsigned)q * 16 + (unsigned)((int)cw.yf * W2 + (int)cw.xf) * PIX, rowb, PIX);
                }
                const float w[4] = {cw.w00(), cw.w10(), cw.w01(), cw.w11()};
                accumulate_cell(s1[pi][i], s2[pi][i], w, f);  // same accumulation order as the direct kernel (bit-identical results)
            }
        }
        __syncthreads();  // (drains the LDS-DMA) buffer (v+1)&1 is complete; buffer v&1 is free for view v+2
        cur = nxt;
    }

    const float inv_nv = 1.0f / (float)(p.V + 1);
#pragma unroll
    for (int pi = 0; pi < 1; ++pi) {
        const int y = y0 + ly0, x = x0 + lx;
        if (y >= h || x >= w) continue;
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const int d = d0 + i;
            if (d >= D) break;
            *reinterpret_cast<float4*>(p.out + ((((size_t)b * D + d) * h + y) * w + x) * C + q * 4) = variance_finish(s1[pi][i], s2[pi][i], inv_nv);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Wave-autonomous LDS form: like warp_variance_lds_kernel, but every WAVE owns its own 4x2 key tile and its own
// pair of LDS buffers, so there is no workgroup barrier anywhere: a wave prefetches the footprint of view v+1 with
// LDS-DMA into its second buffer, waits only for the OLDER copy with a counted `s_waitcnt vmcnt(N)` (the LDS-DMA
// of the next view stays in flight) and computes view v from its first buffer.  Eight such waves per CU overlap
// each other's latencies.  Lanes: 8 pixels (4 wide x 2 high) x 8 channel quads; ND planes per task.
template <int ND>
__global__ void __launch_bounds__(256, 2) warp_variance_wave_kernel(WarpParams p) {
    constexpr int C = 32, Q = 8, TXW = 4, TYW = 2;
    constexpr unsigned PIX = 128;
    constexpr int RH = 4, ROWQ = 128;              // staged box: up to 4 rows x 16 pixels, row pitch 128 float4
    constexpr int BUF = RH * ROWQ;                 // float4s per buffer (8 KiB)
    constexpr int NDMA = RH * (ROWQ / 64);         // LDS-DMA instructions per view (always all of them: fixed count)
    extern __shared__ __attribute__((aligned(16))) float4 wlds[];  // [4 waves][2][BUF] = 64 KiB

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int q = lane & 7, pp = lane >> 3;
    const int lx = pp & 3, ly = pp >> 2;
    const int h = p.h, w = p.w, D = p.D;
    float4* __restrict__ mybuf = wlds + wave * 2 * BUF;

    // ---- task decode: xcd | d-chunk fastest | tile group (4 x-adjacent wave tiles per workgroup) | batch ----
    const BlockWork blk = decode_xcd_first(blockIdx.x, (D + ND - 1) / ND, p.tiles_per_xcd);
    const int b = blk.b, grp = blk.tile;               // group of 4 wave tiles = 16 x 2 pixels
    if (grp >= p.tiles_x * p.tiles_y) return;          // block-uniform
    const int gy = grp / p.tiles_x;
    const int x0 = (grp - gy * p.tiles_x) * (4 * TXW) + wave * TXW, y0 = gy * TYW;
    if (x0 >= w) return;                               // wave-uniform (ragged right edge)
    const int d0 = blk.chunk * ND;
    const int dl = min(d0 + ND, D) - 1;

    const float sx = (float)w / (float)(w - 1), sy = (float)h / (float)(h - 1);
    const float xhi = (float)w, yhi = (float)h;
    const int W2 = w + 3;
    const unsigned rowb = (unsigned)W2 * PIX;
    const unsigned img_bytes = (unsigned)(h + 3) * rowb;
    const int xs = min(x0 + lx, w - 1), ysr = min(y0 + ly, h - 1);
    const float fxs = (float)xs, fys = (float)ysr;
    const float* __restrict__ dvals = p.depth + (size_t)b * D;
    float dep[ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) dep[i] = dvals[min(d0 + i, D - 1)];
    const float dfirst = dvals[d0], dlast = dvals[dl];
    const float cxs[2] = {(float)x0, (float)min(x0 + TXW - 1, w - 1)};
    const float cys[2] = {(float)y0, (float)min(y0 + TYW - 1, h - 1)};

    float4 s1[ND], s2[ND];
    {
        const float4 k = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.key) + (size_t)b * img_bytes +
                                                          (unsigned)(ysr + 1) * rowb + (unsigned)(xs + 1) * PIX + q * 16);
        const float4 k2 = make_float4(k.x * k.x, k.y * k.y, k.z * k.z, k.w * k.w);
#pragma unroll
        for (int i = 0; i < ND; ++i) { s1[i] = k; s2[i] = k2; }
    }

    struct Box { int x0, y0, rw, rh; bool staged; };
    auto footprint = [&](int v) {
        const float* __restrict__ M = p.M + ((size_t)v * p.B + b) * 12;
        float bx0 = 3e38f, bx1 = -3e38f, by0 = 3e38f, by1 = -3e38f, zmin = 3e38f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const SamplePos c = sample_position<false>(M, cxs[a & 1], cys[a >> 1], e ? dlast : dfirst, sx, sy, xhi, yhi);
                bx0 = fminf(bx0, c.ix); bx1 = fmaxf(bx1, c.ix);
                by0 = fminf(by0, c.iy); by1 = fmaxf(by1, c.iy);
                zmin = fminf(zmin, c.Z);
            }
        }
        Box bx;
        bx.x0 = (int)floorf(bx0) + 1;  // padded coordinates
        bx.y0 = (int)floorf(by0) + 1;
        bx.rw = (int)floorf(bx1) + 3 - bx.x0;
        bx.rh = (int)floorf(by1) + 3 - bx.y0;
        bx.staged = zmin > 1e-6f && bx.rh <= RH && bx.rw * Q <= ROWQ;
        // wave-uniform by construction (computed from wave-uniform inputs); make it so for the compiler too
        bx.x0 = __builtin_amdgcn_readfirstlane(bx.x0);
        bx.y0 = __builtin_amdgcn_readfirstlane(bx.y0);
        bx.rw = __builtin_amdgcn_readfirstlane(bx.rw);
        bx.rh = __builtin_amdgcn_readfirstlane(bx.rh);
        bx.staged = __builtin_amdgcn_readfirstlane((int)bx.staged) != 0;
        return bx;
    };
    // exactly NDMA LDS-DMA instructions per call (rows / columns beyond the box re-read a valid element)
    auto dma = [&](int v, const Box& bx, float4* __restrict__ dst) {
        const float4* __restrict__ g = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.src.p[v]) +
                                                                         (size_t)b * img_bytes) + ((size_t)bx.y0 * W2 + bx.x0) * Q;
        const int rowq = bx.rw * Q;
#pragma unroll
        for (int r = 0; r < RH; ++r) {
            const int row = min(r, bx.rh - 1);
#pragma unroll
            for (int c = 0; c < ROWQ / 64; ++c)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(g + (size_t)row * W2 * Q + min(lane + 64 * c, rowq - 1)),
                    (__attribute__((address_space(3))) void*)(dst + r * ROWQ + c * 64), 16, 0, 0);
        }
    };

    Box cur = footprint(0);
    if (cur.staged) dma(0, cur, mybuf);

    for (int v = 0; v < p.V; ++v) {
        Box nxt = cur;
        bool next_dma = false;
        if (v + 1 < p.V) {
            nxt = footprint(v + 1);
            next_dma = nxt.staged;
            if (next_dma) dma(v + 1, nxt, mybuf + ((v + 1) & 1) * BUF);  // streams in while view v is computed
        }
        // the copy of view v must have landed; the NDMA newer instructions (view v+1) may stay in flight
        if (next_dma) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

        const float* __restrict__ M = p.M + ((size_t)v * p.B + b) * 12;
        const u32x4* __restrict__ reg = reinterpret_cast<const u32x4*>(mybuf + (v & 1) * BUF);
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(reinterpret_cast<const char*>(p.src.p[v]) + (size_t)b * img_bytes), 0, (int)img_bytes,
            0x00020000);
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const SamplePos sp = sample_position<false>(M, fxs, fys, dep[i], sx, sy, xhi, yhi);
            const CellWeights cw = cell_weights(sp.ix, sp.iy);
            u32x4 f[4];
            if (cur.staged) {
                const int xi = (int)cw.xf + 1 - cur.x0, yi = (int)cw.yf + 1 - cur.y0;
                const int xa = min(max(xi, 0), cur.rw - 1), xb = min(max(xi + 1, 0), cur.rw - 1);
                const int ya = min(max(yi, 0), cur.rh - 1), yb = min(max(yi + 1, 0), cur.rh - 1);
                const int ra = ya * ROWQ + q, rb = yb * ROWQ + q;
                f[0] = reg[ra + xa * Q];
                f[1] = reg[ra + xb * Q];
                f[2] = reg[rb + xa * Q];
                f[3] = reg[rb + xb * Q];
            } else {
                gather_cell<RowPitch::in_voffset>(f, rsrc, rowb + PIX + (unsigned)q * 16 + (unsigned)((int)cw.yf * W2 + (int)cw.xf) * PIX, rowb, PIX);
            }
            const float w[4] = {cw.w00(), cw.w10(), cw.w01(), cw.w11()};
            accumulate_cell(s1[i], s2[i], w, f);  // same accumulation order as the direct kernel (bit-identical results)
        }
        cur = nxt;
    }

    const float inv_nv = 1.0f / (float)(p.V + 1);
    const int y = y0 + ly, x = x0 + lx;
    if (y < h && x < w) {
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const int d = d0 + i;
            if (d >= D) break;
            *reinterpret_cast<float4*>(p.out + ((((size_t)b * D + d) * h + y) * w + x) * C + q * 4) = variance_finish(s1[i], s2[i], inv_nv);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Experimental (MVD_K3_CFG=q8): C = 32, channel-last output, folded grid arithmetic, ONE QUAD PER KEY PIXEL with 8
// channels per lane and 2 planes per workgroup.  The per-(pixel, plane, view) overhead of the direct kernel (position
// arithmetic, DPP broadcasts, re-gather pattern, addresses) is amortised over twice the FMAs per lane; lanes q and q^2
// of a quad both locate plane q & 1.  Bit-identical to the direct kernel.
__device__ __forceinline__ void gather_cell_q8(u32x4 (&f)[4], u32x4 (&g)[4], __amdgpu_buffer_rsrc_t rsrc, unsigned o, unsigned rowb) {
    constexpr unsigned PIX = 128;
    f[0] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o, 0, 0);
    g[0] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o + 16, 0, 0);
    f[1] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o + PIX, 0, 0);
    g[1] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o + PIX + 16, 0, 0);
    f[2] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o + rowb, 0, 0);
    g[2] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o + rowb + 16, 0, 0);
    f[3] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o + rowb + PIX, 0, 0);
    g[3] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o + rowb + PIX + 16, 0, 0);
}

template <bool ANY1>
__device__ __forceinline__ void step_q8(float4 (&s1)[2][2], float4 (&s2)[2][2], const float (&w0)[4], const float (&w1)[4],
                                        unsigned o0, unsigned o1, __amdgpu_buffer_rsrc_t rsrc, unsigned rowb) {
    u32x4 f0[4], g0[4], f1[4], g1[4];
    gather_cell_q8(f0, g0, rsrc, o0, rowb);
    if constexpr (ANY1) gather_cell_q8(f1, g1, rsrc, o1, rowb);
    accumulate_cell(s1[0][0], s2[0][0], w0, f0);
    accumulate_cell(s1[0][1], s2[0][1], w0, g0);
    accumulate_cell(s1[1][0], s2[1][0], w1, ANY1 ? f1 : f0);
    accumulate_cell(s1[1][1], s2[1][1], w1, ANY1 ? g1 : g0);
}

template <int MINW, int CPB>
__global__ void __launch_bounds__(256, MINW) warp_variance_q8_kernel(WarpParams p) {
    constexpr unsigned PIX = 128;
    const int tid = threadIdx.x;
    const int q = tid & 3;    // channels 8q .. 8q+7; locates plane d0 + (q & 1)
    const int px = tid >> 2;  // 0..63: 32 columns x 2 rows
    const int h = p.h, w = p.w, D = p.D;

    // CPB chunks of 2 planes per workgroup: one index decode and key fetch for all
    const BlockWork blk = decode_xcd_first(blockIdx.x, (D + 2 * CPB - 1) / (2 * CPB), p.tiles_per_xcd);
    const int dc = blk.chunk, b = blk.b, tile = blk.tile;
    if (tile >= p.tiles_x * p.tiles_y) return;  // block-uniform
    const int ty = tile / p.tiles_x;
    const int x = (tile - ty * p.tiles_x) * 32 + (px & 31);
    const int y = ty * 2 + (px >> 5);
    const bool active = x < w && y < h;
    const int xc = min(x, w - 1), yc = min(y, h - 1);

    const float sx = (float)w / (float)(w - 1), sy = (float)h / (float)(h - 1);
    const float fx = (float)xc, fy = (float)yc;
    const float xhi = (float)w, yhi = (float)h;
    const int W2 = w + 3;
    const float W2f = (float)W2;
    const unsigned rowb = (unsigned)W2 * PIX;
    const unsigned img_bytes = (unsigned)(h + 3) * rowb;
    const unsigned org = rowb + PIX + (unsigned)q * 32;

    float4 k0, k1;
    {
        const float4* kp = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.key) + (size_t)b * img_bytes + org +
                                                           (unsigned)yc * rowb + (unsigned)xc * PIX);
        k0 = kp[0]; k1 = kp[1];
    }
    const float inv_nv = 1.0f / (float)(p.V + 1);  // mvsnet.py:135, V there counts the key view
#pragma unroll 1
    for (int cc = 0; cc < CPB; ++cc) {
    const int d0 = (dc * CPB + cc) * 2;
    if (d0 >= D) break;  // block-uniform
    float4 s1[2][2], s2[2][2];  // [plane][channel half]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        s1[i][0] = k0; s1[i][1] = k1;
        s2[i][0] = make_float4(k0.x * k0.x, k0.y * k0.y, k0.z * k0.z, k0.w * k0.w);
        s2[i][1] = make_float4(k1.x * k1.x, k1.y * k1.y, k1.z * k1.z, k1.w * k1.w);
    }
    const float mydep = p.depth[(size_t)b * D + min(d0 + (q & 1), D - 1)];

    float Mn[12];
    const char* srcn;
    auto fetch_view = [&](int v) {
        const float* __restrict__ Mv = p.M + ((size_t)v * p.B + b) * 12;  // wave-uniform: scalar loads
#pragma unroll
        for (int k = 0; k < 12; ++k) Mn[k] = Mv[k];
        srcn = reinterpret_cast<const char*>(p.src.p[v]);
    };
    fetch_view(0);
    for (int v = 0; v < p.V; ++v) {
        float M[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) M[k] = Mn[k];
        const char* srcv = srcn;
        fetch_view(min(v + 1, p.V - 1));
        const SamplePos sp = sample_position<false>(M, fx, fy, mydep, sx, sy, xhi, yhi);
        const CellWeights m = cell_weights(sp.ix, sp.iy);
        const unsigned mpo = (unsigned)(int)fmaf(m.yf, W2f, m.xf) * PIX;  // exact in fp32 (checked on the host)
        const float wt[2][4] = {{quad_bcast<0>(m.w00()), quad_bcast<0>(m.w10()), quad_bcast<0>(m.w01()), quad_bcast<0>(m.w11())},
                                {quad_bcast<1>(m.w00()), quad_bcast<1>(m.w10()), quad_bcast<1>(m.w01()), quad_bcast<1>(m.w11())}};
        const unsigned off[2] = {org + quad_bcast<0>(mpo), org + quad_bcast<1>(mpo)};
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(srcv + (size_t)b * img_bytes), 0, (int)img_bytes, 0x00020000);
        if (__builtin_amdgcn_ballot_w64(off[1] != off[0]) != 0) step_q8<true>(s1, s2, wt[0], wt[1], off[0], off[1], rsrc, rowb);
        else step_q8<false>(s1, s2, wt[0], wt[1], off[0], off[1], rsrc, rowb);
    }

    if (active) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int d = d0 + i;
        if (d >= D) break;  // block-uniform
        float4* op = reinterpret_cast<float4*>(p.out + ((((size_t)b * D + d) * h + y) * w + x) * 32 + q * 8);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            op[hf] = variance_finish(s1[i][hf], s2[i][hf], inv_nv);
        }
    }
    }
    }
}

static int launch_warp_q8(const WarpParams& p0, hipStream_t st, int minw) {
    WarpParams p = p0;
    p.tiles_x = (p.w + 31) / 32;
    p.tiles_y = (p.h + 1) / 2;
    const long long tiles = (long long)p.tiles_x * p.tiles_y;
    p.tiles_per_xcd = (int)((tiles + 7) / 8);
    // (several 2-plane chunks per workgroup, to amortise the index decode and key fetch, measured 1.5 ms: CPB stays 1)
    const long long nblk = 8LL * p.tiles_per_xcd * ((p.D + 1) / 2) * p.B;
    if (nblk > 0x7fffffffLL) {
        set_error("warp_variance: %lld workgroups exceed the grid limit", nblk);
        return MVD_ERR_INVALID_ARG;
    }
    timing_begin(st);
    const dim3 grid((unsigned)nblk);
    if (minw == 3) hipLaunchKernelGGL((warp_variance_q8_kernel<3, 1>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((warp_variance_q8_kernel<4, 1>), grid, dim3(256), 0, st, p);
    timing_end(st);
    return launch_status("warp_variance_q8");
}

static int launch_warp_wave(const WarpParams& p0, hipStream_t st, int nd) {
    WarpParams p = p0;
    p.tiles_x = (p.w + 15) / 16;  // groups of 4 wave tiles (16 x 2 pixels)
    p.tiles_y = (p.h + 1) / 2;
    const long long groups = (long long)p.tiles_x * p.tiles_y;
    p.tiles_per_xcd = (int)((groups + 7) / 8);
    const long long nblk = 8LL * p.tiles_per_xcd * ((p.D + nd - 1) / nd) * p.B;
    if (nblk > 0x7fffffffLL) {
        set_error("warp_variance: %lld workgroups exceed the grid limit", nblk);
        return MVD_ERR_INVALID_ARG;
    }
    const size_t lds = (size_t)4 * 2 * 4 * 128 * sizeof(float4);
    timing_begin(st);
    switch (nd) {
#define MVD_W(ND)                                                                                                  \
    case ND:                                                                                                       \
        (void)hipFuncSetAttribute((const void*)warp_variance_wave_kernel<ND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL(warp_variance_wave_kernel<ND>, dim3((unsigned)nblk), dim3(256), lds, st, p);            \
        break;
        MVD_W(4) MVD_W(8)
#undef MVD_W
        default:
            set_error("warp_variance: MVD_K3_CFG wave,%d is not a compiled variant", nd);
            return MVD_ERR_INVALID_ARG;
    }
    timing_end(st);
    return launch_status("warp_variance_wave");
}

static int launch_warp_lds(const WarpParams& p0, hipStream_t st, int nd) {
    WarpParams p = p0;
    p.tiles_x = (p.w + 7) / 8;
    p.tiles_y = (p.h + 3) / 4;
    const long long tiles = (long long)p.tiles_x * p.tiles_y;
    p.tiles_per_xcd = (int)((tiles + 7) / 8);
    const long long nblk = 8LL * p.tiles_per_xcd * ((p.D + nd - 1) / nd) * p.B;
    if (nblk > 0x7fffffffLL) {
        set_error("warp_variance: %lld workgroups exceed the grid limit", nblk);
        return MVD_ERR_INVALID_ARG;
    }
    timing_begin(st);
    switch (nd) {
        case 2: hipLaunchKernelGGL(warp_variance_lds_kernel<2>, dim3((unsigned)nblk), dim3(256), 0, st, p); break;
        case 4: hipLaunchKernelGGL(warp_variance_lds_kernel<4>, dim3((unsigned)nblk), dim3(256), 0, st, p); break;
        case 8: hipLaunchKernelGGL(warp_variance_lds_kernel<8>, dim3((unsigned)nblk), dim3(256), 0, st, p); break;
        default:
            set_error("warp_variance: MVD_K3_CFG lds,%d is not a compiled variant", nd);
            return MVD_ERR_INVALID_ARG;
    }
    timing_end(st);
    return launch_status("warp_variance_lds");
}


// ------------------------------------------------------------------------------------------------
// K3, round-2 form ("located"): C = 32, channel-last output, folded grid arithmetic.
//
// What bounded the gather kernel (warp_variance.hip; profiles/r01_k3_uniform_pmc.txt): 273 M vector-ALU wave-instructions per launch
// (the SIMDs 59 % VALU-busy) of which only 85 M are the bilinear/variance FMAs; the rest is the sampling-position
// arithmetic — done by 8 lanes per pixel, i.e. twice per (pixel, plane, view) even with the quad sharing — plus 20
// DPP broadcasts per view, at 148 VGPRs = 3 waves per SIMD, too few to cover the gather latency and the store
// acknowledgements (the store stream by itself runs at 6.6 TB/s: profiles/r02_storebw.txt).
//
// Here a workgroup first LOCATES: thread t computes the position, cell offset and four bilinear weights of exactly
// one (pixel, plane, view) combination per pass (32 pixels x 4 planes x V views = 128 V combinations, no redundancy,
// view wave-uniform so the transform comes through the scalar cache) and parks them in LDS (20 B each).  After one
// barrier the same threads BLEND as before — 8 lanes per pixel, 4 channels each — but read weights and offsets from
// LDS (broadcast reads, no VALU) instead of computing and shuffling them, and keep at most three cells in flight
// (gather_blend_4planes_lds) so that the kernel fits 128 VGPRs = 4 waves per SIMD.  Same arithmetic, operation for
// operation, as warp_variance_kernel: results are bit-identical.

template <int MASK, int I, class TAP>
__device__ __forceinline__ void blend_plane_lds(float4 (&s1)[4], float4 (&s2)[4], const float4 wq, const TAP (&f)[4]) {
    const float w[4] = {wq.x, wq.y, wq.z, wq.w};
    accumulate_cell(s1[I], s2[I], w, f);
}

// the cell's taps with the row pitch in the scalar offset operand; C = 32: a pixel is 8 lanes wide
template <class TAP>
__device__ __forceinline__ void gather_cell_s(TAP (&f)[4], __amdgpu_buffer_rsrc_t rsrc, unsigned o, unsigned rowb) {
    gather_cell<RowPitch::in_soffset>(f, rsrc, o, rowb, 8u * (unsigned)sizeof(TAP));
}

// the three-set schedule with plane I's weights in LDS at wl[32 I] (broadcast reads: they land long before the gathers do)
template <int MASK, int KO = 0>
__device__ __forceinline__ void gather_blend_4planes_lds(float4 (&s1)[4], float4 (&s2)[4], const float4* __restrict__ wl,
                                                         const unsigned (&off)[4], __amdgpu_buffer_rsrc_t rsrc, unsigned rowb) {
    gather_blend_4planes_3sets<MASK>(
        s1, s2, off, [&](auto I) { return wl[32 * decltype(I)::value]; },
        [&](u32x4 (&f)[4], unsigned o) {
            if constexpr (KO & 2) {  // knock-out: taps from registers, no memory access
                f[0] = u32x4{o, o + 1, o + 2, o + 3}; f[1] = u32x4{o + 4, o + 5, o + 6, o + 7};
                f[2] = u32x4{o + rowb, o + 9, o + 10, o + 11}; f[3] = u32x4{o + rowb + 4, o + 13, o + 14, o + 15};
            } else {
                gather_cell_s(f, rsrc, o, rowb);
            }
        });
}

// KO != 0: knock-out builds that time parts of the kernel (they compute wrong results):
// 1 no locate arithmetic, 2 gathers replaced by register values, 4 no stores, 8 one view only
template <int MINW, int KO = 0>
__global__ void __launch_bounds__(256, MINW) warp_variance_located_kernel(WarpParams p) {
    constexpr int DPB = 4, PPB = 32;
    constexpr unsigned PIX = 128;
    extern __shared__ __attribute__((aligned(16))) float4 lds_loc[];  // [V][4][32] float4 weights, then [V][4][32] u32 offsets
    const int V = (KO & 8) ? 1 : p.V;
    unsigned* __restrict__ lds_off = reinterpret_cast<unsigned*>(lds_loc + V * (DPB * PPB));

    const int tid = threadIdx.x;
    const int h = p.h, w = p.w, D = p.D;

    const BlockWork blk = decode_xcd_first(blockIdx.x, (D + DPB - 1) / DPB, p.tiles_per_xcd);
    const int b = blk.b, tile = blk.tile;
    if (tile >= p.tiles_x * h) return;  // block-uniform
    const int y = tile / p.tiles_x;
    const int x0 = (tile - y * p.tiles_x) * PPB;
    const int d0 = blk.chunk * DPB;

    const int W2 = w + 3;
    const unsigned rowb = (unsigned)W2 * PIX;             // bytes per padded row
    const unsigned img_bytes = (unsigned)(h + 3) * rowb;  // bytes per padded image

    // ---- locate: one (pixel, plane, view) per thread and pass -------------------------------------------------
    {
        const int lpx = tid & 31, li = (tid >> 5) & 3;
        const int xl = min(x0 + lpx, w - 1);
        const float fx = (float)xl, fy = (float)y;
        const float sx = (float)w / (float)(w - 1), sy = (float)h / (float)(h - 1);
        const float xhi = (float)w, yhi = (float)h;
        const float W2f = (float)W2;
        const float depth = p.depth[(size_t)b * D + min(d0 + li, D - 1)];
        for (int v = __builtin_amdgcn_readfirstlane(tid >> 7); v < ((KO & 1) ? 0 : V); v += 2) {  // wave-uniform view
            const SamplePos sp = sample_position<false>(p.M + ((size_t)v * p.B + b) * 12, fx, fy, depth, sx, sy, xhi, yhi);  // scalar loads
            const CellWeights cw = cell_weights(sp.ix, sp.iy);
            const int slot = (v * DPB + li) * PPB + lpx;
            lds_loc[slot] = cw.all();
            lds_off[slot] = (unsigned)(int)fmaf(cw.yf, W2f, cw.xf) * PIX;  // exact in fp32 (checked on the host)
        }
    }

    // ---- blend: 8 lanes per pixel, 4 channels per lane ---------------------------------------------------------
    const int q = tid & 7, px = tid >> 3;
    const int xc = min(x0 + px, w - 1);
    const unsigned org = rowb + PIX + (unsigned)q * 16;  // padded (1,1) + this lane's channel quad
    float4 s1[DPB], s2[DPB];
    {
        const float4 k = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.key) + (size_t)b * img_bytes + org +
                                                          (unsigned)y * rowb + (unsigned)xc * PIX);
        const float4 k2 = make_float4(k.x * k.x, k.y * k.y, k.z * k.z, k.w * k.w);
#pragma unroll
        for (int i = 0; i < DPB; ++i) { s1[i] = k; s2[i] = k2; }
    }
    __syncthreads();

    // the next view's cell offsets and source pointer are fetched (LDS / scalar cache) under the current view's gathers
    unsigned offn[DPB];
    const char* srcn;
    auto fetch_view = [&](int v) {
        const unsigned* __restrict__ ol = lds_off + v * (DPB * PPB) + px;
#pragma unroll
        for (int i = 0; i < DPB; ++i) offn[i] = ol[i * PPB];
        srcn = reinterpret_cast<const char*>(p.src.p[v]);
    };
    fetch_view(0);
    for (int v = 0; v < V; ++v) {
        unsigned off[DPB];
#pragma unroll
        for (int i = 0; i < DPB; ++i) off[i] = offn[i] + org;
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(srcn + (size_t)b * img_bytes), 0, (int)img_bytes, 0x00020000);
        const float4* __restrict__ wl = lds_loc + v * (DPB * PPB) + px;
        fetch_view(min(v + 1, V - 1));
        dispatch_mask(cell_change_mask(off), [&](auto mask) { gather_blend_4planes_lds<decltype(mask)::value, KO>(s1, s2, wl, off, rsrc, rowb); });
    }

    const float inv_nv = 1.0f / (float)(p.V + 1);  // mvsnet.py:135, V there counts the key view
    if (x0 + px < w) {
#pragma unroll
        for (int i = 0; i < DPB; ++i) {
            const int d = d0 + i;
            if (d >= D) break;  // block-uniform
            const float4 r = variance_finish(s1[i], s2[i], inv_nv);
            if ((KO & 4) && r.x != 123.456f) continue;
            *reinterpret_cast<float4*>(p.out + ((((size_t)b * D + d) * h + y) * w + (x0 + px)) * 32 + q * 4) = r;
        }
    }
}


// ------------------------------------------------------------------------------------------------
// Marching form of the located kernel.  Knock-out timings of warp_variance_located_kernel (profiles/r02_k3_located_ko.txt)
// show that nothing in it overlaps: 0.16 ms of per-workgroup prologue latency (kernel arguments -> depth -> locate ->
// barrier), 0.10 ms of blend arithmetic per view, +0.15 ms of exposed gather latency, +0.17 ms of exposed store
// acknowledgements add up linearly to the 0.82 ms.  Here a workgroup keeps its 32-pixel row segment and MARCHES through
// `nch` consecutive 4-plane chunks: index decode and key fetch once, chunk c+1 is located (into the other half of a
// double-buffered LDS table, depths through the scalar cache so that nothing queues behind the stores) before chunk c is
// blended, one barrier per chunk, and the stores of chunk c drain while chunk c+1 is located and its first gathers fly.
// NSETS = 2 keeps two cells in flight instead of three (96 VGPRs = 5 waves per SIMD).
constexpr int cell_of(int mask, int i) { return i == 0 ? 0 : cell_of(mask, i - 1) + ((mask >> (i - 1)) & 1); }
constexpr int ncells_of(int mask) { return cell_of(mask, 3) + 1; }
constexpr int first_plane_of_cell(int mask, int k) {
    for (int i = 0; i < 4; ++i)
        if (cell_of(mask, i) == k) return i;
    return 3;
}

template <int MASK, int K, int I, class TAP>
__device__ __forceinline__ void blend_if_cell(float4 (&s1)[4], float4 (&s2)[4], const float4 (&w)[4], const TAP (&X)[4],
                                              const TAP (&Y)[4]) {
    if constexpr (cell_of(MASK, I) == K) blend_plane_lds<MASK, I>(s1, s2, w[I], (K & 1) ? Y : X);
}

struct NoHook {
    __device__ __forceinline__ void operator()() const {}
};

// `after_last_gather` runs right behind the LAST gather request of the view (the parked stores of the previous chunk go there:
// every later wait of this view is for loads that are OLDER than those stores)
template <int MASK, int K, class TAP, class Hook = NoHook>
__device__ __forceinline__ void cell_step(float4 (&s1)[4], float4 (&s2)[4], const float4 (&w)[4], TAP (&X)[4], TAP (&Y)[4],
                                          const unsigned (&off)[4], __amdgpu_buffer_rsrc_t rsrc, unsigned rowb,
                                          const Hook& after_last_gather = Hook()) {
    if constexpr (K < ncells_of(MASK)) {
        blend_if_cell<MASK, K, 0>(s1, s2, w, X, Y);
        blend_if_cell<MASK, K, 1>(s1, s2, w, X, Y);
        blend_if_cell<MASK, K, 2>(s1, s2, w, X, Y);
        blend_if_cell<MASK, K, 3>(s1, s2, w, X, Y);
        if constexpr (K + 2 < ncells_of(MASK)) {  // the set this cell just released takes the cell after next
            __builtin_amdgcn_sched_barrier(0);    // (left alone, the scheduler hoists these loads above the blends and spills)
            gather_cell_s((K & 1) ? Y : X, rsrc, off[first_plane_of_cell(MASK, K + 2)], rowb);
            if constexpr (K + 2 == ncells_of(MASK) - 1) {
                after_last_gather();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

template <int MASK, class TAP = u32x4, class Hook = NoHook>
__device__ __forceinline__ void gather_blend_4planes_2sets(float4 (&s1)[4], float4 (&s2)[4], const float4* __restrict__ wl,
                                                           const unsigned (&off)[4], __amdgpu_buffer_rsrc_t rsrc, unsigned rowb,
                                                           const Hook& after_last_gather = Hook()) {
    TAP X[4], Y[4];
    gather_cell_s(X, rsrc, off[0], rowb);
    if constexpr (ncells_of(MASK) > 1) gather_cell_s(Y, rsrc, off[first_plane_of_cell(MASK, 1)], rowb);
    if constexpr (ncells_of(MASK) <= 2) {
        after_last_gather();
        __builtin_amdgcn_sched_barrier(0);
    }
    const float4 w[4] = {wl[0], wl[32], wl[64], wl[96]};
    cell_step<MASK, 0>(s1, s2, w, X, Y, off, rsrc, rowb, after_last_gather);
    cell_step<MASK, 1>(s1, s2, w, X, Y, off, rsrc, rowb, after_last_gather);
    cell_step<MASK, 2>(s1, s2, w, X, Y, off, rsrc, rowb, after_last_gather);
    cell_step<MASK, 3>(s1, s2, w, X, Y, off, rsrc, rowb, after_last_gather);
}

// Pipelined form: the first cell of this view (set X) was gathered while the PREVIOUS view was blended; the second cell (if
// the chunk has one) is requested first thing, then the chain of cell_steps runs as above.
template <int MASK, class TAP = u32x4>
__device__ __forceinline__ void blend_view_prefetched(float4 (&s1)[4], float4 (&s2)[4], const float4* __restrict__ wl, TAP (&X)[4],
                                                      TAP (&Y)[4], const unsigned (&off)[4], __amdgpu_buffer_rsrc_t rsrc,
                                                      unsigned rowb) {
    if constexpr (ncells_of(MASK) > 1) gather_cell_s(Y, rsrc, off[first_plane_of_cell(MASK, 1)], rowb);
    const float4 w[4] = {wl[0], wl[32], wl[64], wl[96]};
    cell_step<MASK, 0>(s1, s2, w, X, Y, off, rsrc, rowb);
    cell_step<MASK, 1>(s1, s2, w, X, Y, off, rsrc, rowb);
    cell_step<MASK, 2>(s1, s2, w, X, Y, off, rsrc, rowb);
    cell_step<MASK, 3>(s1, s2, w, X, Y, off, rsrc, rowb);
}

// F16: features are fp16 zero-bordered channel-last maps (64 B per pixel), the volume is written as fp16 (B,D,h,w,32);
// positions, weights, blend and variance stay fp32 (mvd_warp_variance_f16, BASELINE configs[3]).
// WP (wave-private locate): every wave locates the 128 (pixel, plane, view) combinations of ITS OWN 8 pixels (2 per lane;
// the two half-waves take even / odd views, so the transforms come from a small LDS table instead of the scalar cache) and
// is the only reader of those table entries: no workgroup barrier inside the march, the four waves drift apart freely.
// PIPE: views are software-pipelined.  A wave spends most of a (chunk, view) waiting for the view's first gather (vector ALU 46 %
// busy, texture addresser 74 %, four waves per SIMD: profiles/r02_k3_march_pmc.txt); here the first cell of view v+1 is
// requested before view v is blended, into a second pair of tap sets (64 tap VGPRs, three waves per SIMD).
// PARK (needs WP): a chunk's results are not stored at its end but parked in LDS (16 KB, wave-private) and stored from the
// middle of the NEXT chunk's first view, right behind that view's last gather request.  vmcnt retires loads and stores in one
// order: stores issued at the end of a chunk sit in front of the next chunk's first gathers, and the first blend then waits for
// their write acknowledgements (knock-out timings, profiles/r02_k3_march_ko.txt: no stores -0.10 ms, no gathers -0.12 ms,
// neither -0.25 ms of 0.72).
template <int MINW, int NSETS, bool F16 = false, bool WP = false, bool PIPE = false, bool PARK = false>
__global__ void __launch_bounds__(256, MINW) warp_variance_march_kernel(WarpParams p, int nch) {
    constexpr int DPB = 4, PPB = 32;
    constexpr unsigned PIX = F16 ? 64 : 128;  // bytes per pixel
    constexpr unsigned QB = F16 ? 8 : 16;     // bytes per lane (4 channels)
    extern __shared__ __attribute__((aligned(16))) float4 lds_raw[];  // 2 x ([V][4][32] float4 weights + [V][4][32] u32 offsets)
    const int V = p.V;
    const int half_q = V * (DPB * PPB) * 5 / 4;  // float4 slots per table half (weights + offsets)
    constexpr int NH = (WP && PARK) ? 1 : 2;     // table halves in the allocation (the wave-private locate uses one)

    const int tid = threadIdx.x;
    const int h = p.h, w = p.w, D = p.D;

    const int dchunks = (D + DPB - 1) / DPB;
    const BlockWork blk = decode_xcd_first(blockIdx.x, (dchunks + nch - 1) / nch, p.tiles_per_xcd);  // chunk groups
    const int dg = blk.chunk, b = blk.b, tile = blk.tile;
    if (tile >= p.tiles_x * h) return;  // block-uniform
    const int y = tile / p.tiles_x;
    const int x0 = (tile - y * p.tiles_x) * PPB;
    const int c_begin = dg * nch, c_end = min(c_begin + nch, dchunks);

    const int W2 = w + 3;
    const unsigned rowb = (unsigned)W2 * PIX;             // bytes per padded row
    const unsigned img_bytes = (unsigned)(h + 3) * rowb;  // bytes per padded image
    // constant address space: uniform reads of the depth samples and transforms become scalar-cache loads (lgkmcnt);
    // as ordinary global loads they would be vector-memory operations that retire in order BEHIND the previous chunk's
    // stores (profiles/r02_k3_march_pmc.txt: 17 vector loads per wave too many)
    typedef const float __attribute__((address_space(4))) cfloat;
    cfloat* dvals = (cfloat*)(p.depth + (size_t)b * D);

    // locate-phase constants: thread = (pixel lpx, plane li), views two at a time (wave-uniform)
    const int lpx = tid & 31, li = (tid >> 5) & 3;
    const float lfx = (float)min(x0 + lpx, w - 1), lfy = (float)y;
    const float sx = (float)w / (float)(w - 1), sy = (float)h / (float)(h - 1);
    const float xhi = (float)w, yhi = (float)h;
    const float W2f = (float)W2;
    const int v_first = __builtin_amdgcn_readfirstlane(tid >> 7);
    // wave-private form: lane = (pixel of this wave l&7, plane (l>>3)&3, view parity l>>5)
    float4* __restrict__ mtab = lds_raw + NH * half_q + 256;  // [V][3] float4: the composed transforms (WP only)
    if constexpr (WP) {
        if (tid < V * 3) {
            cfloat* Mg = (cfloat*)(p.M + ((size_t)(tid / 3) * p.B + b) * 12 + (tid % 3) * 4);
            mtab[tid] = make_float4(Mg[0], Mg[1], Mg[2], Mg[3]);
        }
    }
    auto locate_wp = [&](int c) {
        float4* __restrict__ loc = lds_raw;
        unsigned* __restrict__ offs = reinterpret_cast<unsigned*>(loc + V * (DPB * PPB));
        // lane-derived values are recomputed from an opaque copy of the thread index (a few integer ops per chunk) instead of
        // living in registers across the whole march: the kernel sits exactly at the 128-VGPR boundary of 4 waves per SIMD
        int t_ = tid;
        asm volatile("" : "+v"(t_));
        const int wpx = (t_ >> 6) * 8 + (t_ & 7), wpi = (t_ >> 3) & 3, wvp = (t_ >> 5) & 1;
        const float wfx = (float)min(x0 + wpx, w - 1);
        const int d0 = c * DPB;
        const float e0 = dvals[min(d0, D - 1)], e1 = dvals[min(d0 + 1, D - 1)], e2 = dvals[min(d0 + 2, D - 1)],
                    e3 = dvals[min(d0 + 3, D - 1)];
        const float depth = wpi == 0 ? e0 : wpi == 1 ? e1 : wpi == 2 ? e2 : e3;
        for (int v = wvp; v < V; v += 2) {
            const float4 m0 = mtab[v * 3], m1 = mtab[v * 3 + 1], m2 = mtab[v * 3 + 2];
            const float M[12] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w};
            const SamplePos sp = sample_position<false>(M, wfx, lfy, depth, sx, sy, xhi, yhi);
            const CellWeights cw = cell_weights(sp.ix, sp.iy);
            const int slot = (v * DPB + wpi) * PPB + wpx;
            loc[slot] = cw.all();
            offs[slot] = (unsigned)(int)fmaf(cw.yf, W2f, cw.xf) * PIX;
        }
    };
    auto locate = [&](int c, int buf) {
        float4* __restrict__ loc = lds_raw + buf * half_q;
        unsigned* __restrict__ offs = reinterpret_cast<unsigned*>(loc + V * (DPB * PPB));
        // the chunk's four depths are wave-uniform: scalar loads (lgkmcnt), so nothing here queues behind the
        // vector-memory stores of the previous chunk
        const int d0 = c * DPB;
        const float e0 = dvals[min(d0, D - 1)], e1 = dvals[min(d0 + 1, D - 1)], e2 = dvals[min(d0 + 2, D - 1)],
                    e3 = dvals[min(d0 + 3, D - 1)];
        const float depth = li == 0 ? e0 : li == 1 ? e1 : li == 2 ? e2 : e3;
        for (int v = v_first; v < V; v += 2) {
            cfloat* Mc = (cfloat*)(p.M + ((size_t)v * p.B + b) * 12);  // scalar loads
            const float M[12] = {Mc[0], Mc[1], Mc[2], Mc[3], Mc[4], Mc[5], Mc[6], Mc[7], Mc[8], Mc[9], Mc[10], Mc[11]};
            const SamplePos sp = sample_position<false>(M, lfx, lfy, depth, sx, sy, xhi, yhi);
            const CellWeights cw = cell_weights(sp.ix, sp.iy);
            const int slot = (v * DPB + li) * PPB + lpx;
            loc[slot] = cw.all();
            offs[slot] = (unsigned)(int)fmaf(cw.yf, W2f, cw.xf) * PIX;  // exact in fp32 (checked on the host)
        }
    };

    // blend-phase constants: 8 lanes per pixel, 4 channels per lane
    const int q = tid & 7, px = tid >> 3;
    const int xc = min(x0 + px, w - 1);
    const unsigned org = rowb + PIX + (unsigned)q * QB;  // padded (1,1) + this lane's channel quad
    // the key features of this thread's (pixel, channel quad) stay in LDS between chunks (4 fewer long-lived VGPRs)
    float4* __restrict__ key_slot = lds_raw + NH * half_q + tid;
    {
        const char* kp = reinterpret_cast<const char*>(p.key) + (size_t)b * img_bytes + org + (unsigned)y * rowb + (unsigned)xc * PIX;
        if constexpr (F16) {
            const u32x2 kh = *reinterpret_cast<const u32x2*>(kp);
            const f16x2 lo = as_h2(kh.x), hi = as_h2(kh.y);
            *key_slot = make_float4((float)lo.x, (float)lo.y, (float)hi.x, (float)hi.y);
        } else {
            *key_slot = *reinterpret_cast<const float4*>(kp);
        }
    }
    const float inv_nv = 1.0f / (float)(V + 1);  // mvsnet.py:135, V there counts the key view
    // stores: one descriptor per output plane (scalar arithmetic), one 32-bit offset per lane.  Inactive lanes (ragged
    // right edge) carry pixel w-1 like the last active lane and store the same values to the same address: no divergent
    // branch around the stores
    const unsigned out_off = ((unsigned)y * (unsigned)w + (unsigned)xc) * PIX + (unsigned)q * QB;
    const size_t plane_bytes = (size_t)h * w * PIX;
    // PARK: [4 planes][256 lanes] float4 behind the transforms; each lane reads back what it wrote
    float4* __restrict__ park_base = lds_raw + NH * half_q + 256 + ((V * 3 + 3) & ~3);
    int parked_d0 = -1;  // first plane of the chunk whose results are parked (wave-uniform)
    auto drain = [&]() {
        if (parked_d0 < 0) return;
        // the kernel sits exactly at 128 VGPRs: lane-derived addresses are recomputed from an opaque copy of the thread index
        // and the planes leave one at a time (4 VGPRs in flight)
        int t_ = tid;
        asm volatile("" : "+v"(t_));
        const unsigned oo = ((unsigned)y * (unsigned)w + (unsigned)min(x0 + (t_ >> 3), w - 1)) * PIX + (unsigned)(t_ & 7) * QB;
        const float4* __restrict__ pk = park_base + t_;
#pragma unroll
        for (int i = 0; i < DPB; ++i) {
            const float4 r = pk[i * 256];
            const int d = min(parked_d0 + i, D - 1);
            const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
                reinterpret_cast<char*>(p.out) + ((size_t)b * D + d) * plane_bytes, 0, parked_d0 + i < D ? (int)plane_bytes : 0, 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(r.x), __float_as_uint(r.y), __float_as_uint(r.z),
                                                         __float_as_uint(r.w)}, orsrc, oo, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    if constexpr (WP) __syncthreads();  // transforms and key slots are staged; no further workgroup barrier
    else locate(c_begin, 0);
    int buf = 0;
    for (int c = c_begin; c < c_end; ++c, buf ^= (WP ? 0 : 1)) {
        if constexpr (WP) {
            locate_wp(c);  // this wave's own table entries (same-wave LDS accesses execute in order)
        } else {
            __syncthreads();  // table `buf` is complete; every wave is done reading table `buf ^ 1`
            if (c + 1 < c_end) locate(c + 1, buf ^ 1);
        }
        const float4* __restrict__ loc = lds_raw + buf * half_q;
        const unsigned* __restrict__ offs = reinterpret_cast<const unsigned*>(loc + V * (DPB * PPB));
        float4 s1[DPB], s2[DPB];
        {
            const float4 k = *key_slot;
            const float4 k2 = make_float4(k.x * k.x, k.y * k.y, k.z * k.z, k.w * k.w);
#pragma unroll
            for (int i = 0; i < DPB; ++i) { s1[i] = k; s2[i] = k2; }
        }
        if constexpr (PIPE) {
            using TAP = typename std::conditional<F16, u32x2, u32x4>::type;
            TAP X0[4], Y0[4], X1[4], Y1[4];
            unsigned offa[DPB], offb[DPB], ma = 0, mb = 0;
            __amdgpu_buffer_rsrc_t ra, rb;
            // offsets + re-gather pattern of view v (wave-uniform mask), its descriptor, and the request for its first cell
            auto open_view = [&](int v, unsigned (&off)[DPB], unsigned& mask, TAP (&X)[4]) {
                const unsigned* __restrict__ ol = offs + v * (DPB * PPB) + px;
#pragma unroll
                for (int i = 0; i < DPB; ++i) off[i] = ol[i * PPB] + org;
                mask = cell_change_mask(off);
                const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<char*>(reinterpret_cast<const char*>(p.src.p[v]) + (size_t)b * img_bytes), 0, (int)img_bytes, 0x00020000);
                gather_cell_s(X, r, off[0], rowb);
                return r;
            };
            auto blend_view = [&](unsigned mask, TAP (&X)[4], TAP (&Y)[4], const unsigned (&off)[DPB], __amdgpu_buffer_rsrc_t rs, int v) {
                dispatch_mask(mask, [&](auto m) { blend_view_prefetched<decltype(m)::value, TAP>(s1, s2, loc + v * (DPB * PPB) + px, X, Y, off, rs, rowb); });
            };
            // Every path between a request and the first use of its taps is straight-line code: behind a conditional request
            // the compiler must assume the smaller number of outstanding loads and would wait for the prefetch it just issued.
            ra = open_view(0, offa, ma, X0);
            for (int v = 0; v + 1 < V; v += 2) {
                rb = open_view(v + 1, offb, mb, X1);
                blend_view(ma, X0, Y0, offa, ra, v);
                if (v + 2 < V) {
                    ra = open_view(v + 2, offa, ma, X0);
                    blend_view(mb, X1, Y1, offb, rb, v + 1);
                } else {
                    blend_view(mb, X1, Y1, offb, rb, v + 1);
                }
            }
            if (V & 1) blend_view(ma, X0, Y0, offa, ra, V - 1);  // the last view of an odd count was opened by the iteration before it (or above, V = 1)
        } else {
            unsigned offn[DPB];
            const char* srcn;
            auto fetch_view = [&](int v) {
                const unsigned* __restrict__ ol = offs + v * (DPB * PPB) + px;
    #pragma unroll
                for (int i = 0; i < DPB; ++i) offn[i] = ol[i * PPB];
                srcn = reinterpret_cast<const char*>(p.src.p[v]);
            };
            fetch_view(0);
            for (int v = 0; v < V; ++v) {
                unsigned off[DPB];
    #pragma unroll
                for (int i = 0; i < DPB; ++i) off[i] = offn[i] + org;
                const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<char*>(srcn + (size_t)b * img_bytes), 0, (int)img_bytes, 0x00020000);
                const float4* __restrict__ wl = loc + v * (DPB * PPB) + px;
                fetch_view(min(v + 1, V - 1));
                // PARK: the previous chunk's parked results leave behind the first view's last gather request
                const bool first = v == 0;  // wave-uniform
                auto drain_v0 = [&]() { if (first) drain(); };
                dispatch_mask(cell_change_mask(off), [&](auto m) {
                    constexpr int Mk = decltype(m)::value;
                    if constexpr (PARK) gather_blend_4planes_2sets<Mk, u32x4>(s1, s2, wl, off, rsrc, rowb, drain_v0);
                    else if constexpr (F16) gather_blend_4planes_2sets<Mk, u32x2>(s1, s2, wl, off, rsrc, rowb);
                    else if constexpr (NSETS == 2) gather_blend_4planes_2sets<Mk, u32x4>(s1, s2, wl, off, rsrc, rowb);
                    else gather_blend_4planes_lds<Mk>(s1, s2, wl, off, rsrc, rowb);
                });
            }
        }
        const int d0 = c * DPB;
#pragma unroll
        for (int i = 0; i < DPB; ++i) {
            if (d0 + i >= D) break;  // block-uniform (only in the last chunk of a D that is not a multiple of 4)
            const float4 r = variance_finish(s1[i], s2[i], inv_nv);
            if constexpr (PARK) {
                park_base[i * 256 + tid] = r;
                continue;
            }
            const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
                reinterpret_cast<char*>(p.out) + ((size_t)b * D + d0 + i) * plane_bytes, 0, (int)plane_bytes, 0x00020000);
            if constexpr (F16) {  // round to nearest even, one rounding
                const f16x2 lo = {(_Float16)r.x, (_Float16)r.y}, hi = {(_Float16)r.z, (_Float16)r.w};
                store_b64(u32x2{as_u32(lo), as_u32(hi)}, orsrc, out_off);
            } else {
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(r.x), __float_as_uint(r.y), __float_as_uint(r.z),
                                                             __float_as_uint(r.w)}, orsrc, out_off, 0, 0);
            }
        }
        if constexpr (PARK) parked_d0 = d0;
    }
    if constexpr (PARK) drain();
}

// LDS of the marching kernel grows with V (the tile kernel's does not): up to 64 KiB (V <= 12) it launches without an attribute
// and keeps at least two workgroups per CU
static size_t march_lds_bytes(int V) {
    return 2 * (size_t)V * 4 * 32 * (sizeof(float4) + sizeof(unsigned)) + 256 * sizeof(float4) + (size_t)V * 3 * sizeof(float4);
}

static int launch_warp_march(const WarpParams& p0, hipStream_t st, int minw, int nsets, int nch, bool f16 = false) {
    WarpParams p = p0;
    p.tiles_x = (p.w + 31) / 32;
    const long long tiles = (long long)p.tiles_x * p.h;
    p.tiles_per_xcd = (int)((tiles + 7) / 8);
    const int dchunks = (p.D + 3) / 4;
    if (nch < 1) nch = 1;
    if ((long long)p.h * p.w * (f16 ? 64 : 128) >= 0x7fffffffLL) {  // one output plane is addressed through a 32-bit buffer offset
        set_error("warp_variance: an output plane of %dx%dx32 floats exceeds the 2 GiB buffer-offset range", p.h, p.w);
        return MVD_ERR_INVALID_ARG;
    }
    const int dgroups = (dchunks + nch - 1) / nch;
    const long long nblk = 8LL * p.tiles_per_xcd * dgroups * p.B;
    if (nblk > 0x7fffffffLL) {
        set_error("warp_variance: %lld workgroups exceed the grid limit", nblk);
        return MVD_ERR_INVALID_ARG;
    }
    const size_t lds = march_lds_bytes(p.V);  // 5 KiB per view + key slots + transforms (V <= 12 keeps it within 64 KiB)
    const dim3 grid((unsigned)nblk);
    timing_begin(st);
#define MVD_M(MW, NS) hipLaunchKernelGGL((warp_variance_march_kernel<MW, NS>), grid, dim3(256), lds, st, p, nch)
    if (f16) {
        hipLaunchKernelGGL((warp_variance_march_kernel<4, 2, true>), grid, dim3(256), lds, st, p, nch);
        timing_end(st);
        return launch_status("warp_variance_march_f16");
    }
    switch (minw * 10 + nsets) {
        case 43: MVD_M(4, 3); break;
        case 52: MVD_M(5, 2); break;
        case 62: MVD_M(6, 2); break;
        case 72: hipLaunchKernelGGL((warp_variance_march_kernel<4, 2, false, true>), grid, dim3(256), lds, st, p, nch); break;  // "M7,2,n": wave-private locate
        case 82: hipLaunchKernelGGL((warp_variance_march_kernel<3, 2, false, false, true>), grid, dim3(256), lds, st, p, nch); break;  // "M8,2,n": views pipelined
        case 92: hipLaunchKernelGGL((warp_variance_march_kernel<4, 2, false, false, true>), grid, dim3(256), lds, st, p, nch); break;  // "M9,2,n": views pipelined, 128 VGPRs
        case 102: hipLaunchKernelGGL((warp_variance_march_kernel<4, 2, false, true, false, true>), grid, dim3(256), lds + 4 * 256 * sizeof(float4) + 64, st, p, nch); break;  // "M10,2,n": wave-private locate + parked stores
        case 112: hipLaunchKernelGGL((warp_variance_march_kernel<3, 2, false, true, false, true>), grid, dim3(256), lds + 4 * 256 * sizeof(float4) + 64, st, p, nch); break;  // "M11,2,n": the same at three waves per SIMD
        default: MVD_M(4, 2); break;
    }
#undef MVD_M
    timing_end(st);
    return launch_status("warp_variance_march");
}

static int launch_warp_located(const WarpParams& p0, hipStream_t st, int minw, int ko = 0) {
    WarpParams p = p0;
    p.tiles_x = (p.w + 31) / 32;
    const long long tiles = (long long)p.tiles_x * p.h;
    p.tiles_per_xcd = (int)((tiles + 7) / 8);
    const long long nblk = 8LL * p.tiles_per_xcd * ((p.D + 3) / 4) * p.B;
    if (nblk > 0x7fffffffLL) {
        set_error("warp_variance: %lld workgroups exceed the grid limit", nblk);
        return MVD_ERR_INVALID_ARG;
    }
    const size_t lds = (size_t)p.V * 4 * 32 * (sizeof(float4) + sizeof(unsigned));  // 2.5 KiB per view
    const dim3 grid((unsigned)nblk);
    timing_begin(st);
    switch (ko) {
#define MVD_KO(K) case K: hipLaunchKernelGGL((warp_variance_located_kernel<4, K>), grid, dim3(256), lds, st, p); break;
        MVD_KO(1) MVD_KO(2) MVD_KO(4) MVD_KO(6) MVD_KO(7) MVD_KO(8) MVD_KO(14) MVD_KO(15)
#undef MVD_KO
        case 0:
            if (minw == 3) hipLaunchKernelGGL(warp_variance_located_kernel<3>, grid, dim3(256), lds, st, p);
            else hipLaunchKernelGGL(warp_variance_located_kernel<4>, grid, dim3(256), lds, st, p);
            break;
        default:
            timing_end(st);
            set_error("warp_variance: MVD_K3_CFG L%d,%d is not a compiled variant", minw, ko);
            return MVD_ERR_INVALID_ARG;
    }
    timing_end(st);
    return launch_status("warp_variance_located");
}

// ------------------------------------------------------------------------------------------------
// MVD_K3_CFG, the experiments library's K3 selector.  Set (even to ""), it turns the tile kernel off for fp32 calls unless it
// names it:
//   "T<tw>,<win>,<nch>,<sets>"           the tile kernel in another form (C = 32 channel-last; fp32 and fp16)
//   "L3", "L4", "L4,<ko>"                 the located kernel, 3 / 4 waves per SIMD, <ko> a knock-out build (V <= 25)
//   "M<minw>,<nsets>,<nch>"               the marching kernel (fp16: any "M…" runs its one fp16 form)
//   "lds,<nd>", "wave,<nd>", "q8,<minw>"  the forms at the top of this file
//   "<dpb>,<minw>", "r…", "u…", "v…"      the gather kernel in another form (C = 32 on the folded grid: GatherForm)
// L, M, lds, wave and q8 apply to fp32 C = 32 channel-last volumes on the folded grid.  Every call no part of the selector
// applies to runs the gather kernel's product form (fp16: the product's tile kernel).
int warp_variance_experiment(const char* e, const WarpParams& p, int C, bool warp_only, bool f16, hipStream_t st,
                             const GatherForm* forms, int nforms) {
    const bool exact = p.exact_grid != 0;  // (never for fp16)
    const bool c32_ndhwc = f16 || (!warp_only && C == 32 && p.layout == MVD_LAYOUT_NDHWC);
    if (c32_ndhwc && e[0] == 'T') {
        int tw = 8, win = f16 ? 128 : 104, nch = f16 ? 16 : 8, sets = f16 ? 2 : 1;
        sscanf(e, "T%d,%d,%d,%d", &tw, &win, &nch, &sets);
        return launch_warp_tile(p, st, tw, win, nch, sets, f16, exact);
    }
    if (f16) return e[0] == 'M' ? launch_warp_march(p, st, 4, 2, 4, true) : launch_warp_tile(p, st, 8, 128, 8, 1, true, false);
    if (c32_ndhwc && !exact) {
        if (e[0] == 'L' && (size_t)p.V * 4 * 32 * 20 <= 64 * 1024) {  // 2.5 KiB of LDS per view
            int minw = 4, ko = 0;
            sscanf(e, "L%d,%d", &minw, &ko);
            return launch_warp_located(p, st, minw, ko);
        }
        if (e[0] == 'M') { int mw = 5, ns = 2, nc = 4; sscanf(e, "M%d,%d,%d", &mw, &ns, &nc); return launch_warp_march(p, st, mw, ns, nc); }
        if (e[0] == 'l') { int nd = 4; sscanf(e, "lds,%d", &nd); return launch_warp_lds(p, st, nd); }
        if (e[0] == 'q') { int mw = 4; sscanf(e, "q8,%d", &mw); return launch_warp_q8(p, st, mw); }
        if (e[0] == 'w') { int nd = 8; sscanf(e, "wave,%d", &nd); return launch_warp_wave(p, st, nd); }
    }
    if (C != 32 || exact) return launch_warp_gather(p, C, warp_only, st);
    // (planes per workgroup, min waves per SIMD, Reuse); a selector of another kind keeps the product's (4, 3, wave_uniform)
    int dpb = 4, minw = 3;
    Reuse reuse = Reuse::wave_uniform;
    if (e[0] >= '0' && e[0] <= '9') { sscanf(e, "%d,%d", &dpb, &minw); reuse = Reuse::none; }
    if (e[0] == 'r') { sscanf(e, "r%d,%d", &dpb, &minw); reuse = Reuse::per_lane; }
    if (e[0] == 'u') { sscanf(e, "u%d,%d", &dpb, &minw); reuse = Reuse::wave_uniform; }
    if (e[0] == 'v') { sscanf(e, "v%d,%d", &dpb, &minw); reuse = Reuse::wave_uniform_late; }
    for (int i = 0; i < nforms; ++i)
        if (forms[i].reuse == reuse && forms[i].dpb == dpb && forms[i].minw == minw) return launch_gather(p, 8, dpb, forms[i].kernel, st);
    set_error("warp_variance: MVD_K3_CFG=%s is not a compiled variant", e);
    return MVD_ERR_INVALID_ARG;
}

}  // namespace mvd
