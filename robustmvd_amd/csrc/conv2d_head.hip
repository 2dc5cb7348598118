// FeatureNet's two full-resolution layers in one pass (rmvd/models/blocks/mvsnet_components.py:47-48:
// ConvBnReLU(3, 8, 3, 1, 1) -> ConvBnReLU(8, 8, 3, 1, 1)) — HBM-bound: 3 input and 8 output channels per pixel, 1.6 kFLOP between.
// As two launches the 8-channel intermediate (141 MB at 5 x 768 x 1152) is written and read once each and both layers sit at
// about half the streaming rate; here a workgroup keeps the intermediate of its 8 x 64-pixel tile (+ one halo ring) in LDS:
//   1. the 3-channel image patch (12 x 68) -> LDS, zeros outside the image;
//   2. conv0 + folded BN + ReLU on the 10 x 66 pixels the tile's conv1 needs, one pixel per lane -> LDS as two float4 planes
//      (positions outside the image are conv1's zero padding, NOT conv0 of padding);
//   3. conv1 + folded BN + ReLU, two pixels per lane four rows apart (lanes = consecutive columns: conflict-free b128 reads),
//      channel-last float4 stores.
// fp32 on the vector ALU, every product one lane of a v_pk_fma_f32 (pixel value broadcast x a pair of output channels' weights);
// the 216 + 576 weights (packed [ky][kx][cin][cout] by the caller) arrive through the scalar cache as SGPR operands, one tap's 24 / 64
// per iteration of a runtime tap loop (unrolled, the compiler issues every load up front: 900 spilled SGPRs; as broadcast LDS
// reads they made the kernel LDS-bound: 16 weight reads per 64 packed FMAs, the LDS shared by four SIMDs — 158 us).
#include "mvd_common.h"
#include "split_operand.h"

namespace mvd {

typedef float hd2 __attribute__((ext_vector_type(2)));
typedef float hd4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) hd4* hd_c4;  // constant address space: uniform loads go through the scalar cache

constexpr int HD_TH = 8, HD_TW = 64;

struct HeadParams {
    const float* img;  // (B,3,H,W)
    const float* w0;   // [3][3][3][8]  ky, kx, cin, cout
    const float* s0;   // 8
    const float* b0;   // 8
    const float* w1;   // [3][3][8][8]
    const float* s1;
    const float* b1;
    float* y;          // (B,H,W,8)
    float* tile_max;   // optional: one float per workgroup, max |y| over the finite outputs of its tile
    int B, H, W, tiles_x, tiles_y;
};

__global__ void __launch_bounds__(256) conv2d_head_kernel(HeadParams p) {
    constexpr int IR = HD_TH + 4, IC = HD_TW + 4;  // image patch
    constexpr int MR = HD_TH + 2, MC = HD_TW + 2;  // conv0 outputs the tile's conv1 reads
    __shared__ float img[3][IR][IC];
    __shared__ __attribute__((aligned(16))) hd4 mid[2][MR][MC];  // channels 0-3 / 4-7

    const int tid = threadIdx.x;
    int bx = blockIdx.x;
    const int tx = bx % p.tiles_x; bx /= p.tiles_x;
    const int ty = bx % p.tiles_y;
    const int b = bx / p.tiles_y;
    const int r0 = ty * HD_TH, c0 = tx * HD_TW;
    const int H = p.H, W = p.W;

    // ---- 1: image patch ----
    const float* __restrict__ im = p.img + (size_t)b * 3 * H * W;
    for (int e = tid; e < 3 * IR * IC; e += 256) {
        const int ch = e / (IR * IC), rem = e - ch * (IR * IC);
        const int r = rem / IC, c = rem - r * IC;
        const int gr = r0 - 2 + r, gc = c0 - 2 + c;
        const bool in = gr >= 0 && gr < H && gc >= 0 && gc < W;
        (&img[0][0][0])[e] = in ? im[((size_t)ch * H + gr) * W + gc] : 0.0f;
    }
    __syncthreads();

    // ---- 2: conv0 on the tile + halo ----
    for (int e = tid; e < MR * MC; e += 256) {
        const int mr = e / MC, mc = e - mr * MC;
        hd2 acc[4] = {hd2{0.f, 0.f}, hd2{0.f, 0.f}, hd2{0.f, 0.f}, hd2{0.f, 0.f}};
#pragma unroll 1  // a runtime loop over the taps (see the header)
        for (int t = 0; t < 9; ++t) {
            const int ky = t / 3, kx = t - 3 * ky;
            const hd_c4 wt = (hd_c4)(unsigned long long)(p.w0 + t * 24);  // the tap's 24 weights: scalar loads, SGPR operands
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const float x = img[ci][mr + ky][mc + kx];
                const hd4 wa = wt[ci * 2], wb = wt[ci * 2 + 1];
                const hd2 xx = {x, x};
                acc[0] = __builtin_elementwise_fma(xx, wa.xy, acc[0]);
                acc[1] = __builtin_elementwise_fma(xx, wa.zw, acc[1]);
                acc[2] = __builtin_elementwise_fma(xx, wb.xy, acc[2]);
                acc[3] = __builtin_elementwise_fma(xx, wb.zw, acc[3]);
            }
        }
        const int gr = r0 - 1 + mr, gc = c0 - 1 + mc;
        const bool in = gr >= 0 && gr < H && gc >= 0 && gc < W;
        const hd_c4 sp = (hd_c4)(unsigned long long)p.s0, bp = (hd_c4)(unsigned long long)p.b0;
        const hd4 sa = sp[0], sb = sp[1], ba = bp[0], bb = bp[1];
        hd4 va = {fmaf(acc[0].x, sa.x, ba.x), fmaf(acc[0].y, sa.y, ba.y), fmaf(acc[1].x, sa.z, ba.z), fmaf(acc[1].y, sa.w, ba.w)};
        hd4 vb = {fmaf(acc[2].x, sb.x, bb.x), fmaf(acc[2].y, sb.y, bb.y), fmaf(acc[3].x, sb.z, bb.z), fmaf(acc[3].y, sb.w, bb.w)};
        const hd4 zero = {0.f, 0.f, 0.f, 0.f};
        va = in ? __builtin_elementwise_max(va, zero) : zero;
        vb = in ? __builtin_elementwise_max(vb, zero) : zero;
        mid[0][mr][mc] = va;
        mid[1][mr][mc] = vb;
    }
    __syncthreads();

    // ---- 3: conv1, pixels (row, col) and (row + 4, col) ----
    const int row = tid >> 6, col = tid & 63;
    hd2 accA[4] = {hd2{0.f, 0.f}, hd2{0.f, 0.f}, hd2{0.f, 0.f}, hd2{0.f, 0.f}};
    hd2 accB[4] = {hd2{0.f, 0.f}, hd2{0.f, 0.f}, hd2{0.f, 0.f}, hd2{0.f, 0.f}};
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
        const int ky = t / 3, kx = t - 3 * ky;
        const hd4 xa0 = mid[0][row + ky][col + kx], xa1 = mid[1][row + ky][col + kx];
        const hd4 xb0 = mid[0][row + 4 + ky][col + kx], xb1 = mid[1][row + 4 + ky][col + kx];
        const hd_c4 wt = (hd_c4)(unsigned long long)(p.w1 + t * 64);  // the tap's 64 weights: scalar loads, SGPR operands
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) {
            const float xa = ci < 4 ? xa0[ci & 3] : xa1[ci & 3];
            const float xb = ci < 4 ? xb0[ci & 3] : xb1[ci & 3];
            const hd4 wa = wt[ci * 2], wb = wt[ci * 2 + 1];
            const hd2 xxa = {xa, xa}, xxb = {xb, xb};
            accA[0] = __builtin_elementwise_fma(xxa, wa.xy, accA[0]);
            accA[1] = __builtin_elementwise_fma(xxa, wa.zw, accA[1]);
            accA[2] = __builtin_elementwise_fma(xxa, wb.xy, accA[2]);
            accA[3] = __builtin_elementwise_fma(xxa, wb.zw, accA[3]);
            accB[0] = __builtin_elementwise_fma(xxb, wa.xy, accB[0]);
            accB[1] = __builtin_elementwise_fma(xxb, wa.zw, accB[1]);
            accB[2] = __builtin_elementwise_fma(xxb, wb.xy, accB[2]);
            accB[3] = __builtin_elementwise_fma(xxb, wb.zw, accB[3]);
        }
    }
    const hd_c4 sp = (hd_c4)(unsigned long long)p.s1, bp = (hd_c4)(unsigned long long)p.b1;
    const hd4 sa = sp[0], sb = sp[1], ba = bp[0], bb = bp[1];
    const hd4 zero = {0.f, 0.f, 0.f, 0.f};
    const int gc = c0 + col;
    float m = 0.0f;
    auto store = [&](const hd2 (&a)[4], int gr) {
        if (gr >= H || gc >= W) return;
        hd4 va = {fmaf(a[0].x, sa.x, ba.x), fmaf(a[0].y, sa.y, ba.y), fmaf(a[1].x, sa.z, ba.z), fmaf(a[1].y, sa.w, ba.w)};
        hd4 vb = {fmaf(a[2].x, sb.x, bb.x), fmaf(a[2].y, sb.y, bb.y), fmaf(a[3].x, sb.z, bb.z), fmaf(a[3].y, sb.w, bb.w)};
        va = __builtin_elementwise_max(va, zero);
        vb = __builtin_elementwise_max(vb, zero);
        hd4* o = reinterpret_cast<hd4*>(p.y + (((size_t)b * H + gr) * W + gc) * 8);
        o[0] = va;
        o[1] = vb;
#pragma unroll
        for (int k = 0; k < 4; ++k) m = fmaxf(m, fmaxf(finite_abs_or_zero(va[k]), finite_abs_or_zero(vb[k])));
    };
    store(accA, r0 + row);
    store(accB, r0 + row + 4);
    if (p.tile_max) {  // per-tile maxima with plain stores (a second tiny pass reduces them): no atomics on one address
        __shared__ float wmax[4];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if ((tid & 63) == 0) wmax[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) p.tile_max[blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    }
}

// ---- the same pair of layers with conv1 on the matrix pipe (the default of FeatureNet's split layers) ---------------------
// conv1 (8 -> 8, 3x3) is 576 of the fp32 kernel's 856 packed FMAs per wave.  Here phase 2 leaves conv0's outputs in LDS as the two
// fp16 terms of split_operand.h (the same 32 bytes per pixel), scaled by a power of two from max |conv0| over the finite values of
// the workgroup's own 10 x 66 patch, and conv1 is 6 v_mfma_f32_16x16x32_f16 per 16 pixels of a row:
//   B = activations: column n = pixel c + n of the row, K = 32 = the 8 channels of the pixels c + n + kx, kx = 0..2, and a pad
//       slot that every lane reads from ONE always-zero pixel (a neighbour's inf or NaN must not meet the pad's zero weights);
//   A = weights: rows [w_hi of the 8 output channels | w_lo of the 8], K as above, one fragment per ky, each channel divided by its
//       2^k_c (pack_head_split_kernel, once per model);
//   one K step per ky, once with a_hi and once with a_lo: w_hi a_hi in rows 0..7 and w_lo a_hi in rows 8..15 of the first
//   accumulator, w_hi a_lo in rows 0..7 of the second.  A lane holds 4 consecutive rows of one pixel, so the lanes 0..31 fetch
//   w_lo a_hi from lane + 32, add the terms, multiply by 2^e 2^k_c, apply BN and ReLU and store their pixel's channels 4 (l / 16) ..
//   + 3 as one float4.  (conv0_split_kernel has the operands the other way round and stores single floats.)
// A wave owns two output rows of the tile: a fragment read (input row) feeds both.
typedef _Float16 hdh8 __attribute__((ext_vector_type(8)));
typedef unsigned int hdu4 __attribute__((ext_vector_type(4)));

constexpr float HD_LO_FACTOR = 2048.0f;    // the lo terms of both operands are stored times 2^11 (split_operand.h)
constexpr int HD_WPK_BYTES = 3 * 64 * 16;  // the three weight fragments; the 8 floats 2^k_c follow

struct HeadSplitParams {
    const float* img;  // (B,3,H,W)
    const float* w0;   // [3][3][3][8]  ky, kx, cin, cout
    const float* s0;
    const float* b0;
    const char* w1pk;  // pack_head_split_kernel's fragments + 2^k_c
    const float* s1;
    const float* b1;
    float* y;          // (B,H,W,8)
    float* tile_max;   // optional: one float per workgroup, max |y| over the finite outputs of its tile
    int B, H, W, tiles_x, tiles_y;
};

// w (8, 8, 3, 3) = conv1's Conv2d weight, wscale = its channels' 2^k_c -> [ky][lane 64][8 halves]: lane l = row l % 16 (0..7: w_hi
// of cout l % 16, 8..15: w_lo of cout l % 16 - 8), K values 8 (l / 16) .. + 7 = (kx = l / 16, cin); kx = 3 is the zero pad
__global__ void pack_head_split_kernel(const float* __restrict__ w, const float* __restrict__ wscale, _Float16* __restrict__ packed) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * 64 * 8) return;
    const int j = e & 7, lane = (e >> 3) & 63, ky = e >> 9;
    const int row = lane & 15, kx = lane >> 4, cout = row & 7;
    const float v = kx < 3 ? w[((cout * 8 + j) * 3 + ky) * 3 + kx] / wscale[cout] : 0.0f;
    _Float16 hi, lo;
    split_weight(v, HD_LO_FACTOR, hi, lo);
    packed[e] = row < 8 ? hi : lo;
}

// max over the finite values of v >= 0 (after ReLU: never negative, never NaN; +inf is the one value to skip), kept as the
// bits of the maximum + 2^23: +inf wraps to a negative integer and loses every signed comparison.  finite_abs_or_zero's result
// for such v at two instructions per value instead of three; finite_max_value() undoes the offset.
constexpr int HD_FMAX_ZERO = 0x00800000;
__device__ __forceinline__ int finite_max_nonneg(int m, float v) {
    return max(m, (int)(__float_as_uint(v) + (unsigned)HD_FMAX_ZERO));  // the wrap is meant: unsigned arithmetic
}
__device__ __forceinline__ float finite_max_value(int m) { return __uint_as_float((unsigned)(m - HD_FMAX_ZERO)); }

__global__ void __launch_bounds__(256) conv2d_head_split_kernel(HeadSplitParams p) {
    constexpr int IR = HD_TH + 4, IC = HD_TW + 4;  // image patch
    constexpr int MR = HD_TH + 2, MC = HD_TW + 2;  // conv0 outputs the tile's conv1 reads
    constexpr int NPX = MR * MC, NK = (NPX + 255) / 256;
    __shared__ float img[3 * IR * IC];
    __shared__ __attribute__((aligned(16))) hdu4 mid[2 * NPX + 2];  // per pixel (hi terms, lo terms): 32 bytes; the zero pixel last
    __shared__ float wmax[8];

    const int tid = threadIdx.x;
    int bx = blockIdx.x;
    const int tx = bx % p.tiles_x; bx /= p.tiles_x;
    const int ty = bx % p.tiles_y;
    const int b = bx / p.tiles_y;
    const int r0 = ty * HD_TH, c0 = tx * HD_TW;
    const int H = p.H, W = p.W;

    // ---- 1: image patch: 36 (channel, row) lines of 68 floats.  Wave w takes lines w, w + 4, ..: lane l column l (the line's
    // row tests are scalar, nine loads in flight); columns 64 .. 67 of all lines are one more load of 144 threads ----
    const float* __restrict__ im = p.img + (size_t)b * 3 * H * W;
    {
        const int lane = tid & 63, wvu = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int gca = c0 - 2 + lane;
        const bool ca = gca >= 0 && gca < W;
#pragma unroll
        for (int i = 0; i < 3 * IR / 4; ++i) {
            const int ln = wvu + 4 * i, ch = ln / IR, gr = r0 - 2 + (ln - ch * IR);
            img[ln * IC + lane] = (ca && gr >= 0 && gr < H) ? im[((size_t)ch * H + gr) * W + gca] : 0.0f;
        }
        if (tid < 3 * IR * 4) {
            const int ln = tid >> 2, c = 64 + (tid & 3), ch = ln / IR, gr = r0 - 2 + (ln - ch * IR), gc = c0 - 2 + c;
            img[ln * IC + c] = (gr >= 0 && gr < H && gc < W) ? im[((size_t)ch * H + gr) * W + gc] : 0.0f;
        }
    }
    if (tid < 2) mid[2 * NPX + tid] = hdu4{0u, 0u, 0u, 0u};
    __syncthreads();

    // ---- 2: conv0 on the tile + halo: the fp32 kernel's chains, a thread's (up to) three pixels side by side ----
    int ioff[NK];
    bool in[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int e = min(tid + 256 * k, NPX - 1);
        const int mr = e / MC, mc = e - mr * MC;
        const int gr = r0 - 1 + mr, gc = c0 - 1 + mc;
        ioff[k] = mr * IC + mc;
        in[k] = gr >= 0 && gr < H && gc >= 0 && gc < W;
    }
    hd2 acc[NK][4];
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[k][q] = hd2{0.f, 0.f};
#pragma unroll 1  // a runtime loop over the taps: one tap's 24 weights in SGPRs at a time
    for (int t = 0; t < 9; ++t) {
        const int ky = t / 3, kx = t - 3 * ky;
        const hd_c4 wt = (hd_c4)(unsigned long long)(p.w0 + t * 24);
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
            const hd4 wa = wt[ci * 2], wb = wt[ci * 2 + 1];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const float x = img[ci * IR * IC + ioff[k] + ky * IC + kx];
                const hd2 xx = {x, x};
                acc[k][0] = __builtin_elementwise_fma(xx, wa.xy, acc[k][0]);
                acc[k][1] = __builtin_elementwise_fma(xx, wa.zw, acc[k][1]);
                acc[k][2] = __builtin_elementwise_fma(xx, wb.xy, acc[k][2]);
                acc[k][3] = __builtin_elementwise_fma(xx, wb.zw, acc[k][3]);
            }
        }
    }
    int mb = HD_FMAX_ZERO;
    {
        const hd_c4 sp = (hd_c4)(unsigned long long)p.s0, bp = (hd_c4)(unsigned long long)p.b0;
        const hd4 sa = sp[0], sb = sp[1], ba = bp[0], bb = bp[1];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const hd2 (&a)[4] = acc[k];
            float v[8] = {fmaf(a[0].x, sa.x, ba.x), fmaf(a[0].y, sa.y, ba.y), fmaf(a[1].x, sa.z, ba.z), fmaf(a[1].y, sa.w, ba.w),
                          fmaf(a[2].x, sb.x, bb.x), fmaf(a[2].y, sb.y, bb.y), fmaf(a[3].x, sb.z, bb.z), fmaf(a[3].y, sb.w, bb.w)};
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                v[c] = in[k] ? fmaxf(v[c], 0.0f) : 0.0f;  // positions outside the image are conv1's zero padding
                mb = finite_max_nonneg(mb, v[c]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[k][q] = hd2{v[2 * q], v[2 * q + 1]};
        }
    }
    // the tile's power-of-two scale: max |conv0| over the finite values of the patch, the same in every lane
    workgroup_max(finite_max_value(mb), wmax, tid);
    const float pm = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));  // behind the barrier inside: all four are there
    float xs, xs_inv;
    split_xscale_of((unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint(pm)), xs, xs_inv);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        hdu4 hv, lv;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned hi, lo;
            split2(xs, acc[k][q].x, acc[k][q].y, hi, lo, HD_LO_FACTOR);
            hv[q] = hi; lv[q] = lo;
        }
        if (tid + 256 * k < NPX) {
            mid[2 * (tid + 256 * k)] = hv;
            mid[2 * (tid + 256 * k) + 1] = lv;
        }
    }
    __syncthreads();

    // ---- 3: conv1 on the matrix pipe: wave wv = output rows 2 wv, 2 wv + 1, four groups of 16 columns ----
    const int lane = tid & 63, wv = tid >> 6, n = lane & 15, g = lane >> 4;
    hdh8 wf[3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) wf[ky] = *reinterpret_cast<const hdh8*>(p.w1pk + (ky * 64 + lane) * 16);
    // epilogue constants of the lanes that store (g < 2): output channels 4 g .. 4 g + 3
    const int cq = g & 1;
    const hd4 wsc = reinterpret_cast<const hd4*>(p.w1pk + HD_WPK_BYTES)[cq];
    const hd4 s1 = reinterpret_cast<const hd4*>(p.s1)[cq] * wsc;  // 2^k_c folded into the BN scale: exact
    const hd4 b1 = reinterpret_cast<const hd4*>(p.b1)[cq];
    int ymb = HD_FMAX_ZERO;
    float* const yl = p.y + (((size_t)b * H + r0 + 2 * wv) * W + c0 + n) * 8 + 4 * g;  // the lane's pixel of row 0, group 0
#pragma unroll
    for (int cg = 0; cg < 4; ++cg) {
        hd4 ah[2] = {hd4{0.f, 0.f, 0.f, 0.f}, hd4{0.f, 0.f, 0.f, 0.f}};  // A = [w_hi | w_lo], B = a_hi
        hd4 al[2] = {hd4{0.f, 0.f, 0.f, 0.f}, hd4{0.f, 0.f, 0.f, 0.f}};  // B = a_lo
        const int px0 = 2 * wv * MC + cg * 16 + n + g;  // the lane's K slice: pixel n + kx of input row 0, kx = g
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int px = g < 3 ? px0 + rr * MC : NPX;
            const hdh8 fh = __builtin_bit_cast(hdh8, mid[2 * px]);
            const hdh8 fl = __builtin_bit_cast(hdh8, mid[2 * px + 1]);
#pragma unroll
            for (int row = 0; row < 2; ++row) {
                const int ky = rr - row;
                if (ky < 0 || ky > 2) continue;
                ah[row] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ky], fh, ah[row], 0, 0, 0);
                al[row] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ky], fl, al[row], 0, 0, 0);
            }
        }
        const int gc = c0 + cg * 16 + n;
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            const int gr = r0 + 2 * wv + row;
            hd4 r;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float hl = __shfl_down(ah[row][i], 32);  // w_lo a_hi of this lane's channels sits 32 lanes up
                float v = fmaf(hl + al[row][i], 1.0f / HD_LO_FACTOR, ah[row][i]);
                // 2^e here, 2^k_c inside s1: two powers of two, their product may leave fp32's range where the result does not
                r[i] = fmaxf(fmaf(v * xs_inv, s1[i], b1[i]), 0.0f);
            }
            if (g < 2 && gr < H && gc < W) {
                *reinterpret_cast<hd4*>(yl + ((size_t)row * W + cg * 16) * 8) = r;
#pragma unroll
                for (int i = 0; i < 4; ++i) ymb = finite_max_nonneg(ymb, r[i]);
            }
        }
    }
    if (p.tile_max) {  // per-tile maxima with plain stores (a second tiny pass reduces them): no atomics on one address
        const float ym = workgroup_max(finite_max_value(ymb), wmax + 4, tid);
        if (tid == 0) p.tile_max[blockIdx.x] = ym;
    }
}

}  // namespace mvd

extern "C" {

size_t mvd_conv2d_head_split_packed_bytes(void) { return mvd::HD_WPK_BYTES + 8 * sizeof(float); }

int mvd_pack_conv2d_head_split_weights(const float* w1, void* packed, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(w1 && packed, "pack_conv2d_head_split_weights: NULL argument");
    MVD_REQUIRE(((uintptr_t)packed & 15) == 0, "pack_conv2d_head_split_weights: packed must be 16-byte aligned");
    float* wscale = reinterpret_cast<float*>(static_cast<char*>(packed) + HD_WPK_BYTES);
    split_wscale_launch(w1, wscale, 8, 8, 9, false, 8, 8, (hipStream_t)stream);
    hipLaunchKernelGGL(pack_head_split_kernel, dim3(6), dim3(256), 0, (hipStream_t)stream, w1, wscale, static_cast<_Float16*>(packed));
    return launch_status("pack_conv2d_head_split_weights");
}

int mvd_conv2d_head_split_f32(const float* image, const float* w0, const float* scale0, const float* shift0, const void* w1_packed,
                              const float* scale1, const float* shift1, float* y, float* tile_absmax, int B, int H, int W,
                              mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(image && w0 && scale0 && shift0 && w1_packed && scale1 && shift1 && y, "conv2d_head_split: NULL argument");
    MVD_REQUIRE(B > 0 && H > 0 && W > 0, "conv2d_head_split: non-positive dimension");
    MVD_REQUIRE((((uintptr_t)w0 | (uintptr_t)w1_packed | (uintptr_t)scale0 | (uintptr_t)shift0 | (uintptr_t)scale1 | (uintptr_t)shift1 | (uintptr_t)y) & 15) == 0,
                "conv2d_head_split: weights, scales, shifts and y must be 16-byte aligned");
    HeadSplitParams p{};
    p.img = image; p.w0 = w0; p.s0 = scale0; p.b0 = shift0; p.w1pk = static_cast<const char*>(w1_packed); p.s1 = scale1; p.b1 = shift1;
    p.y = y; p.tile_max = tile_absmax;
    p.B = B; p.H = H; p.W = W;
    p.tiles_x = (W + HD_TW - 1) / HD_TW;
    p.tiles_y = (H + HD_TH - 1) / HD_TH;
    const long long nblk = (long long)p.tiles_x * p.tiles_y * B;
    MVD_REQUIRE(nblk <= 0x7fffffffLL, "conv2d_head_split: %lld workgroups exceed the grid limit", nblk);
    hipLaunchKernelGGL(conv2d_head_split_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, p);
    return launch_status("conv2d_head_split");
}

size_t mvd_conv2d_head_tile_count(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)((W + mvd::HD_TW - 1) / mvd::HD_TW) * ((H + mvd::HD_TH - 1) / mvd::HD_TH) * B;
}

int mvd_conv2d_head_f32(const float* image, const float* w0, const float* scale0, const float* shift0, const float* w1,
                        const float* scale1, const float* shift1, float* y, float* tile_absmax, int B, int H, int W,
                        mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(image && w0 && scale0 && shift0 && w1 && scale1 && shift1 && y, "conv2d_head: NULL argument");
    MVD_REQUIRE(B > 0 && H > 0 && W > 0, "conv2d_head: non-positive dimension");
    MVD_REQUIRE((((uintptr_t)w0 | (uintptr_t)w1 | (uintptr_t)scale0 | (uintptr_t)shift0 | (uintptr_t)scale1 | (uintptr_t)shift1 | (uintptr_t)y) & 15) == 0,
                "conv2d_head: weights, scales, shifts and y must be 16-byte aligned");
    HeadParams p{};
    p.img = image; p.w0 = w0; p.s0 = scale0; p.b0 = shift0; p.w1 = w1; p.s1 = scale1; p.b1 = shift1; p.y = y; p.tile_max = tile_absmax;
    p.B = B; p.H = H; p.W = W;
    p.tiles_x = (W + HD_TW - 1) / HD_TW;
    p.tiles_y = (H + HD_TH - 1) / HD_TH;
    const long long nblk = (long long)p.tiles_x * p.tiles_y * B;
    MVD_REQUIRE(nblk <= 0x7fffffffLL, "conv2d_head: %lld workgroups exceed the grid limit", nblk);
    hipLaunchKernelGGL(conv2d_head_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, p);
    return launch_status("conv2d_head");
}
}
