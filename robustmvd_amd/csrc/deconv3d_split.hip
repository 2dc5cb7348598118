// K4's transposed layers (ConvTranspose3d 3x3x3, stride 2, padding 1, output_padding 1: conv7 64 -> 32, conv9 32 -> 16 and
// conv11 16 -> 8 of CostRegNet, rmvd/models/blocks/mvsnet_components.py:84-109) with split fp32 operands on fp16 MFMA:
// deconv3d_all_kernel's decomposition (conv3d.hip) with conv2d_split.hip's arithmetic.
//
// Decomposition: out[2a + p] along each axis uses kernel index 1 on input a (p = 0) or indices 0 / 2 on inputs a + 1 / a (p = 1), so
// every one of the 27 taps belongs to exactly one of the 8 output parity classes (bit per axis = k != 1) and reads the staged
// input at offset (k == 0).  A workgroup (4 waves, wave r = input row r of the tile) stages 2 input planes x (4 + 1) rows x
// (TW + 1) columns ONCE and produces the 2 x 8 x 2 TW output block of all eight classes: no structural zeros among the products,
// and the two w-parities of an output row are stored back to back.
//
// Arithmetic: every activation a and weight w becomes two fp16 terms after an exact power-of-two scaling, a 2^-e = a_hi + a_lo and
// w 2^-k_c = w_hi + w_lo (split_operand.h, lo-term factor 1), and a w is evaluated as w_hi a_hi + w_lo a_hi + w_hi a_lo on
// v_mfma_f32_16x16x32_f16 into ONE fp32 accumulator: 3 MFMAs per (tap, 32 input channels, 16 voxels x 16 output channels) against 8
// fp32 MFMAs of twice the length.  The epilogue multiplies by 2^(e + k_c), applies the folded batch-norm affine, the ReLU and the
// skip addition.  A value v is represented to |error| <= max(2^-22 |v|, 2^-39 max|x|).  inf / NaN inputs give inf / NaN outputs where
// they reach.
//
// GEMM view: A = weights (16 output channels x K 32), B = activations (K 32 x 16 voxels of one input row), so a lane ends up with
// 4 consecutive output channels of one voxel (float4 stores that tile the channel-last output).  K = 32 input channels (CIN = 64:
// two K steps per tap).  CIN = 16 (conv11, 8 output channels) is the PAIR form of deconv3d_pair_kernel: the 16 rows are (output
// w-parity, 8 channels) and K = (input column c: 16 channels | column c + 1: 16 channels) with the weights [kw = 1 | 0] for
// w-parity 0 and [kw = 2 | kw = 0] for w-parity 1: one K step per (kd, kh), four (d, h)-parity classes of accumulators.
//
// LDS: per term and 8-channel group a plane of 16-byte pixels, the planes a whole number of 256-byte bank rows apart: the 16
// voxels of a fragment read 256 contiguous bytes per K group, which is the conflict-free case of ds_read_b128 (DESIGN.md, K4:
// tools/micro/ldsbank.hip; the same layout as conv2d_split.hip's C8S planes).
#include "mvd_common.h"
#include "split_operand.h"
#include <stdlib.h>

// experiments (EXPFLAGS=-DDS_TWO_PHASE=1): the two-phase epilogue of the max |y| variant in the plain variant too
#ifndef DS_TWO_PHASE
#define DS_TWO_PHASE 0
#endif
// experiments (EXPFLAGS=-DDS_STAGE_PIXMAJOR=1): the persistent form stages its slab pixel-major
#ifndef DS_STAGE_PIXMAJOR
#define DS_STAGE_PIXMAJOR 0
#endif

namespace mvd {

typedef _Float16 dsh8 __attribute__((ext_vector_type(8)));
typedef float dsf4 __attribute__((ext_vector_type(4)));
typedef unsigned int dsu4 __attribute__((ext_vector_type(4)));

constexpr int DS_TH = 4, DS_ROWS = DS_TH + 1;

template <int CIN, int MT>
struct DSGeom {
    static constexpr bool PAIR = CIN == 16;
    static constexpr int TW = 16 * MT, COLS = TW + 1;
    static constexpr int NG = CIN / 8;                       // 8-channel groups per voxel
    static constexpr int KS = PAIR ? 1 : CIN / 32;           // K steps per tap
    static constexpr int PIX = 2 * DS_ROWS * COLS;           // staged pixels: [plane 2][row][col]
    static constexpr int GS = (PIX * 16 + 255) / 256 * 256;  // bytes between the planes of consecutive channel groups
    static constexpr int TERM = NG * GS;                     // the hi (or lo) part of the slab
    static constexpr int LDS = 2 * TERM;
    static constexpr int ITEMS = PIX * NG, NIT = (ITEMS + 255) / 256;  // staging items (pixel, 8-channel group)
    static constexpr int NCLS = PAIR ? 4 : 8;                // accumulator classes: (d, h) parities, times w parities
};
// weight fragments (each a hi and a lo term of 64 lanes x 16 bytes) per tile of 16 GEMM rows
static constexpr int ds_nfrag(int cin) { return cin == 16 ? 9 : 27 * (cin / 32); }
static constexpr size_t DS_FRAG_BYTES = 2 * 64 * 16;

// w (Cin, Cout, 3, 3, 3) -> [row tile][fragment][term hi, lo][lane 64][8 halves]; lane l = GEMM row l % 16, K values 8 (l / 16) .. + 7.
// CIN = 32 / 64: row = output channel 16 nt + l % 16, fragment = (tap, K step ks), K = input channel - 32 ks.
// CIN = 16: row = (w-parity pw, channel), fragment = (kd, kh), K = 16 s + input channel, s = 0: input column c (kw = 1 for pw = 0,
// kw = 2 for pw = 1), s = 1: column c + 1 (kw = 0 for pw = 1, nothing for pw = 0).  eun: split_wscale_kernel's 2^k_c per GEMM row
// (entry r of the CIN = 16 form is row r = (w-parity, channel r & 7)), appended to the packed buffer.
__global__ void deconv_split_pack_kernel(const float* __restrict__ w, const float* __restrict__ eun, _Float16* __restrict__ packed, int Cin,
                                         int Cout, int nfrag, long long total) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int j = (int)(e & 7), lane = (int)((e >> 3) & 63), term = (int)((e >> 9) & 1);
    const int f = (int)((e >> 10) % nfrag), nt = (int)((e >> 10) / nfrag);
    const int row = lane & 15, k = 8 * (lane >> 4) + j;
    int cout, cin, tap;
    if (Cin == 16) {
        const int pw = row >> 3, s = k >> 4;
        const int kw = s == 0 ? (pw ? 2 : 1) : (pw ? 0 : -1);
        cout = row & 7; cin = k & 15;
        tap = kw >= 0 ? f * 3 + kw : -1;
    } else {
        const int ks = f % (Cin / 32);
        cout = nt * 16 + row; cin = 32 * ks + k;
        tap = f / (Cin / 32);
    }
    const float v = tap >= 0 ? w[((size_t)cin * Cout + cout) * 27 + tap] / eun[nt * 16 + row] : 0.f;
    _Float16 hi, lo;
    split_weight(v, 1.0f, hi, lo);
    packed[e] = term == 0 ? hi : lo;
}

struct DSParams {
    const float* x;       // (B, Di, hi, wi, CIN) fp32
    const float* xamax;   // max |x| (device, one float)
    const char* wpk;      // packed fragments, then the rows' 2^k_c
    const float* scale;
    const float* shift;
    const float* skip;    // NULL or like y
    float* y;             // (B, 2 Di, 2 hi, 2 wi, Cout) fp32
    float* yamax;         // YAMAX: raised to max |y| over the finite outputs (zeroed by the caller)
    int B, Di, hi, wi, Cout, relu;
    int tiles_w, tiles_h, ncb;  // ncb: output channel blocks of 16 NT channels, one per workgroup
    int tiles;                  // the persistent form: ncb tiles_w tiles_h Di B
};

// NT: 16-channel tiles per workgroup; MT: 16-column tiles per wave (TW = 16 MT input columns); YAMAX: also max |y| (a variant
// of its own, as conv0_split_kernel's)
template <int CIN, int NT, int MT, bool YAMAX>
__global__ void __launch_bounds__(256) deconv3d_split_kernel(DSParams p) {
    const float amax_seen = absmax_seen(YAMAX ? p.yamax : nullptr);  // read now, used at the end (see raise_absmax_seen)
    using G = DSGeom<CIN, MT>;
    constexpr bool PAIR = G::PAIR;
    constexpr int COLS = G::COLS, NG = G::NG, KS = G::KS, GS = G::GS, TERM = G::TERM, NCLS = G::NCLS, NFRAG = ds_nfrag(CIN);
    static_assert(!PAIR || NT == 1, "the pair form has one row tile");
    extern __shared__ __attribute__((aligned(16))) char dslab[];  // [term][channel group][plane 2][row][col] x 16 bytes

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int vox = lane & 15, q = lane >> 4;
    int bx = blockIdx.x;
    const int cb = bx % p.ncb; bx /= p.ncb;  // the channel blocks of a tile run next to each other: one input through one L2
    const int tw = bx % p.tiles_w; bx /= p.tiles_w;
    const int th = bx % p.tiles_h; bx /= p.tiles_h;
    const int zd = bx % p.Di;
    const int b = bx / p.Di;
    const int r0 = th * DS_TH, c0 = tw * G::TW;

    float xsc, xsc_inv;
    split_xscale(p.xamax, xsc, xsc_inv);

    // weight fragments of one (kd, kh) step in one batch, fetched one step ahead of the MFMAs that use them where both batches
    // fit the register file (as deconv3d_all_kernel)
    constexpr int NKW = PAIR ? 1 : 3;
    const char* __restrict__ wl = p.wpk + (size_t)cb * NT * NFRAG * DS_FRAG_BYTES + lane * 16;
    auto load_a = [&](int step, dsh8 (&dst)[NKW][KS][NT][2]) {
#pragma unroll
        for (int kw = 0; kw < NKW; ++kw)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int t = 0; t < 2; ++t)
                        dst[kw][ks][n][t] = *reinterpret_cast<const dsh8*>(
                            wl + ((size_t)n * NFRAG + (step * NKW + kw) * KS + ks) * DS_FRAG_BYTES + t * 1024);
    };
    constexpr bool AHEAD = 2 * NKW * KS * NT * 2 * 4 <= 112;
    dsh8 af[NKW][KS][NT][2];
    if constexpr (AHEAD) load_a(0, af);

    // per-lane constants of this lane's 4 output channels: 2^(e + k_c) as TWO factors 2^floor(s/2) 2^(s - floor(s/2)) (e + k_c alone
    // can leave fp32's exponent range, 2^-157 for activations of 1e-30 and weights of 1e-10, where the result does not),
    // batch-norm scale and shift
    float emul[NT][4], emul2[NT][4], esc[NT][4], esh[NT][4];
    {
        const float* __restrict__ eun = reinterpret_cast<const float*>(p.wpk + (size_t)p.ncb * NT * NFRAG * DS_FRAG_BYTES);
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = (cb * NT + n) * 16 + q * 4 + k;
                const int ch = PAIR ? (row & 7) : row;
                const int se = (int)((__float_as_uint(eun[row]) >> 23) & 0xffu) + (int)((__float_as_uint(xsc_inv) >> 23) & 0xffu) - 254;
                emul[n][k] = __uint_as_float((unsigned)(127 + (se >> 1)) << 23);
                emul2[n][k] = __uint_as_float((unsigned)(127 + se - (se >> 1)) << 23);
                esc[n][k] = p.scale[ch];
                esh[n][k] = p.shift[ch];
            }
    }

    // ---- stage input planes zd and zd + 1 (zero beyond the volume), split into the two fp16 terms on the way ----
    {
        constexpr int NIT = G::NIT, C4 = CIN / 4;
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(p.x) + (size_t)b * p.Di * p.hi * p.wi * C4;
        float4 pf[NIT][2];
        bool ok[NIT];
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int e = tid + 256 * i;
            const int g = e % NG, pix = e / NG;
            const int col = pix % COLS, r = pix / COLS;
            const int pl = r / DS_ROWS, row = r - pl * DS_ROWS;
            const int plane = zd + pl, gr = r0 + row, gc = c0 + col;
            ok[i] = e < G::ITEMS && plane < p.Di && gr < p.hi && gc < p.wi;
            const size_t o = ok[i] ? (((size_t)plane * p.hi + gr) * p.wi + gc) * C4 + 2 * g : 0;
            pf[i][0] = x4[o];
            pf[i][1] = x4[o + 1];
        }
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int e = tid + 256 * i;
            const int g = e % NG, pix = e / NG;
            unsigned h[4], l[4];
            split2(xsc, pf[i][0].x, pf[i][0].y, h[0], l[0]);
            split2(xsc, pf[i][0].z, pf[i][0].w, h[1], l[1]);
            split2(xsc, pf[i][1].x, pf[i][1].y, h[2], l[2]);
            split2(xsc, pf[i][1].z, pf[i][1].w, h[3], l[3]);
            dsu4 hv = {h[0], h[1], h[2], h[3]}, lv = {l[0], l[1], l[2], l[3]};
            if (!ok[i]) { hv = dsu4{0, 0, 0, 0}; lv = dsu4{0, 0, 0, 0}; }
            if (e < G::ITEMS) {
                *reinterpret_cast<dsu4*>(dslab + g * GS + pix * 16) = hv;
                *reinterpret_cast<dsu4*>(dslab + TERM + g * GS + pix * 16) = lv;
            }
        }
    }
    __syncthreads();

    dsf4 acc[NCLS][MT][NT];
#pragma unroll
    for (int c = 0; c < NCLS; ++c)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[c][m][n] = dsf4{0.f, 0.f, 0.f, 0.f};

    // this lane's fragment of GEMM column `vox` of the wave's row: channel group q of the K step (PAIR: group q & 1 of input
    // column vox + (q >> 1))
    const char* __restrict__ lbase = dslab + (PAIR ? (q & 1) * GS + (q >> 1) * 16 : q * GS) + (wave * COLS + vox) * 16;

#pragma unroll
    for (int step = 0; step < 9; ++step) {
        const int kd = step / 3, kh = step % 3;
        dsh8 af_next[NKW][KS][NT][2];
        if constexpr (AHEAD) {
            if (step + 1 < 9) load_a(step + 1, af_next);
        } else {
            load_a(step, af);
        }
        const int rowpix = ((kd == 0 ? DS_ROWS : 0) + (kh == 0)) * COLS;
#pragma unroll
        for (int kw = 0; kw < NKW; ++kw) {
            const int cls = PAIR ? (((kd != 1) << 1) | (kh != 1)) : (((kd != 1) << 2) | ((kh != 1) << 1) | (kw != 1));
            const int colpix = PAIR ? 0 : (kw == 0);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                dsh8 xh[MT], xl[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const char* a = lbase + ks * 4 * GS + (rowpix + colpix + m * 16) * 16;
                    xh[m] = *reinterpret_cast<const dsh8*>(a);
                    xl[m] = *reinterpret_cast<const dsh8*>(a + TERM);
                }
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        acc[cls][m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[kw][ks][n][0], xh[m], acc[cls][m][n], 0, 0, 0);
                        acc[cls][m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[kw][ks][n][1], xh[m], acc[cls][m][n], 0, 0, 0);
                        acc[cls][m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[kw][ks][n][0], xl[m], acc[cls][m][n], 0, 0, 0);
                    }
            }
        }
        if constexpr (AHEAD) {
            if (step + 1 < 9) {
#pragma unroll
                for (int kw = 0; kw < NKW; ++kw)
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                        for (int n = 0; n < NT; ++n) {
                            af[kw][ks][n][0] = af_next[kw][ks][n][0];
                            af[kw][ks][n][1] = af_next[kw][ks][n][1];
                        }
            }
        }
    }

    // ---- epilogue: class (pd, ph, pw) -> output voxel (2 zd + pd, 2 row + ph, 2 col + pw); y = act(conv 2^(e + k_c) scale + shift) + skip.
    // PAIR: the lane's rows are w-parity q >> 1, channels 4 (q & 1) .. + 3 ----
    const int arow = r0 + wave;
    const bool row_ok = arow < p.hi;  // wave-uniform
    auto offset = [&](int c, int m, int n) {  // of the lane's float4 in y (and skip)
        const int pd = PAIR ? c >> 1 : c >> 2, ph = PAIR ? c & 1 : (c >> 1) & 1, pw = PAIR ? q >> 1 : c & 1;
        const size_t row_base = (((size_t)b * 2 * p.Di + 2 * zd + pd) * 2 * p.hi + 2 * arow + ph) * 2 * p.wi;
        const int cbase = PAIR ? 4 * (q & 1) : (cb * NT + n) * 16 + q * 4;
        return (row_base + 2 * (c0 + m * 16 + vox) + pw) * p.Cout + cbase;
    };
    auto finish = [&](int c, int m, int n, size_t o) {
        float4 sk = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.skip) sk = *reinterpret_cast<const float4*>(p.skip + o);
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // the two products are exact (powers of two) unless the result is a denormal
            float val = fmaf(acc[c][m][n][k] * emul[n][k] * emul2[n][k], esc[n][k], esh[n][k]);
            if (p.relu) val = fmaxf(val, 0.f);
            r[k] = val;
        }
        return dsf4{r[0] + sk.x, r[1] + sk.y, r[2] + sk.z, r[3] + sk.w};
    };
    if constexpr (!(YAMAX || DS_TWO_PHASE)) {
        if (row_ok) {
#pragma unroll
            for (int c = 0; c < NCLS; ++c)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    if (c0 + m * 16 + vox >= p.wi) continue;
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const size_t o = offset(c, m, n);
                        *reinterpret_cast<dsf4*>(p.y + o) = finish(c, m, n, o);
                    }
                }
        }
    } else {
        // Two phases: every output value first (in place of its accumulator), then the stores.  max |y| is reduced between the
        // two: a barrier behind the stores would wait for them to be acknowledged (its release fence), and a wave that has
        // issued its stores otherwise just ends.
        [[maybe_unused]] float amax = 0.f;  // max |y| over this lane's finite outputs
        if (row_ok) {
#pragma unroll
            for (int c = 0; c < NCLS; ++c)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    if (c0 + m * 16 + vox >= p.wi) continue;
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const dsf4 out = finish(c, m, n, offset(c, m, n));
                        acc[c][m][n] = out;
                        if constexpr (YAMAX)
                            amax = fmaxf(fmaxf(amax, fmaxf(finite_abs_or_zero(out[0]), finite_abs_or_zero(out[1]))),
                                         fmaxf(finite_abs_or_zero(out[2]), finite_abs_or_zero(out[3])));
                    }
                }
        }
        if constexpr (YAMAX) {  // what the next split-operand layer scales its activations by: ONE atomic per workgroup
            // the four floats: 16 bytes behind the slab, which other waves may still read
            const float m = workgroup_max(amax, reinterpret_cast<float*>(dslab + G::LDS), tid);
            // Against the slot as it was when the workgroup started, and then an atomic whose result nobody waits for: a second
            // look at the slot (raise_absmax) is a dependent load at the very end of the workgroup, and while the slot is still
            // rising, in the first round of resident workgroups of every forward, all of them queue for that one address.
            if (tid == 0) {
                if (m > amax_seen) atomicMax(reinterpret_cast<unsigned*>(p.yamax), __float_as_uint(m));
            }
        }
        if (row_ok) {
#pragma unroll
            for (int c = 0; c < NCLS; ++c)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    if (c0 + m * 16 + vox >= p.wi) continue;
#pragma unroll
                    for (int n = 0; n < NT; ++n) *reinterpret_cast<dsf4*>(p.y + offset(c, m, n)) = acc[c][m][n];
                }
        }
    }
}

// The persistent, software-pipelined form: the same sums in the same order, bit for bit.  A workgroup walks the tiles t = blockIdx.x,
// + gridDim.x, ... (a bound from the parameters alone: no ticket, no flag, no wait on another workgroup), decoded as above; with a
// grid that is a multiple of ncb it keeps its channel block.  Once per workgroup: the activation scale, the per-lane channel
// constants (again only where the channel block changes), and at the very end ONE workgroup_max
// and atomic over everything the workgroup wrote: the lane maximum is carried across the tiles, so the epilogue has one phase and
// no barrier.
//
// Loads in flight.  vmcnt retires in order, so what a step waits for is requested ahead of what may stay outstanding:
//   * weights: LA = 9 (the pair form: 18 fragments, 72 registers) keeps all of them for the life of the workgroup.  LA < 9 streams
//     them LA (kd, kh) steps ahead in a ring that runs on ACROSS the tiles: step s requests the fragments of step (s + LA) % 9, of
//     the next tile once that wraps, into the registers step s - 1 has just finished with (all indices are static: a tile is
//     exactly nine steps);
//   * the skip values and then the next tile's slab (into registers) go out right behind the last request for THIS tile's weights,
//     at step 8 - LA (LA = 9: behind the staging): steps 9 - LA .. 8 and the epilogue wait with the slab still in flight, and it
//     lands under them, the stores and the barrier at the top of the next tile.  SKIP_EARLY = false (conv7, which has no 32
//     registers left for them) reads the skip values behind the last step instead, as deconv3d_split_kernel does.
// For the wait counts to be static every load is unconditional: staging items outside the volume load the batch's first voxel and
// are zeroed when they are split (a neighbour's inf or NaN cannot leak), lanes without an output load the skip of offset 0, a layer
// without a skip reads y in its place and selects zero, and the last tile prefetches its own slab again.
// PIXMAJOR: staging item e = (channel group, pixel) with the pixel running fastest, so that consecutive lanes write consecutive
// 16-byte slots of one plane (no bank conflicts) and read 32 bytes each of consecutive voxels; otherwise the order of
// deconv3d_split_kernel (consecutive lanes read consecutive bytes and write planes a multiple of 256 bytes apart).
template <int CIN, int NT, int MT, bool YAMAX, int LA, int WAVES, bool SKIP_EARLY, bool PIXMAJOR>
__global__ void __launch_bounds__(256, WAVES) deconv3d_split_persist_kernel(DSParams p) {
    const float amax_seen = absmax_seen(YAMAX ? p.yamax : nullptr);
    using G = DSGeom<CIN, MT>;
    constexpr bool PAIR = G::PAIR;
    constexpr int COLS = G::COLS, NG = G::NG, KS = G::KS, GS = G::GS, TERM = G::TERM, NCLS = G::NCLS, NFRAG = ds_nfrag(CIN);
    constexpr int NIT = G::NIT, C4 = CIN / 4, NKW = PAIR ? 1 : 3;
    static_assert(!PAIR || NT == 1, "the pair form has one row tile");
    static_assert(LA >= 1 && LA <= 9 && (LA < 9 || PAIR), "resident weights: the pair form (one channel block) only");
    static_assert(NIT <= 32, "one bit per staging item");
    extern __shared__ __attribute__((aligned(16))) char dslab[];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // a scalar: a tile's output offsets are scalar + lane
    const int vox = lane & 15, q = lane >> 4;
    int t = blockIdx.x;
    if (t >= p.tiles) return;

    float xsc, xsc_inv;
    split_xscale(p.xamax, xsc, xsc_inv);

    struct Tile { int cb, b, zd, r0, c0; };
    auto tile_of = [&](int bx) {
        Tile tl;
        tl.cb = bx % p.ncb; bx /= p.ncb;
        tl.c0 = (bx % p.tiles_w) * G::TW; bx /= p.tiles_w;
        tl.r0 = (bx % p.tiles_h) * DS_TH; bx /= p.tiles_h;
        tl.zd = bx % p.Di;
        tl.b = bx / p.Di;
        return tl;
    };

    // staging item i of this thread, e = tid + 256 i: where it goes in the slab (-1: beyond the items) and which voxel of a tile it
    // is.  Worked out again where it is used (tz: a zero the compiler cannot see through), which is cheaper than 2 NIT registers
    // held for the life of the workgroup.
    struct Item { int loff, pl, row, col, g; };
    auto item_of = [&](int i, int tz) {
        const int e = tid + tz + 256 * i;
        const int g = PIXMAJOR ? e / G::PIX : e % NG, pix = PIXMAJOR ? e % G::PIX : e / NG;
        const int col = pix % COLS, r = pix / COLS;
        const int pl = r / DS_ROWS;
        return Item{e < G::ITEMS ? g * GS + pix * 16 : -1, pl, r - pl * DS_ROWS, col, g};
    };
    // the loads in flight for the next slab, and which of its items lie inside the volume
    float4 pf[NIT][2];
    unsigned okm = 0;
    auto prefetch = [&](const Tile& tl) {
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(p.x) + (size_t)tl.b * p.Di * p.hi * p.wi * C4;
        okm = 0;
        int tz = 0;
        asm volatile("" : "+v"(tz));
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const Item it = item_of(i, tz);
            const int plane = tl.zd + it.pl, gr = tl.r0 + it.row, gc = tl.c0 + it.col;
            const bool ok = it.loff >= 0 && plane < p.Di && gr < p.hi && gc < p.wi;
            const size_t o = ok ? (((size_t)plane * p.hi + gr) * p.wi + gc) * C4 + 2 * it.g : 0;
            pf[i][0] = x4[o];
            pf[i][1] = x4[o + 1];
            okm |= (ok ? 1u : 0u) << i;
        }
    };

    // weight fragments of step `step` of channel block cb
    dsh8 w[9][NKW][KS][NT][2];
    auto load_w = [&](int cb, int step) {
        const char* __restrict__ wl = p.wpk + (size_t)cb * NT * NFRAG * DS_FRAG_BYTES + lane * 16;
#pragma unroll
        for (int kw = 0; kw < NKW; ++kw)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm)
                        w[step][kw][ks][n][tm] = *reinterpret_cast<const dsh8*>(
                            wl + ((size_t)n * NFRAG + (step * NKW + kw) * KS + ks) * DS_FRAG_BYTES + tm * 1024);
    };

    // per-lane constants of this lane's 4 output channels (see deconv3d_split_kernel)
    float emul[NT][4], emul2[NT][4], esc[NT][4], esh[NT][4];
    auto load_consts = [&](int cb) {
        const float* __restrict__ eun = reinterpret_cast<const float*>(p.wpk + (size_t)p.ncb * NT * NFRAG * DS_FRAG_BYTES);
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = (cb * NT + n) * 16 + q * 4 + k;
                const int ch = PAIR ? (row & 7) : row;
                const int se = (int)((__float_as_uint(eun[row]) >> 23) & 0xffu) + (int)((__float_as_uint(xsc_inv) >> 23) & 0xffu) - 254;
                emul[n][k] = __uint_as_float((unsigned)(127 + (se >> 1)) << 23);
                emul2[n][k] = __uint_as_float((unsigned)(127 + se - (se >> 1)) << 23);
                esc[n][k] = p.scale[ch];
                esh[n][k] = p.shift[ch];
            }
    };

    const char* __restrict__ lbase = dslab + (PAIR ? (q & 1) * GS + (q >> 1) * 16 : q * GS) + (wave * COLS + vox) * 16;
    const float* __restrict__ skp = p.skip ? p.skip : p.y;

    Tile tl = tile_of(t);
    load_consts(tl.cb);
    int cb_have = tl.cb;
    prefetch(tl);
#pragma unroll
    for (int s = 0; s < LA; ++s) load_w(tl.cb, s);
    [[maybe_unused]] float amax = 0.f;  // max |y| over this lane's finite outputs, all tiles

    for (;;) {
        const int tn = t + (int)gridDim.x;
        const bool more = tn < p.tiles;
        Tile tnext;  // decoded where the requests for it begin (scalar registers)
        if (tl.cb != cb_have) {
            load_consts(tl.cb);
            cb_have = tl.cb;
        }

        // this lane's outputs: class c, column tile m, channel tile n -> offset of its float4 in y (and skip) = the tile's scalar
        // base (class 0, m 0, n 0) + an offset of 32 bits (the launcher bounds an output plane): one scalar pair for all of them
        const int arow = tl.r0 + wave;
        const bool row_ok = arow < p.hi;  // wave-uniform
        const size_t obase = ((((size_t)tl.b * 2 * p.Di + 2 * tl.zd) * 2 * p.hi + 2 * arow) * 2 * p.wi + 2 * tl.c0) * p.Cout + (PAIR ? 0 : tl.cb * NT * 16);
        auto delta = [&](int c, int m, int n) {
            const int pd = PAIR ? c >> 1 : c >> 2, ph = PAIR ? c & 1 : (c >> 1) & 1, pw = PAIR ? 0 : c & 1;
            return ((pd * 2 * p.hi + ph) * 2 * p.wi + 32 * m + pw) * p.Cout + 16 * n;
        };
        const int lane_off = (2 * vox + (PAIR ? q >> 1 : 0)) * p.Cout + (PAIR ? 4 * (q & 1) : q * 4);
        bool has[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) has[m] = row_ok && tl.c0 + m * 16 + vox < p.wi;

        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();  // every wave has finished reading the previous tile's slab
        int tz = 0;
        asm volatile("" : "+v"(tz));
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int lo = item_of(i, tz).loff;
            if (lo < 0) continue;
            unsigned h[4], l[4];
            split2(xsc, pf[i][0].x, pf[i][0].y, h[0], l[0]);
            split2(xsc, pf[i][0].z, pf[i][0].w, h[1], l[1]);
            split2(xsc, pf[i][1].x, pf[i][1].y, h[2], l[2]);
            split2(xsc, pf[i][1].z, pf[i][1].w, h[3], l[3]);
            dsu4 hv = {h[0], h[1], h[2], h[3]}, lv = {l[0], l[1], l[2], l[3]};
            if (!((okm >> i) & 1u)) { hv = dsu4{0, 0, 0, 0}; lv = dsu4{0, 0, 0, 0}; }
            *reinterpret_cast<dsu4*>(dslab + lo) = hv;
            *reinterpret_cast<dsu4*>(dslab + TERM + lo) = lv;
        }
        __builtin_amdgcn_sched_barrier(0);

        float4 sk[NCLS][MT][NT];
        auto request_skip = [&]() {
#pragma unroll
            for (int c = 0; c < NCLS; ++c)
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int n = 0; n < NT; ++n) sk[c][m][n] = *reinterpret_cast<const float4*>(
                            skp + (row_ok ? obase : 0) + (unsigned)(row_ok && tl.c0 + m * 16 < p.wi ? delta(c, m, n) + (has[m] ? lane_off : 0) : 0));
        };
        auto request_skip_and_slab = [&]() {
            if constexpr (SKIP_EARLY) request_skip();
            tnext = tile_of(more ? tn : t);
            prefetch(tnext);
        };
        if constexpr (LA == 9) {
            request_skip_and_slab();
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();

        dsf4 acc[NCLS][MT][NT];
#pragma unroll
        for (int c = 0; c < NCLS; ++c)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[c][m][n] = dsf4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
        for (int step = 0; step < 9; ++step) {
            const int kd = step / 3, kh = step % 3;
            if constexpr (LA < 9) {
                if (step + LA < 9) load_w(tl.cb, step + LA);
                else load_w(tnext.cb, step + LA - 9);
                if (step == 8 - LA) request_skip_and_slab();
                __builtin_amdgcn_sched_barrier(0);
            }
            const int rowpix = ((kd == 0 ? DS_ROWS : 0) + (kh == 0)) * COLS;
#pragma unroll
            for (int kw = 0; kw < NKW; ++kw) {
                const int cls = PAIR ? (((kd != 1) << 1) | (kh != 1)) : (((kd != 1) << 2) | ((kh != 1) << 1) | (kw != 1));
                const int colpix = PAIR ? 0 : (kw == 0);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    dsh8 xh[MT], xl[MT];
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        const char* a = lbase + ks * 4 * GS + (rowpix + colpix + m * 16) * 16;
                        xh[m] = *reinterpret_cast<const dsh8*>(a);
                        xl[m] = *reinterpret_cast<const dsh8*>(a + TERM);
                    }
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int n = 0; n < NT; ++n) {
                            acc[cls][m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[step][kw][ks][n][0], xh[m], acc[cls][m][n], 0, 0, 0);
                            acc[cls][m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[step][kw][ks][n][1], xh[m], acc[cls][m][n], 0, 0, 0);
                            acc[cls][m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[step][kw][ks][n][0], xl[m], acc[cls][m][n], 0, 0, 0);
                        }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!SKIP_EARLY) request_skip();

        // ---- epilogue, as deconv3d_split_kernel's: y = act(conv 2^(e + k_c) scale + shift) + skip ----
#pragma unroll
        for (int c = 0; c < NCLS; ++c)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    float r[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float val = fmaf(acc[c][m][n][k] * emul[n][k] * emul2[n][k], esc[n][k], esh[n][k]);
                        if (p.relu) val = fmaxf(val, 0.f);
                        r[k] = val;
                    }
                    const float4 s4 = p.skip ? sk[c][m][n] : make_float4(0.f, 0.f, 0.f, 0.f);
                    const dsf4 out = {r[0] + s4.x, r[1] + s4.y, r[2] + s4.z, r[3] + s4.w};
                    if (has[m]) {
                        if constexpr (YAMAX)
                            amax = fmaxf(fmaxf(amax, fmaxf(finite_abs_or_zero(out[0]), finite_abs_or_zero(out[1]))),
                                         fmaxf(finite_abs_or_zero(out[2]), finite_abs_or_zero(out[3])));
                        *reinterpret_cast<dsf4*>(p.y + obase + (unsigned)(delta(c, m, n) + lane_off)) = out;
                    }
                }
        if (!more) break;
        t = tn;
        tl = tnext;
    }
    if constexpr (YAMAX) {  // ONE atomic per workgroup, against the slot as it was when the workgroup started
        const float m = workgroup_max(amax, reinterpret_cast<float*>(dslab + G::LDS), tid);
        if (tid == 0) {
            if (m > amax_seen) atomicMax(reinterpret_cast<unsigned*>(p.yamax), __float_as_uint(m));
        }
    }
}

// The layers of the persistent form: the tile each runs at (the entry point's choice below) and, per layer, how far ahead its weights
// are requested and the waves per SIMD its registers are bounded to.  DS_PERSIST_WGS[layer] = workgroups per CU of its grid where
// the layer passed the ship rule (in the headline forward its median below the minimum of one tile per workgroup,
// profiles/deconv_persist_frame.txt); 0 where the layer stays on deconv3d_split_kernel.  The product library builds the instances of
// the non-zero entries alone; the experiments library builds all of them and reaches them with MVD_DS_PERSIST (0 one tile per
// workgroup, 1 this rule, n > 1 a grid of exactly n workgroups) and MVD_DS_LA (another look-ahead).
enum { DS_CONV7 = 0, DS_CONV9 = 1, DS_CONV11 = 2 };
constexpr int DS_PERSIST_WGS[3] = {2, 2, 2};
template <int CIN> struct DSPersist;
// (ALT_LA, ALT_WAVES: the other instance of the experiments library, MVD_DS_LA=<ALT_LA>)
template <> struct DSPersist<64> { static constexpr int LAYER = DS_CONV7, LA = 1, WAVES = 2, ALT_LA = 1, ALT_WAVES = 2; static constexpr bool SKIP_EARLY = false, ALT_SKIP_EARLY = false; };
template <> struct DSPersist<32> { static constexpr int LAYER = DS_CONV9, LA = 2, WAVES = 2, ALT_LA = 1, ALT_WAVES = 2; static constexpr bool SKIP_EARLY = true, ALT_SKIP_EARLY = true; };
template <> struct DSPersist<16> { static constexpr int LAYER = DS_CONV11, LA = 9, WAVES = 2, ALT_LA = 2, ALT_WAVES = 3; static constexpr bool SKIP_EARLY = true, ALT_SKIP_EARLY = false; };
#ifdef MVD_EXPERIMENTS
constexpr bool DS_EXP = true;
#else
constexpr bool DS_EXP = false;
#endif
// grid of the persistent form (0 = not taken): at most 256 CUs x the table's workgroups, a multiple of ncb so that a workgroup
// keeps its channel block.  (All of them resident beats an even share: conv7's 1152 tiles on 512 workgroups, two or three each,
// take 39 - 41 us alone, on 384 with three each 45 - 47.)
static long long ds_persist_grid(int layer, long long tiles, int ncb, long long plane_floats) {
    if (tiles > 0x3fffffffLL || plane_floats > (1LL << 28)) return 0;  // 32-bit tile indices and in-tile output offsets
    const int wgs = DS_PERSIST_WGS[layer];
    if (const char* e = exp_env("MVD_DS_PERSIST")) {
        const long long v = atoll(e);
        if (v <= 0) return 0;
        if (v > 1) return v < tiles ? v : tiles;
    }
    if (wgs == 0) return 0;
    const long long grid = (256LL * wgs + ncb - 1) / ncb * ncb;
    return grid < tiles ? grid : tiles;
}

template <int CIN, int NT, int MT, bool YAMAX, int LA, int WAVES, bool SKIP_EARLY>
static int ds_launch_persist(const DSParams& p, long long grid, hipStream_t st) {
    using G = DSGeom<CIN, MT>;
    hipLaunchKernelGGL((deconv3d_split_persist_kernel<CIN, NT, MT, YAMAX, LA, WAVES, SKIP_EARLY, DS_STAGE_PIXMAJOR != 0>), dim3((unsigned)grid), dim3(256),
                       G::LDS + 16, st, p);
    return launch_status("deconv3d_split: persistent");
}

// PERSIST: the tile is the one the layer's persistent form is built for
template <int CIN, int NT, int MT, bool YAMAX, bool PERSIST>
static int ds_launch_v(DSParams p, hipStream_t st) {
    using G = DSGeom<CIN, MT>;
    static_assert(G::LDS <= 64 * 1024, "slab exceeds the default LDS limit");
    p.tiles_h = (p.hi + DS_TH - 1) / DS_TH;
    p.tiles_w = (p.wi + G::TW - 1) / G::TW;
    p.ncb = G::PAIR ? 1 : p.Cout / (16 * NT);
    const long long nblk = (long long)p.ncb * p.tiles_w * p.tiles_h * p.Di * p.B;
    MVD_REQUIRE(nblk <= 0x7fffffffLL, "deconv3d_split: %lld workgroups exceed the grid limit", nblk);
    if constexpr (PERSIST && (DS_EXP || DS_PERSIST_WGS[DSPersist<CIN>::LAYER] > 0)) {
        using P = DSPersist<CIN>;
        if (const long long grid = ds_persist_grid(P::LAYER, nblk, p.ncb, (2LL * p.hi + 2) * 2 * p.wi * p.Cout)) {
            p.tiles = (int)nblk;
#ifdef MVD_EXPERIMENTS
            if (const char* e = exp_env("MVD_DS_LA")) {  // the layer's other instance: another look-ahead of the streamed weights
                if (P::ALT_LA != P::LA && atoi(e) == P::ALT_LA) return ds_launch_persist<CIN, NT, MT, YAMAX, P::ALT_LA, P::ALT_WAVES, P::ALT_SKIP_EARLY>(p, grid, st);
            }
#endif
            return ds_launch_persist<CIN, NT, MT, YAMAX, P::LA, P::WAVES, P::SKIP_EARLY>(p, grid, st);
        }
    }
    hipLaunchKernelGGL((deconv3d_split_kernel<CIN, NT, MT, YAMAX>), dim3((unsigned)nblk), dim3(256), G::LDS + 16, st, p);
    return launch_status("deconv3d_split");
}
template <int CIN, int NT, int MT, bool PERSIST = false>
static int ds_launch(const DSParams& p, hipStream_t st) {
    return p.yamax ? ds_launch_v<CIN, NT, MT, true, PERSIST>(p, st) : ds_launch_v<CIN, NT, MT, false, PERSIST>(p, st);
}

}  // namespace mvd

// (Cin, Cout): 64 or 32 input channels with 16, 32, 48 or 64 output channels; 16 -> 8 (the pair form)
static bool ds_shape_ok(int Cin, int Cout) {
    return ((Cin == 64 || Cin == 32) && Cout >= 16 && Cout <= 64 && Cout % 16 == 0) || (Cin == 16 && Cout == 8);
}
static int ds_row_tiles(int Cin, int Cout) { return Cin == 16 ? 1 : Cout / 16; }
static size_t ds_frag_bytes(int Cin, int Cout) { return (size_t)ds_row_tiles(Cin, Cout) * mvd::ds_nfrag(Cin) * mvd::DS_FRAG_BYTES; }

extern "C" {

size_t mvd_deconv3d_split_packed_weight_bytes(int Cin, int Cout) {
    return ds_shape_ok(Cin, Cout) ? ds_frag_bytes(Cin, Cout) + (size_t)ds_row_tiles(Cin, Cout) * 16 * sizeof(float) : 0;
}

int mvd_pack_deconv3d_weights_split(const float* w, int Cin, int Cout, void* packed, mvd_stream_t stream) {
    MVD_REQUIRE(w && packed, "pack_deconv3d_weights_split: NULL argument");
    MVD_REQUIRE(ds_shape_ok(Cin, Cout), "pack_deconv3d_weights_split: 32 or 64 input channels with 16, 32, 48 or 64 output channels, or 16 -> 8, are built (got %d -> %d)",
                Cin, Cout);
    float* eun = reinterpret_cast<float*>(static_cast<char*>(packed) + ds_frag_bytes(Cin, Cout));
    const int rows = ds_row_tiles(Cin, Cout) * 16;
    mvd::split_wscale_launch(w, eun, Cin, Cout, 27, true, rows, rows, (hipStream_t)stream);
    const long long total = (long long)(ds_frag_bytes(Cin, Cout) / 2);
    hipLaunchKernelGGL(mvd::deconv_split_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, eun,
                       (_Float16*)packed, Cin, Cout, mvd::ds_nfrag(Cin), total);
    return mvd::launch_status("pack_deconv3d_weights_split");
}

int mvd_deconv3d_bn_relu_f32_split(const float* x, const float* x_absmax, const void* packed_w, const float* scale, const float* shift,
                                   const float* skip, float* y, float* y_absmax, int B, int Di, int hi, int wi, int Cin, int Cout, int relu,
                                   mvd_stream_t stream) {
    MVD_REQUIRE(x && x_absmax && packed_w && scale && shift && y, "deconv3d_split: NULL argument");
    MVD_REQUIRE(ds_shape_ok(Cin, Cout), "deconv3d_split: 32 or 64 input channels with 16, 32, 48 or 64 output channels, or 16 -> 8, are built (got %d -> %d)", Cin, Cout);
    MVD_REQUIRE(B > 0 && Di > 0 && hi > 0 && wi > 0, "deconv3d_split: non-positive dimension");
    mvd::DSParams p{};
    p.x = x; p.xamax = x_absmax; p.wpk = (const char*)packed_w; p.scale = scale; p.shift = shift; p.skip = skip; p.y = y; p.yamax = y_absmax;
    p.B = B; p.Di = Di; p.hi = hi; p.wi = wi; p.Cout = Cout; p.relu = relu;
    hipStream_t st = (hipStream_t)stream;
    // tile per layer, measured at the headline shapes (tools/bench_deconv_split.py); MVD_DS_CFG = 10 NT + MT picks another one in
    // the experiments library
    int cfg = 0;
    if (const char* e = mvd::exp_env("MVD_DS_CFG")) cfg = atoi(e);
    if (Cin == 16) return cfg % 10 == 3 ? mvd::ds_launch<16, 1, 3>(p, st) : mvd::ds_launch<16, 1, 2, true>(p, st);
    if (Cin == 32) return cfg % 10 == 2 ? mvd::ds_launch<32, 1, 2>(p, st) : mvd::ds_launch<32, 1, 1, true>(p, st);
    if (cfg / 10 == 2 && Cout % 32 == 0) return mvd::ds_launch<64, 2, 1>(p, st);
    return mvd::ds_launch<64, 1, 1, true>(p, st);
}
}
