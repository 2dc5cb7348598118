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
//
// Two kernels, one tile per workgroup (deconv3d_split_kernel) and persistent (deconv3d_split_persist_kernel), that differ in their
// SCHEDULE alone: what is requested when, which barriers, which waits, and how an output's offset is formed.  What they compute
// has one definition each, above them: the tile decode (ds_tile), the per-lane channel constants (ds_chan), the weight fragments of
// a (kd, kh) step (ds_load_w), a staging item, its place in the volume and its split-and-store (ds_item, ds_item_goff,
// ds_stage_store), the (kd, kh) step (ds_kstep), the parities of an accumulator class (ds_class), the epilogue value and the lane's
// max |y| (ds_finish, ds_lane_max) and the workgroup's one atomic (ds_raise); split8_store, split_wpair and split_mfma3 under them
// are the family's (split_operand.h).
#include "mvd_common.h"
#include "split_operand.h"
#include <stdlib.h>

namespace mvd {

constexpr int DS_TH = 4, DS_ROWS = DS_TH + 1;

// weight fragments (each a hi and a lo term of 64 lanes x 16 bytes) per tile of 16 GEMM rows
static constexpr int ds_nfrag(int cin) { return cin == 16 ? 9 : 27 * (cin / 32); }
static constexpr size_t DS_FRAG_BYTES = 2 * 64 * 16;

// MT: 16-column tiles per wave (TW = 16 MT input columns)
template <int CIN_, int MT_>
struct DSGeom {
    static constexpr int CIN = CIN_, MT = MT_;
    static constexpr bool PAIR = CIN == 16;
    static constexpr int TW = 16 * MT, COLS = TW + 1;
    static constexpr int NG = CIN / 8, C4 = CIN / 4;         // 8-channel groups, float4s per voxel
    static constexpr int KS = PAIR ? 1 : CIN / 32;           // K steps per tap
    static constexpr int NKW = PAIR ? 1 : 3;                 // kw taps per (kd, kh) step (the pair form has them inside K)
    static constexpr int NFRAG = ds_nfrag(CIN);
    static constexpr int PIX = 2 * DS_ROWS * COLS;           // staged pixels: [plane 2][row][col]
    static constexpr int GS = (PIX * 16 + 255) / 256 * 256;  // bytes between the planes of consecutive channel groups
    static constexpr int TERM = NG * GS;                     // the hi (or lo) part of the slab
    static constexpr int LDS = 2 * TERM;
    static constexpr int ITEMS = PIX * NG, NIT = (ITEMS + 255) / 256;  // staging items (pixel, 8-channel group)
    static constexpr int NCLS = PAIR ? 4 : 8;                // accumulator classes: (d, h) parities, times w parities
};

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

// ---- what both kernels compute: G = DSGeom<CIN, MT>, NT = 16-channel tiles per workgroup ----

// tile bx of the launch: channel block cb (innermost: the channel blocks of a tile run next to each other, one input through one
// L2), input columns c0 .. + TW, rows r0 .. + 4, planes zd and zd + 1 of batch element b
struct DSTile { int cb, b, zd, r0, c0; };
template <class G>
__device__ __forceinline__ DSTile ds_tile(const DSParams& p, int bx) {
    DSTile tl;
    tl.cb = bx % p.ncb; bx /= p.ncb;
    tl.c0 = (bx % p.tiles_w) * G::TW; bx /= p.tiles_w;
    tl.r0 = (bx % p.tiles_h) * DS_TH; bx /= p.tiles_h;
    tl.zd = bx % p.Di;
    tl.b = bx / p.Di;
    return tl;
}

// per-lane constants of the lane's 4 output channels (4 q .. + 3 of each 16-channel tile of channel block cb): 2^(e + k_c) as TWO
// factors 2^floor(s/2) 2^(s - floor(s/2)) (e + k_c alone can leave fp32's exponent range, 2^-157 for activations of 1e-30 and
// weights of 1e-10, where the result does not), batch-norm scale and shift
template <int NT>
struct DSChan { float mul[NT][4], mul2[NT][4], sc[NT][4], sh[NT][4]; };
template <class G, int NT>
__device__ __forceinline__ void ds_chan(const DSParams& p, int cb, int q, float xsc_inv, DSChan<NT>& c) {
    const float* __restrict__ eun = reinterpret_cast<const float*>(p.wpk + (size_t)p.ncb * NT * G::NFRAG * DS_FRAG_BYTES);
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int row = (cb * NT + n) * 16 + q * 4 + k;
            const int ch = G::PAIR ? (row & 7) : row;
            const int se = (int)((__float_as_uint(eun[row]) >> 23) & 0xffu) + (int)((__float_as_uint(xsc_inv) >> 23) & 0xffu) - 254;
            c.mul[n][k] = __uint_as_float((unsigned)(127 + (se >> 1)) << 23);
            c.mul2[n][k] = __uint_as_float((unsigned)(127 + se - (se >> 1)) << 23);
            c.sc[n][k] = p.scale[ch];
            c.sh[n][k] = p.shift[ch];
        }
}

// the weight fragments of (kd, kh) step `step` of channel block cb, in one batch: [kw][K step][16-channel tile][hi, lo]
template <class G, int NT>
__device__ __forceinline__ void ds_load_w(const DSParams& p, int cb, int lane, int step, sph8 (&dst)[G::NKW][G::KS][NT][2]) {
    const char* __restrict__ wl = p.wpk + (size_t)cb * NT * G::NFRAG * DS_FRAG_BYTES + lane * 16;
#pragma unroll
    for (int kw = 0; kw < G::NKW; ++kw)
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks)
#pragma unroll
            for (int n = 0; n < NT; ++n)
                split_wpair(wl + ((size_t)n * G::NFRAG + (step * G::NKW + kw) * G::KS + ks) * DS_FRAG_BYTES, dst[kw][ks][n][0], dst[kw][ks][n][1]);
}

// staging item e = (pixel e / NG, 8-channel group e % NG) (consecutive lanes read consecutive bytes and write planes a multiple of
// 256 bytes apart), the pixels [plane 2][row][col]: where it goes in one term's half of the slab (-1: beyond the items) and which
// voxel of a tile it is
struct DSItem { int loff, pl, row, col, g; };
template <class G>
__device__ __forceinline__ DSItem ds_item(int e) {
    const int g = e % G::NG, pix = e / G::NG;
    const int col = pix % G::COLS, r = pix / G::COLS;
    const int pl = r / DS_ROWS;
    return DSItem{e < G::ITEMS ? g * G::GS + pix * 16 : -1, pl, r - pl * DS_ROWS, col, g};
}
// ... and its offset in float4s in its batch element's volume; live = it is an item and lies inside the volume, otherwise the
// offset is 0 (both kernels load all the same and zero it when they split it)
template <class G>
__device__ __forceinline__ size_t ds_item_goff(const DSParams& p, const DSTile& tl, const DSItem& it, bool& live) {
    const int plane = tl.zd + it.pl, gr = tl.r0 + it.row, gc = tl.c0 + it.col;
    live = it.loff >= 0 && plane < p.Di && gr < p.hi && gc < p.wi;
    return live ? (((size_t)plane * p.hi + gr) * p.wi + gc) * G::C4 + 2 * it.g : 0;
}
// ... and its eight floats into the slab as their two fp16 terms, zeros for an item outside the volume
template <class G>
__device__ __forceinline__ void ds_stage_store(char* slab, int loff, float xsc, spf4 v0, spf4 v1, bool live) {
    if (loff >= 0) split8_store(slab + loff, G::TERM, xsc, v0, v1, live);
}

// this lane's fragment of GEMM column `vox` of the wave's row: channel group q of the K step (PAIR: group q & 1 of input column
// vox + (q >> 1))
template <class G>
__device__ __forceinline__ const char* ds_lane_base(const char* slab, int wave, int vox, int q) {
    return slab + (G::PAIR ? (q & 1) * G::GS + (q >> 1) * 16 : q * G::GS) + (wave * G::COLS + vox) * 16;
}
// (kd, kh) step `step` of a wave: taps (kd, kh, kw) read the staged input at offset (k == 0) per axis and add into the class with
// bit (k != 1) per axis; w = that step's fragments
template <class G, int NT>
__device__ __forceinline__ void ds_kstep(int step, const char* lbase, const sph8 (&w)[G::NKW][G::KS][NT][2], spf4 (&acc)[G::NCLS][G::MT][NT]) {
    constexpr int MT = G::MT;
    const int kd = step / 3, kh = step % 3;
    const int rowpix = ((kd == 0 ? DS_ROWS : 0) + (kh == 0)) * G::COLS;
#pragma unroll
    for (int kw = 0; kw < G::NKW; ++kw) {
        const int cls = G::PAIR ? (((kd != 1) << 1) | (kh != 1)) : (((kd != 1) << 2) | ((kh != 1) << 1) | (kw != 1));
        const int colpix = G::PAIR ? 0 : (kw == 0);
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
            sph8 xh[MT], xl[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const char* a = lbase + ks * 4 * G::GS + (rowpix + colpix + m * 16) * 16;
                xh[m] = *reinterpret_cast<const sph8*>(a);
                xl[m] = *reinterpret_cast<const sph8*>(a + G::TERM);
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[cls][m][n] = split_mfma3(w[kw][ks][n][0], w[kw][ks][n][1], xh[m], xl[m], acc[cls][m][n]);
        }
    }
}

// class c -> the parities (pd, ph, pw) of its outputs: output voxel (2 zd + pd, 2 row + ph, 2 col + pw).  PAIR: a class is (pd, ph)
// and pw = 0 here; the lane's rows are w-parity q >> 1, channels 4 (q & 1) .. + 3, which the kernels add
template <class G>
__device__ __forceinline__ void ds_class(int c, int& pd, int& ph, int& pw) {
    pd = G::PAIR ? c >> 1 : c >> 2; ph = G::PAIR ? c & 1 : (c >> 1) & 1; pw = G::PAIR ? 0 : c & 1;
}
// the lane's float4 of 16-channel tile n: y = act(conv 2^(e + k_c) scale + shift) + skip.  (sk is a float4 and not an spf4: with the
// skip values as a vector the compiler gives up the packed fp32 instructions of this whole chain)
template <int NT>
__device__ __forceinline__ spf4 ds_finish(const DSParams& p, spf4 a, const DSChan<NT>& c, int n, float4 sk) {
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // the two products are exact (powers of two) unless the result is a denormal
        float val = fmaf(a[k] * c.mul[n][k] * c.mul2[n][k], c.sc[n][k], c.sh[n][k]);
        if (p.relu) val = fmaxf(val, 0.f);
        r[k] = val;
    }
    return spf4{r[0] + sk.x, r[1] + sk.y, r[2] + sk.z, r[3] + sk.w};
}
// max |y| over the lane's finite outputs so far
__device__ __forceinline__ float ds_lane_max(float amax, spf4 out) {
    return fmaxf(fmaxf(amax, fmaxf(finite_abs_or_zero(out[0]), finite_abs_or_zero(out[1]))),
                 fmaxf(finite_abs_or_zero(out[2]), finite_abs_or_zero(out[3])));
}
// What the next split-operand layer scales its activations by: ONE atomic per workgroup.  wmax: the 16 bytes behind the slab, which
// other waves may still read.  Against the slot as it was when the workgroup started (amax_seen, see raise_absmax_seen), and then
// an atomic whose result nobody waits for: a second look at the slot (raise_absmax) is a dependent load at the very end of the
// workgroup, and while the slot is still rising, in the first round of resident workgroups of every forward, all of them queue for
// that one address.
__device__ __forceinline__ void ds_raise(float amax, float* wmax, int tid, float* yamax, float amax_seen) {
    const float m = workgroup_max(amax, wmax, tid);
    if (tid == 0) {
        if (m > amax_seen) atomicMax(reinterpret_cast<unsigned*>(yamax), __float_as_uint(m));
    }
}

// One tile per workgroup.  Schedule: the first step's weights, the channel constants and the slab's loads go out together; one
// barrier behind the staging; the weights of step s + 1 are requested ahead of the MFMAs of step s where both batches fit the
// register file (AHEAD, as deconv3d_all_kernel); the skip values are read in the epilogue.  YAMAX: also max |y| (a variant of its
// own, as conv0_split_kernel's), with the epilogue in two phases.
template <int CIN, int NT, int MT, bool YAMAX>
__global__ void __launch_bounds__(256) deconv3d_split_kernel(DSParams p) {
    const float amax_seen = absmax_seen(YAMAX ? p.yamax : nullptr);  // read now, used at the end (see raise_absmax_seen)
    using G = DSGeom<CIN, MT>;
    constexpr bool PAIR = G::PAIR;
    constexpr int NKW = G::NKW, KS = G::KS, NCLS = G::NCLS, NIT = G::NIT;
    static_assert(!PAIR || NT == 1, "the pair form has one row tile");
    extern __shared__ __attribute__((aligned(16))) char dslab[];  // [term][channel group][plane 2][row][col] x 16 bytes

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int vox = lane & 15, q = lane >> 4;
    const DSTile tl = ds_tile<G>(p, blockIdx.x);

    float xsc, xsc_inv;
    split_xscale(p.xamax, xsc, xsc_inv);

    constexpr bool AHEAD = 2 * NKW * KS * NT * 2 * 4 <= 112;
    sph8 af[NKW][KS][NT][2];
    if constexpr (AHEAD) ds_load_w<G, NT>(p, tl.cb, lane, 0, af);
    DSChan<NT> kc;
    ds_chan<G, NT>(p, tl.cb, q, xsc_inv, kc);

    // ---- stage input planes zd and zd + 1 (zero beyond the volume), split into the two fp16 terms on the way ----
    {
        const spf4* __restrict__ x4 = reinterpret_cast<const spf4*>(p.x) + (size_t)tl.b * p.Di * p.hi * p.wi * G::C4;
        spf4 pf[NIT][2];
        bool ok[NIT];
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const size_t o = ds_item_goff<G>(p, tl, ds_item<G>(tid + 256 * i), ok[i]);
            pf[i][0] = x4[o];
            pf[i][1] = x4[o + 1];
        }
#pragma unroll
        for (int i = 0; i < NIT; ++i) ds_stage_store<G>(dslab, ds_item<G>(tid + 256 * i).loff, xsc, pf[i][0], pf[i][1], ok[i]);
    }
    __syncthreads();

    spf4 acc[NCLS][MT][NT];
#pragma unroll
    for (int c = 0; c < NCLS; ++c)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[c][m][n] = spf4{0.f, 0.f, 0.f, 0.f};

    const char* __restrict__ lbase = ds_lane_base<G>(dslab, wave, vox, q);
#pragma unroll
    for (int step = 0; step < 9; ++step) {
        sph8 af_next[NKW][KS][NT][2];
        if constexpr (AHEAD) {
            if (step + 1 < 9) ds_load_w<G, NT>(p, tl.cb, lane, step + 1, af_next);
        } else {
            ds_load_w<G, NT>(p, tl.cb, lane, step, af);
        }
        ds_kstep<G, NT>(step, lbase, af, acc);
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

    // ---- epilogue: one 64-bit offset per output ----
    const int arow = tl.r0 + wave;
    const bool row_ok = arow < p.hi;  // wave-uniform
    auto offset = [&](int c, int m, int n) {  // of the lane's float4 in y (and skip)
        int pd, ph, pw;
        ds_class<G>(c, pd, ph, pw);
        if (PAIR) pw = q >> 1;
        const size_t row_base = (((size_t)tl.b * 2 * p.Di + 2 * tl.zd + pd) * 2 * p.hi + 2 * arow + ph) * 2 * p.wi;
        const int cbase = PAIR ? 4 * (q & 1) : (tl.cb * NT + n) * 16 + q * 4;
        return (row_base + 2 * (tl.c0 + m * 16 + vox) + pw) * p.Cout + cbase;
    };
    auto finish = [&](int c, int m, int n, size_t o) {
        float4 sk = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.skip) sk = *reinterpret_cast<const float4*>(p.skip + o);
        return ds_finish(p, acc[c][m][n], kc, n, sk);
    };
    if constexpr (!YAMAX) {
        if (row_ok) {
#pragma unroll
            for (int c = 0; c < NCLS; ++c)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    if (tl.c0 + m * 16 + vox >= p.wi) continue;
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const size_t o = offset(c, m, n);
                        *reinterpret_cast<spf4*>(p.y + o) = finish(c, m, n, o);
                    }
                }
        }
    } else {
        // Two phases: every output value first (in place of its accumulator), then the stores.  max |y| is reduced between the
        // two: a barrier behind the stores would wait for them to be acknowledged (its release fence), and a wave that has
        // issued its stores otherwise just ends.
        float amax = 0.f;
        if (row_ok) {
#pragma unroll
            for (int c = 0; c < NCLS; ++c)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    if (tl.c0 + m * 16 + vox >= p.wi) continue;
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        acc[c][m][n] = finish(c, m, n, offset(c, m, n));
                        amax = ds_lane_max(amax, acc[c][m][n]);
                    }
                }
        }
        ds_raise(amax, reinterpret_cast<float*>(dslab + G::LDS), tid, p.yamax, amax_seen);
        if (row_ok) {
#pragma unroll
            for (int c = 0; c < NCLS; ++c)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    if (tl.c0 + m * 16 + vox >= p.wi) continue;
#pragma unroll
                    for (int n = 0; n < NT; ++n) *reinterpret_cast<spf4*>(p.y + offset(c, m, n)) = acc[c][m][n];
                }
        }
    }
}

// The persistent, software-pipelined form: the same sums in the same order, bit for bit.  A workgroup walks the tiles t = blockIdx.x,
// + gridDim.x, ... (a bound from the parameters alone: no ticket, no flag, no wait on another workgroup); with a grid that is a
// multiple of ncb it keeps its channel block.  Once per workgroup: the activation scale, the per-lane channel constants (again only
// where the channel block changes), and at the very end ONE ds_raise over everything the workgroup wrote: the lane maximum is
// carried across the tiles, so the epilogue has one phase and no barrier.
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
// Output offsets: a tile's scalar base plus offsets of 32 bits (with one 64-bit offset per output, as above, conv9 spilled 8 scalar
// registers).
template <int CIN, int NT, int MT, bool YAMAX, int LA, int WAVES, bool SKIP_EARLY>
__global__ void __launch_bounds__(256, WAVES) deconv3d_split_persist_kernel(DSParams p) {
    const float amax_seen = absmax_seen(YAMAX ? p.yamax : nullptr);
    using G = DSGeom<CIN, MT>;
    constexpr bool PAIR = G::PAIR;
    constexpr int NKW = G::NKW, KS = G::KS, NCLS = G::NCLS, NIT = G::NIT;
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

    // The loads in flight for the next slab, and which of its items lie inside the volume.  A thread's item i is e = tid + 256 i,
    // worked out again where it is used (tz: a zero the compiler cannot see through), which is cheaper than 2 NIT registers held for
    // the life of the workgroup.
    spf4 pf[NIT][2];
    unsigned okm = 0;
    auto prefetch = [&](const DSTile& tl) {
        const spf4* __restrict__ x4 = reinterpret_cast<const spf4*>(p.x) + (size_t)tl.b * p.Di * p.hi * p.wi * G::C4;
        okm = 0;
        int tz = 0;
        asm volatile("" : "+v"(tz));
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            bool ok;
            const size_t o = ds_item_goff<G>(p, tl, ds_item<G>(tid + tz + 256 * i), ok);
            pf[i][0] = x4[o];
            pf[i][1] = x4[o + 1];
            okm |= (ok ? 1u : 0u) << i;
        }
    };

    sph8 w[9][NKW][KS][NT][2];  // the ring of weight fragments, by step
    DSChan<NT> kc;
    const char* __restrict__ lbase = ds_lane_base<G>(dslab, wave, vox, q);
    const float* __restrict__ skp = p.skip ? p.skip : p.y;

    DSTile tl = ds_tile<G>(p, t);
    ds_chan<G, NT>(p, tl.cb, q, xsc_inv, kc);
    int cb_have = tl.cb;
    prefetch(tl);
#pragma unroll
    for (int s = 0; s < LA; ++s) ds_load_w<G, NT>(p, tl.cb, lane, s, w[s]);
    [[maybe_unused]] float amax = 0.f;  // max |y| over this lane's finite outputs, all tiles

    for (;;) {
        const int tn = t + (int)gridDim.x;
        const bool more = tn < p.tiles;
        DSTile tnext;  // decoded where the requests for it begin (scalar registers)
        if (tl.cb != cb_have) {
            ds_chan<G, NT>(p, tl.cb, q, xsc_inv, kc);
            cb_have = tl.cb;
        }

        // this lane's outputs: class c, column tile m, channel tile n -> offset of its float4 in y (and skip) = the tile's scalar
        // base (class 0, m 0, n 0) + an offset of 32 bits (the launcher bounds an output plane): one scalar pair for all of them
        const int arow = tl.r0 + wave;
        const bool row_ok = arow < p.hi;  // wave-uniform
        const size_t obase = ((((size_t)tl.b * 2 * p.Di + 2 * tl.zd) * 2 * p.hi + 2 * arow) * 2 * p.wi + 2 * tl.c0) * p.Cout + (PAIR ? 0 : tl.cb * NT * 16);
        auto delta = [&](int c, int m, int n) {
            int pd, ph, pw;
            ds_class<G>(c, pd, ph, pw);
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
        for (int i = 0; i < NIT; ++i) ds_stage_store<G>(dslab, ds_item<G>(tid + tz + 256 * i).loff, xsc, pf[i][0], pf[i][1], (okm >> i) & 1u);
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
            tnext = ds_tile<G>(p, more ? tn : t);
            prefetch(tnext);
        };
        if constexpr (LA == 9) {
            request_skip_and_slab();
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();

        spf4 acc[NCLS][MT][NT];
#pragma unroll
        for (int c = 0; c < NCLS; ++c)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[c][m][n] = spf4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
        for (int step = 0; step < 9; ++step) {
            if constexpr (LA < 9) {
                if (step + LA < 9) ds_load_w<G, NT>(p, tl.cb, lane, step + LA, w[step + LA]);
                else ds_load_w<G, NT>(p, tnext.cb, lane, step + LA - 9, w[step + LA - 9]);
                if (step == 8 - LA) request_skip_and_slab();
                __builtin_amdgcn_sched_barrier(0);
            }
            ds_kstep<G, NT>(step, lbase, w[step], acc);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!SKIP_EARLY) request_skip();

        // ---- epilogue: one phase, the stores go out as the values are ready ----
#pragma unroll
        for (int c = 0; c < NCLS; ++c)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const spf4 out = ds_finish(p, acc[c][m][n], kc, n, p.skip ? sk[c][m][n] : make_float4(0.f, 0.f, 0.f, 0.f));
                    if (has[m]) {
                        if constexpr (YAMAX) amax = ds_lane_max(amax, out);
                        *reinterpret_cast<spf4*>(p.y + obase + (unsigned)(delta(c, m, n) + lane_off)) = out;
                    }
                }
        if (!more) break;
        t = tn;
        tl = tnext;
    }
    if constexpr (YAMAX) ds_raise(amax, reinterpret_cast<float*>(dslab + G::LDS), tid, p.yamax, amax_seen);
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
    hipLaunchKernelGGL((deconv3d_split_persist_kernel<CIN, NT, MT, YAMAX, LA, WAVES, SKIP_EARLY>), dim3((unsigned)grid), dim3(256), G::LDS + 16, st, p);
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
#define DS_SHAPES_BUILT "32 or 64 input channels with 16, 32, 48 or 64 output channels, or 16 -> 8, are built (got %d -> %d)"
static int ds_row_tiles(int Cin, int Cout) { return Cin == 16 ? 1 : Cout / 16; }
static size_t ds_frag_bytes(int Cin, int Cout) { return (size_t)ds_row_tiles(Cin, Cout) * mvd::ds_nfrag(Cin) * mvd::DS_FRAG_BYTES; }

extern "C" {

size_t mvd_deconv3d_split_packed_weight_bytes(int Cin, int Cout) {
    return ds_shape_ok(Cin, Cout) ? ds_frag_bytes(Cin, Cout) + (size_t)ds_row_tiles(Cin, Cout) * 16 * sizeof(float) : 0;
}

int mvd_pack_deconv3d_weights_split(const float* w, int Cin, int Cout, void* packed, mvd_stream_t stream) {
    MVD_REQUIRE(w && packed, "pack_deconv3d_weights_split: NULL argument");
    MVD_REQUIRE(ds_shape_ok(Cin, Cout), "pack_deconv3d_weights_split: " DS_SHAPES_BUILT, Cin, Cout);
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
    MVD_REQUIRE(ds_shape_ok(Cin, Cout), "deconv3d_split: " DS_SHAPES_BUILT, Cin, Cout);
    MVD_REQUIRE(B > 0 && Di > 0 && hi > 0 && wi > 0, "deconv3d_split: non-positive dimension");
    mvd::DSParams p{};
    p.x = x; p.xamax = x_absmax; p.wpk = (const char*)packed_w; p.scale = scale; p.shift = shift; p.skip = skip; p.y = y; p.yamax = y_absmax;
    p.B = B; p.Di = Di; p.hi = hi; p.wi = wi; p.Cout = Cout; p.relu = relu;
    hipStream_t st = (hipStream_t)stream;
    // tile per layer, measured at the headline shapes (tools/bench_deconv_split.py)
#ifdef MVD_EXPERIMENTS  // DS_EXP: MVD_DS_CFG = 10 NT + MT picks one of the other tiles that were measured; no layer runs at one
    if (const char* e = mvd::exp_env("MVD_DS_CFG")) {
        const int cfg = atoi(e);
        if (Cin == 16 && cfg % 10 == 3) return mvd::ds_launch<16, 1, 3>(p, st);
        if (Cin == 32 && cfg % 10 == 2) return mvd::ds_launch<32, 1, 2>(p, st);
        if (Cin == 64 && cfg / 10 == 2 && Cout % 32 == 0) return mvd::ds_launch<64, 2, 1>(p, st);
    }
#endif
    if (Cin == 16) return mvd::ds_launch<16, 1, 2, true>(p, st);
    if (Cin == 32) return mvd::ds_launch<32, 1, 1, true>(p, st);
    return mvd::ds_launch<64, 1, 1, true>(p, st);
}
}

