// Path A's 2-D CNN (the DispNet encoder / context encoder / fusion score convs / cost-volume encoder / decoder of robust_mvd:
// rmvd/models/blocks/dispnet_encoder.py:6-27, dispnet_context_encoder.py, learned_fusion.py:8-20,
// dispnet_costvolume_encoder.py:7-50, dispnet_decoder.py:36-138) as ONE implicit-GEMM kernel family on fp16 MFMA with
// split fp32 operands: fp32-grade results at several times the fp32 matrix rate, no layout transposes, no im2col, no `cat`.
//
// Arithmetic (the 2-D form of conv3d_split.hip): every fp32 activation a and weight w becomes two fp16 terms after an exact
// power-of-two scaling, a 2^-e = a_hi + a_lo and w 2^-k_c = w_hi + w_lo per cout (split_operand.h, lo-term factor 1: with the
// block scaling the lo terms stay in fp16's range as they are, denormals included), and a w is evaluated as
// a_hi w_hi + a_hi w_lo + a_lo w_hi on v_mfma_f32_16x16x32_f16 with ONE fp32 accumulator; the epilogue multiplies by
// 2^(e + k_c).  A value v is represented to |error| <= max(2^-22 |v|, 2^-39 max|x|).  max |x| comes from the producer's
// epilogue (every kernel here can leave max |y| behind: one atomicMax per workgroup) or from mvd_absmax_f32.
//
// Data layout: activations NHWC fp32 with a free pixel stride (so that a layer can read or write a channel slice of a wider
// buffer: the decoder's concat inputs are never copied together), channel count a multiple of 8 (pad channels hold zeros and
// meet zero weights).  Weights pre-split and pre-packed in MFMA fragment order.
//
// GEMM view: D[cout][pixel] += W[cout][k] X[k][pixel], k = (tap, channel).  A workgroup (4 waves) owns a 16 x 16 tile of output
// pixels and BN output channels.  Per chunk of CC = 8 U8 input channels the input patch the tile needs is staged ONCE in LDS
// (converted to the two fp16 terms on the way; zero outside the image = the padding), stride-2 layers de-interleave the
// columns by parity so that the 16 pixels of a fragment read conflict-free.  A K step = 4 units of 8 channels (unit = (tap,
// 8-channel group)): per step a wave reads 2 activation fragments per pixel row from LDS and its weight fragments straight from
// L2 (each wave owns its own output channels, so no weight byte is loaded twice per workgroup), 3 MFMAs per 16 x 16 block.
// Layers with few pixels and many weights (conv5 .. deconv_2) split K over workgroups; partial sums go to a workspace and a
// second kernel adds them in a fixed order (run-to-run identical) and applies the epilogue.
//
// Transposed convolutions (4 x 4, stride 2, padding 1) run as four 2 x 2 stride-1 layers, one per output parity class.
#include "mvd_common.h"
#include "split_operand.h"
#include <algorithm>
#include <stdlib.h>
#include <string>

// knock-out builds for tools/ko_conv2d.sh (timing only, WRONG results): 1 stage only a workgroup's first chunk (the persistent form:
// every tile's first chunk), 2 no MFMAs, 4 weights loaded once, 8 activation fragments read once per step, 16 no stores.  A
// knock-out build never takes the 3-D march: it times the kernels the knock-outs are written into
#ifndef C2_KO
#define C2_KO 0
#endif

namespace mvd {

constexpr int C2_TH = 16, C2_TW = 16;  // output pixels per workgroup tile

template <int KH, int KW, int S, int U8, bool IMG = false>
struct C2Geom {
    static constexpr int CC = 8 * U8;                          // input channels per staged chunk
    static constexpr int PB = 16;                              // LDS bytes per pixel, term and 8-channel group
    static constexpr int PH = (C2_TH - 1) * S + KH, PW = (C2_TW - 1) * S + KW;  // staged patch
    static constexpr int PWS = (PW + S - 1) / S;               // columns per parity plane
    static constexpr int ROWB = S * S * PWS * PB;              // LDS bytes between the patch rows of consecutive OUTPUT rows
    // The 8-channel groups of a chunk are PLANES C8S bytes apart, C8S a multiple of the 256-byte bank row: `ds_read_b128` serves the
    // lanes in four NON-contiguous groups of 16 ({0-3, 12-15, 20-27}, ...), i.e. 8 pixels of one K group of the fragment and the
    // other 8 pixels of the next; with the K groups (= channel groups, when a chunk has 4) a whole number of bank rows apart those
    // 16 lanes read 16 different 16-byte slots.  (Pixel-interleaved groups at an odd pitch of 80 bytes kept ONE K group conflict-free
    // but not the hardware's groups: half of the LDS cycles were bank conflicts, profiles/r03_conv2d_fusion3x3_pmc.txt.)
    static constexpr int C8S = (PH * S * PWS * PB + 255) / 256 * 256;
    static constexpr int PLANE = U8 * C8S;                     // one term of the patch
    static constexpr int UNITS = KH * KW * U8;                 // (tap, 8-channel group) units per chunk
    static constexpr int STEPS = (UNITS + 3) / 4;              // MFMA K steps (32 = 4 units) per chunk
    static constexpr int ITEMS = PH * PW * U8;                 // staging items (pixel, 8-channel group)
    static constexpr int NIT = (ITEMS + 255) / 256;
    static_assert(2 * PLANE <= 80 * 1024, "patch exceeds half the LDS (two workgroups per CU)");
    // THE patch layout, [8-channel group][row][column parity][column / S][PB]: LDS byte of patch pixel (py, px), group c8, in one
    // term's plane.  Every staging store (item_loff, conv2d_split_kernel's own item loop) and the fragment reads (c2_tapoff) go through it.
    static __device__ __forceinline__ int lds_byte(int py, int px, int c8) { return ((py * S + px % S) * PWS + px / S) * PB + c8 * C8S; }
    // The persistent kernels' staging item it = (patch pixel it / U8, group it % U8), pixels row by row: its LDS byte, -1 past the patch ...
    static __device__ __forceinline__ int item_loff(int it) {
        const int pix = it / U8;
        return it < ITEMS ? lds_byte(pix / PW, pix % PW, it % U8) : -1;
    }
    // ... and its offset (floats) in an Hi x Wi input plane with pixels xs floats apart whose pixel (iy0, ix0) is the patch's first:
    // -1 past the patch or outside the image (= the padding).  The plane and the chunk's channel offset are the caller's.
    static __device__ __forceinline__ long long item_goff(int it, int iy0, int ix0, int Hi, int Wi, int xs) {
        const int pix = it / U8, iy = iy0 + pix / PW, ix = ix0 + pix % PW;
        return (it < ITEMS && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) ? ((long long)iy * Wi + ix) * xs + it % U8 * 8 : -1;
    }
};
// The first layer on a planar 3-channel image (7 x 7, stride 2): a pixel is 4 halves (r, g, b, 0) = 8 bytes, rows are stored as
// they are (no parity planes), so the 16 bytes a lane reads are the TWO x-adjacent pixels of taps kx = 2g, 2g + 1 and a K step is
// one kernel row: 7 x 4 = 28 real values of 32 (kx = 7 meets zero weights) in 7 steps, against 13 steps of 8-channel pixels.
template <int KH, int KW, int S, int U8>
struct C2Geom<KH, KW, S, U8, true> {
    static_assert(KH == 7 && KW == 7 && S == 2 && U8 == 1, "image layer: 7 x 7, stride 2");
    static constexpr int CC = 8, PB = 8;
    static constexpr int PH = (C2_TH - 1) * S + KH, PW = (C2_TW - 1) * S + KW + 1;  // + the column tap kx = 7 reads
    static constexpr int ROWB = S * PW * PB;
    static constexpr int PLANE = PH * PW * PB;
    static constexpr int STEPS = KH;
    static constexpr int ITEMS = PH * PW;
    static constexpr int NIT = (ITEMS + 255) / 256;
    static_assert(PW % 2 == 0, "16-byte aligned pixel pairs");
};

struct C2Params {
    const float* x;       // input, NHWC, first channel of the slice; pixel stride xs floats.  NCHW3: (B, 3, Hi, Wi) planes
    const float* xamax;   // max |x| (device, one float)
    const char* wpk;      // packed weight fragments (transposed conv: 4 parity classes, cls_bytes apart)
    const float* eun;     // per output channel 2^k_c (padded to a multiple of 16)
    const float* bias;    // Cout or NULL (3-D layers: the folded batch-norm shift)
    const float* scale;   // NULL, or the folded batch-norm scale per channel: y = act(conv * scale + bias)
    const float* skip;    // NULL, or a tensor laid out like y that is added after the activation
    float* y;             // output, NHWC, first channel of the slice; pixel stride ys floats
    float* yamax;         // optional: max |y| over the finite outputs (atomicMax; zeroed by the caller)
    float* part;          // split-K: partial sums [ksplit][B Ho Wo][ncp]; NULL = direct epilogue
    int B, Hi, Wi, xs, nchunks;   // B = output images of the launch: batch x output planes for a 3-D layer
    // 3-D layers (a 2-D layer has Di = Do = KD = SD = 1, pad_d = 0): image b' = (b, od) reads input planes od * SD - pad_d + kd;
    // chunk = kd * nchunks_c + c.  sub3d: a transposed 3 x 3 x 3 stride-2 layer run as a 2 x 2 x 2 convolution whose output channels
    // are (parity class (ad, ay, ax), channel): class goes to output voxel (2 od + ad, 2 oy + ay, 2 ox + ax)
    int Di, Do, Dy, KD, SD, pad_d, nchunks_c, sub3d, Cr;
    int Ho, Wo;           // output grid of this launch (transposed conv: one parity class = the input grid)
    int Hy, Wy, ys;       // the output tensor's full grid; floats between pixels
    long long ys_row, ys_img, ycs;  // floats between output rows, images and channels (ycs = 1: channel-last)
    int oy_mul, ox_mul;   // output pixel (oy, ox) of the grid lands at (oy * oy_mul + a, ox * ox_mul + b)
    int pad_y, pad_x;     // input row of tap ky for output row oy: oy * S - pad_y + ky
    int Cout, ncp;        // output channels; ncp = Cout padded to the launch's BN
    int tiles_x, tiles_y, nblocks, ksplit, chunks_per_split;
    int tiles;            // the persistent form: tiles of the launch (a workgroup walks blockIdx.x, + gridDim.x, ...)
    int march_td, march_runs;  // the 3-D march: output planes per run, runs per batch element (ceil(Do / march_td))
    int ncls;             // 1, or 4 = the output parity classes (a, b) of a transposed conv: pad - (a, b), output offset (a, b)
    long long cls_bytes;
    int act;              // 0 none, 1 LeakyReLU(slope), 2 ReLU
    float slope;
};

// element e of a packed buffer [...][cout tile nt][chunk][step][term hi, lo][lane 64][8 halves]: lane l holds GEMM row 16 nt + l % 16
// and unit 4 step + l / 16 of the chunk, unit u = (tap u / U8, 8-channel group u % U8), halves j = the group's channels
struct C2FragIdx {
    int j, term, row, g, step, chunk;  // row = l % 16, g = l / 16
    long long rest;                    // what is left of e above the chunk: nt, and the class above it where there is one
};
__device__ __forceinline__ C2FragIdx c2_frag_decode(long long e, int steps, int nchunks) {
    C2FragIdx f;
    const int lane = (int)((e >> 3) & 63);
    f.j = (int)(e & 7); f.term = (int)((e >> 9) & 1);
    long long r = e >> 10;
    f.step = (int)(r % steps); r /= steps;
    f.chunk = (int)(r % nchunks);
    f.rest = r / nchunks;
    f.row = lane & 15; f.g = lane >> 4;
    return f;
}

// -> [class][cout tile (16)][chunk][step][term hi, lo][lane 64][8 halves]; lane l: cout 16 nt + l % 16, unit 4 step + l / 16,
// unit u = (tap u / U8, 8-channel group u % U8), channel = chunk CC + 8 (u % U8) + j.  Units past the taps, channels past Cin
// and output channels past Cout get zeros.  Transposed (4 x 4, stride 2, padding 1) class (a, b): tap (ty, tx) of the 2 x 2
// layer = kernel element (3 - a - 2 ty, 3 - b - 2 tx).
__global__ void c2_pack_kernel(const float* __restrict__ w, const float* __restrict__ eun, _Float16* __restrict__ packed, int Cin, int Cout,
                               int KH, int KW, int U8, int nchunks, int ntiles, int steps, int transposed, long long total) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const C2FragIdx f = c2_frag_decode(e, steps, nchunks);
    const int j = f.j, term = f.term, unit = 4 * f.step + f.g;
    const int nt = (int)(f.rest % ntiles), cls = (int)(f.rest / ntiles);
    const int cout = nt * 16 + f.row;
    int tap = unit / U8, cin = f.chunk * 8 * U8 + 8 * (unit % U8) + j;
    if (transposed == 2) {  // image layer: step = kernel row, lane group = the tap pair kx = 2g, 2g + 1, 4 halves per pixel
        const int kx = 2 * f.g + j / 4;
        tap = kx < KW ? f.step * KW + kx : KH * KW;
        cin = j % 4;
    }
    float v = 0.f;
    if (tap < KH * KW && cin < Cin && cout < Cout) {
        const int ty = tap / KW, tx = tap % KW;
        if (transposed == 1) {
            const int a = cls >> 1, b = cls & 1, ky = 3 - a - 2 * ty, kx = 3 - b - 2 * tx;
            v = w[(((size_t)cin * Cout + cout) * 4 + ky) * 4 + kx];
        } else {
            v = w[(((size_t)cout * Cin + cin) * KH + ty) * KW + tx];
        }
        v = v / eun[cout];
    }
    _Float16 hi, lo;
    split_weight(v, 1.0f, hi, lo);
    packed[e] = term == 0 ? hi : lo;
}

// epilogue of 4 consecutive output channels cb .. cb + 3 of output pixel (oy, ox) of image bi (main kernel and split-K reduce)
// the per-channel constants of output channels cb .. cb + 3 (loaded once per channel group, not once per pixel)
struct C2Chan {
    float mul[4], sc[4], bi[4];  // 2^(e + k_c); batch-norm scale (1 when there is none); bias / shift
};
__device__ __forceinline__ C2Chan c2_chan(const C2Params& p, int cb, float xsc_inv) {
    C2Chan k;
    const int c = p.sub3d ? cb % p.Cr : cb;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool in = cb + r < p.Cout;
        k.mul[r] = in ? p.eun[cb + r] * xsc_inv : 0.f;
        k.sc[r] = (in && p.scale) ? p.scale[c + r] : 1.f;
        k.bi[r] = (in && p.bias) ? p.bias[c + r] : 0.f;
    }
    return k;
}
// offset (floats) of output channel cb of output pixel (oy, ox) of image (b, od); consecutive oy are c2_row_step(p) apart
__device__ __forceinline__ size_t c2_out_offset(const C2Params& p, int b, int od, int oy, int ox, int cls, int cb) {
    int c = cb, zo = od, yo = oy * p.oy_mul + (cls >> 1), xo = ox * p.ox_mul + (cls & 1);
    if (p.sub3d) {
        const int k3 = cb / p.Cr;
        c = cb - k3 * p.Cr;
        zo = 2 * od + (k3 >> 2); yo = 2 * oy + ((k3 >> 1) & 1); xo = 2 * ox + (k3 & 1);
    }
    return ((size_t)b * p.Dy + zo) * p.ys_img + (size_t)yo * p.ys_row + (size_t)xo * p.ys + (size_t)c * p.ycs;
}
__device__ __forceinline__ size_t c2_row_step(const C2Params& p) { return (size_t)(p.sub3d ? 2 : p.oy_mul) * p.ys_row; }
// epilogue of 4 consecutive output channels cb .. cb + 3 at output offset o (main kernel and split-K reduce)
__device__ __forceinline__ void c2_finish(const C2Params& p, size_t o, int cb, spf4 a, const C2Chan& k, float& amax) {
    float r4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v = 0.f;
        if (cb + r < p.Cout) {
            const float conv = a[r] * k.mul[r];  // exact: a power of two
            v = p.scale ? fmaf(conv, k.sc[r], k.bi[r]) : conv + k.bi[r];
            if (p.act == 1) v = v > 0.f ? v : v * p.slope;
            else if (p.act == 2) v = fmaxf(v, 0.f);
            if (p.skip) v += p.skip[o + r * p.ycs];
            amax = fmaxf(amax, finite_abs_or_zero(v));
        }
        r4[r] = v;
    }
    if (cb + 3 < p.Cout && p.ycs == 1) {
        *reinterpret_cast<spf4*>(p.y + o) = spf4{r4[0], r4[1], r4[2], r4[3]};
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (cb + r < p.Cout) p.y[o + r * p.ycs] = r4[r];
    }
}

// a workgroup's tile: cout block nb (innermost, so that consecutive workgroups share a patch), K split ks, parity class, tile column and
// row, output image b = (batch element bb, output plane od)
struct C2Tile {
    int nb, ks, cls, b, od, bb, oy0, ox0, iy0, ix0;
};
template <int S>
__device__ __forceinline__ C2Tile c2_tile(const C2Params& p, int bx) {
    C2Tile t;
    t.nb = bx % p.nblocks; bx /= p.nblocks;
    t.ks = bx % p.ksplit; bx /= p.ksplit;
    t.cls = bx % p.ncls; bx /= p.ncls;
    const int tx = bx % p.tiles_x; bx /= p.tiles_x;
    const int ty = bx % p.tiles_y;
    t.b = bx / p.tiles_y;
    t.od = t.b % p.Do; t.bb = t.b / p.Do;
    t.oy0 = ty * C2_TH; t.ox0 = tx * C2_TW;
    t.iy0 = t.oy0 * S - (p.pad_y - (t.cls >> 1)); t.ix0 = t.ox0 * S - (p.pad_x - (t.cls & 1));  // class (0, 0) for a plain convolution
    return t;
}
// LDS byte offset of this lane's activation fragment per K step (row 0 of the wave's rows)
template <class G, int KW, int S, int U8, int STEPS, bool NCHW3>
__device__ __forceinline__ void c2_tapoff(int (&tapoff)[STEPS], int g, int px16, int row0) {
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        if constexpr (NCHW3) {  // step = kernel row, lane group g = the tap pair kx = 2g, 2g + 1
            tapoff[s] = (s * G::PW + 2 * px16 + 2 * g) * G::PB + row0 * G::ROWB;
        } else {
            int unit = 4 * s + g;
            if (unit >= G::UNITS) unit = 0;  // meets zero weights
            // output pixel (row0, px16) reads patch pixel (ky + row0 S, kx + px16 S).  row0 is added outside lds_byte: inside it, the steps
            // of each kernel row get a base register of their own, where now ONE lane-dependent base serves every step through the
            // reads' offset fields (8 - 10 vector registers on the 9-step chunks)
            const int tap = unit / U8, ky = tap / KW, kx = tap % KW;
            tapoff[s] = G::lds_byte(ky, kx + px16 * S, unit % U8) + row0 * G::ROWB;
        }
    }
}
// The persistent kernels' patch loads of one chunk (8 U8 channels at `chan`) of input plane z of the Di planes that start at plane
// `img0` of x: EVERY staging item loads, so that the vmcnt counts are static - an item outside the image reads the plane's first
// pixel, a plane outside the volume reads plane 0; both are zeroed when they are split.  Returns whether the plane exists.
template <int NIT>
__device__ __forceinline__ int c2_prefetch(const float* x, size_t img0, int z, int Di, size_t plane_floats, int chan, const int (&goff)[NIT],
                                           spf4 (&v0)[NIT], spf4 (&v1)[NIT]) {
    const int zlive = z >= 0 && z < Di;
    const float* xim = x + (img0 + (zlive ? z : 0)) * plane_floats + chan;
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        const float* a = xim + max(goff[k], 0);
        v0[k] = *reinterpret_cast<const spf4*>(a);
        v1[k] = *reinterpret_cast<const spf4*>(a + 4);
    }
    return zlive;
}
// The row pipeline of one K step: the wave's MTW pixel rows in turn, body(m, hi fragment, lo fragment) per row with the activation
// fragments read TWO pixel rows ahead (one row = 3 NTW MFMAs = 48 .. 96 clocks: less than a conflicted LDS read).  a = the lane's
// fragment of row 0 (patch + tapoff[s]).
template <class G, int MTW, class Body>
__device__ __forceinline__ void c2_rows(const char* a, Body&& body) {
    constexpr int PLANE = G::PLANE;
    sph8 xh = *reinterpret_cast<const sph8*>(a), xl = *reinterpret_cast<const sph8*>(a + PLANE);
    sph8 yh = xh, yl = xl;
    if (MTW > 1) {
        yh = *reinterpret_cast<const sph8*>(a + G::ROWB);
        yl = *reinterpret_cast<const sph8*>(a + G::ROWB + PLANE);
    }
#pragma unroll
    for (int m = 0; m < MTW; ++m) {
        const sph8 ch = xh, cl = xl;
        xh = yh; xl = yl;
        if (m + 2 < MTW && !(C2_KO & 8)) {
            yh = *reinterpret_cast<const sph8*>(a + (m + 2) * G::ROWB);
            yl = *reinterpret_cast<const sph8*>(a + (m + 2) * G::ROWB + PLANE);
        }
        body(m, ch, cl);
        __builtin_amdgcn_sched_barrier(0);  // keeps the compiler from hoisting every row's reads to the top (registers)
    }
}
// one K step of a wave: its MTW pixel rows against its NTW weight fragments
template <class G, int MTW, int NTW>
__device__ __forceinline__ void c2_kstep(const char* a, const sph8 (&wh)[NTW], const sph8 (&wl)[NTW], spf4 (&acc)[MTW][NTW]) {
    c2_rows<G, MTW>(a, [&](int m, sph8 ch, sph8 cl) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
            if (C2_KO & 2) {
                acc[m][t][0] += (float)ch[0] * (float)wh[t][0] + (float)cl[1] * (float)wl[t][1];
                continue;
            }
            acc[m][t] = split_mfma3(wh[t], wl[t], ch, cl, acc[m][t]);
        }
    });
}
// the epilogue of cout tile `t` of a wave's MTW output rows in the persistent kernels: the first nrows of them are inside the image,
// row m goes to o0 + m ostep.  (conv2d_split_kernel keeps its own loop: through this helper - either form of the row bound, forced
// inline or not - the compiler computes its row conditions ahead of the chunk loop and keeps them as 64-bit masks, and the 16-row
// tiles spill 13 - 31 scalar registers that they do not spill now.)
template <int MTW, int NT>
__device__ __forceinline__ void c2_finish_rows(const C2Params& p, size_t o0, size_t ostep, int nrows, int cb, const spf4 (&acc)[MTW][NT], int t,
                                               const C2Chan& k, float& amax) {
#pragma unroll
    for (int m = 0; m < MTW; ++m)
        if (m < nrows) c2_finish(p, o0 + m * ostep, cb, acc[m][t], k, amax);
}

template <int KH, int KW, int S, int U8, int WM, int NTW, bool NCHW3>
__global__ void __launch_bounds__(256, 2) conv2d_split_kernel(C2Params p) {
    const float amax_seen = absmax_seen(p.part ? nullptr : p.yamax);  // read now, used by the epilogue
    using G = C2Geom<KH, KW, S, U8, NCHW3>;
    constexpr int WN = 4 / WM, MTW = 16 / WM, STEPS = G::STEPS, PB = G::PB, PLANE = G::PLANE;
    // (Measured and dropped: the next chunk's global reads sent to a per-thread LDS scratch by LDS-DMA under this chunk's MFMAs.
    // vmcnt retires in order, so the weight fragments of the next K step then wait for those slow reads: 5-10 % slower.)
    extern __shared__ __attribute__((aligned(16))) char patch[];  // [term][row][column parity][column / S][PB] | 4 floats
    float* const wmax = reinterpret_cast<float*>(patch + 2 * PLANE);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv / WN, wn = wv % WN;
    const int g = lane >> 4, px16 = lane & 15;

    const C2Tile tl = c2_tile<S>(p, blockIdx.x);
    const int nb = tl.nb, ks = tl.ks, cls = tl.cls, b = tl.b, od = tl.od, bb = tl.bb;
    const int oy0 = tl.oy0, ox0 = tl.ox0, iy0 = tl.iy0, ix0 = tl.ix0;

    float xsc, xsc_inv;
    split_xscale(p.xamax, xsc, xsc_inv);

    // staging items of this thread: global offset (floats, without the chunk's channel offset; -1 = outside the image) and LDS byte.
    // (C2Geom::item_goff / item_loff say the same for the persistent kernels.  Called here, the compiler moves part of this arithmetic
    // into the chunk loop ahead of the patch loads; with the loop written out, 28 of the 32 instances compile to the instructions they
    // had before the shared helpers existed, profiles/c2_one_copy_resources.txt.)
    long long goff[G::NIT];
    int loff[G::NIT];
#pragma unroll
    for (int k = 0; k < G::NIT; ++k) {
        const int it = tid + 256 * k;
        const int pix = it / U8, c8 = it % U8;
        const int py = pix / G::PW, pxx = pix % G::PW;
        const int iy = iy0 + py, ix = ix0 + pxx;
        const bool live = it < G::ITEMS;
        const bool inside = live && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
        if constexpr (NCHW3) {
            goff[k] = inside ? ((long long)b * 3 * p.Hi + iy) * p.Wi + ix : -1;
            loff[k] = live ? pix * PB : -1;
        } else {  // inside its input image; the image (plane) is the chunk's
            goff[k] = inside ? ((long long)iy * p.Wi + ix) * p.xs + c8 * 8 : -1;
            loff[k] = live ? G::lds_byte(py, pxx, c8) : -1;
        }
    }
    int tapoff[STEPS];
    c2_tapoff<G, KW, S, U8, STEPS, NCHW3>(tapoff, g, px16, wm * MTW);

    // weights: this wave's cout tiles
    const int nt0 = nb * (WN * NTW) + wn * NTW;
    const size_t nt_stride = (size_t)p.nchunks * STEPS * 2048;
    const char* wlane = p.wpk + (size_t)cls * p.cls_bytes + (size_t)nt0 * nt_stride + lane * 16;

    spf4 acc[MTW][NTW];
#pragma unroll
    for (int m = 0; m < MTW; ++m)
#pragma unroll
        for (int t = 0; t < NTW; ++t) acc[m][t] = spf4{0, 0, 0, 0};

    const int c_begin = ks * p.chunks_per_split, c_end = min(p.nchunks, c_begin + p.chunks_per_split);

    // weight fragments one K step ahead (steps and chunks are consecutive in the packed buffer); the last prefetch re-reads
    sph8 wh[NTW], wl[NTW];
    const char* wc = wlane + (size_t)c_begin * STEPS * 2048;
    const char* const wlast = wlane + ((size_t)max(c_end, c_begin + 1) * STEPS - 1) * 2048;
    if (c_begin < c_end) {
#pragma unroll
        for (int t = 0; t < NTW; ++t) split_wpair(wc + t * nt_stride, wh[t], wl[t]);
    }

    for (int chunk = c_begin; chunk < c_end; ++chunk) {
        // ---- stage the chunk's patch: global fp32 -> two fp16 terms -> LDS -------------------------------------------------------
        if (!(C2_KO & 1) || chunk == c_begin) {
            spf4 v0[G::NIT], v1[G::NIT];
            const int kd = chunk / p.nchunks_c, zi = od * p.SD - p.pad_d + kd;  // the input plane of this chunk (0 for a 2-D layer)
            const bool zlive = zi >= 0 && zi < p.Di;
            const float* xim = p.x + ((size_t)bb * p.Di + (zlive ? zi : 0)) * p.Hi * p.Wi * p.xs + (size_t)(chunk - kd * p.nchunks_c) * G::CC;
#pragma unroll
            for (int k = 0; k < G::NIT; ++k) {
                v0[k] = spf4{0, 0, 0, 0};
                v1[k] = spf4{0, 0, 0, 0};
                if (goff[k] >= 0 && zlive) {
                    if constexpr (NCHW3) {
                        const size_t pl = (size_t)p.Hi * p.Wi;
                        v0[k][0] = p.x[goff[k]]; v0[k][1] = p.x[goff[k] + pl]; v0[k][2] = p.x[goff[k] + 2 * pl];
                    } else {
                        v0[k] = *reinterpret_cast<const spf4*>(xim + goff[k]);
                        v1[k] = *reinterpret_cast<const spf4*>(xim + goff[k] + 4);
                    }
                }
            }
            __syncthreads();  // every wave has finished reading the previous chunk's patch
#pragma unroll
            for (int k = 0; k < G::NIT; ++k) {
                if (loff[k] < 0) continue;
                if constexpr (NCHW3) {  // (r, g, b, 0): 8 bytes per term
                    unsigned h0, h1, l0, l1;
                    split2(xsc, v0[k][0], v0[k][1], h0, l0);
                    split2(xsc, v0[k][2], v0[k][3], h1, l1);
                    *reinterpret_cast<unsigned long long*>(patch + loff[k]) = (unsigned long long)h0 | ((unsigned long long)h1 << 32);
                    *reinterpret_cast<unsigned long long*>(patch + loff[k] + PLANE) = (unsigned long long)l0 | ((unsigned long long)l1 << 32);
                } else {
                    split8_store(patch + loff[k], PLANE, xsc, v0[k], v1[k]);
                }
            }
            __syncthreads();
        }

        // ---- K steps: activation fragments one pixel row ahead, weights one step ahead ---------------------------------------------
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            sph8 nh[NTW], nl[NTW];
            if (C2_KO & 4) {
#pragma unroll
                for (int t = 0; t < NTW; ++t) { nh[t] = wh[t]; nl[t] = wl[t]; }
            } else {
                const char* wn = wc + 2048;
                wn = wn > wlast ? wlast : wn;
#pragma unroll
                for (int t = 0; t < NTW; ++t) split_wpair(wn + t * nt_stride, nh[t], nl[t]);
                wc += 2048;
            }
            c2_kstep<G, MTW, NTW>(patch + tapoff[s], wh, wl, acc);
#pragma unroll
            for (int t = 0; t < NTW; ++t) { wh[t] = nh[t]; wl[t] = nl[t]; }
        }
    }

    // ---- epilogue: lane holds output channels cb .. cb + 3 of pixel (row m, column px16) -------------------------------------------
    const int ox = ox0 + px16;
    float amax = 0.f;
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
        const int cb = (nt0 + t) * 16 + 4 * g;
        if (p.part) {  // split K: raw partial sums, the reduce kernel applies the epilogue
            if (ox < p.Wo)
#pragma unroll
                for (int m = 0; m < MTW; ++m) {
                    const int oy = oy0 + wm * MTW + m;
                    if (oy >= p.Ho) continue;
                    const size_t pl = ((size_t)b * p.Ho + oy) * p.Wo + ox;
                    *reinterpret_cast<spf4*>(p.part + (((size_t)cls * p.ksplit + ks) * p.B * p.Ho * p.Wo + pl) * p.ncp + cb) = acc[m][t];
                }
            continue;
        }
        if (cb >= p.Cout || ((C2_KO & 16) && p.B > 1000)) continue;
        const C2Chan kc = c2_chan(p, cb, xsc_inv);
        if (ox < p.Wo) {
            const size_t o0 = c2_out_offset(p, bb, od, oy0 + wm * MTW, ox, cls, cb), ostep = c2_row_step(p);
#pragma unroll
            for (int m = 0; m < MTW; ++m)
                if (oy0 + wm * MTW + m < p.Ho) c2_finish(p, o0 + m * ostep, cb, acc[m][t], kc, amax);
        }
    }
    if (p.yamax && !p.part) {  // workgroup_max, spelled out: the call costs <3, 3, 2, 1, 4, 1> its 97th vector register (5 -> 4 waves)
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
        if (lane == 0) wmax[wv] = amax;
        __syncthreads();
        if (tid == 0) {
            amax = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
            raise_absmax_seen(p.yamax, amax, amax_seen);
        }
    }
}

// The persistent, software-pipelined form (non-image layers, no K split).  The product library builds ONE instance of it,
// <3, 3, 1, 1, WM 4>: the 3 x 3 layers with 8-channel chunks (3 K steps) and a 16-channel tile, the only kind it measured faster
// for (C2_PERSIST_WGS below); the other instances exist in the experiments library alone, as the record of that measurement.
// a workgroup walks the tiles t = blockIdx.x, + gridDim.x, ... (a bound from the parameters alone: no ticket, no flag, no wait on
// another workgroup), decoded as above.  Once per workgroup: the activation scale, the staging and fragment offsets, the max-|y|
// atomic, and (while the cout block stays the same, i.e. a grid that is a multiple of nblocks) the per-channel constants.  The
// patch of the NEXT chunk - at the end of a tile the first chunk of the next tile - is loaded into registers right after this
// chunk's patch went to LDS, and lands under the K steps, the epilogue and its stores.  vmcnt retires in order, so everything the K
// steps wait for is requested BEFORE that prefetch: all weight fragments of the chunk go out at its top, and the K loop issues no
// global load; its waits are counted and leave the prefetch outstanding.  For the counts to be static every staging item loads
// unconditionally (items outside the image from the plane's first pixel, zeroed when they are split) and the last chunk of the last
// tile prefetches its own tile's first chunk again.  The sums and their order are those of conv2d_split_kernel: bit-identical.
template <int KH, int KW, int S, int U8, int WM, int NTW, int WAVES>
__global__ void __launch_bounds__(256, WAVES) conv2d_split_persist_kernel(C2Params p) {
    const float amax_seen = absmax_seen(p.yamax);
    using G = C2Geom<KH, KW, S, U8, false>;
    constexpr int WN = 4 / WM, MTW = 16 / WM, STEPS = G::STEPS, PLANE = G::PLANE;
    extern __shared__ __attribute__((aligned(16))) char patch[];
    float* const wmax = reinterpret_cast<float*>(patch + 2 * PLANE);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv / WN, wn = wv % WN;
    const int g = lane >> 4, px16 = lane & 15;
    int t = blockIdx.x;
    if (t >= p.tiles) return;

    float xsc, xsc_inv;
    split_xscale(p.xamax, xsc, xsc_inv);
    int loff[G::NIT];
#pragma unroll
    for (int k = 0; k < G::NIT; ++k) loff[k] = G::item_loff(tid + 256 * k);
    int tapoff[STEPS];
    c2_tapoff<G, KW, S, U8, STEPS, false>(tapoff, g, px16, wm * MTW);
    const size_t nt_stride = (size_t)p.nchunks * STEPS * 2048;
    const size_t plane_floats = (size_t)p.Hi * p.Wi * p.xs;  // < 2^31 (launcher)

    // the loads in flight: the patch of one chunk of one tile.  goff: offset in the plane (floats, -1 = outside the image; 32 bits)
    int goff[G::NIT];
    spf4 v0[G::NIT], v1[G::NIT];
    bool zlive;
    auto prefetch = [&](const C2Tile& tl, int chunk, bool new_tile) {
        if (new_tile) {
#pragma unroll
            for (int k = 0; k < G::NIT; ++k) goff[k] = (int)G::item_goff(tid + 256 * k, tl.iy0, tl.ix0, p.Hi, p.Wi, p.xs);
        }
        const int kd = chunk / p.nchunks_c, zi = tl.od * p.SD - p.pad_d + kd;  // the input plane of this chunk (0 for a 2-D layer)
        zlive = c2_prefetch(p.x, (size_t)tl.bb * p.Di, zi, p.Di, plane_floats, (chunk - kd * p.nchunks_c) * G::CC, goff, v0, v1);
    };

    C2Tile tl = c2_tile<S>(p, t);
    prefetch(tl, 0, true);
    C2Chan kc[NTW];
    int nb_have = -1;
    float amax = 0.f;
    for (;;) {
        const int nt0 = tl.nb * (WN * NTW) + wn * NTW;
        const char* const wlane = p.wpk + (size_t)tl.cls * p.cls_bytes + (size_t)nt0 * nt_stride + lane * 16;
        if (tl.nb != nb_have) {
#pragma unroll
            for (int q = 0; q < NTW; ++q) kc[q] = c2_chan(p, (nt0 + q) * 16 + 4 * g, xsc_inv);
            nb_have = tl.nb;
        }
        const int tn = t + (int)gridDim.x;
        const bool more = tn < p.tiles;
        const C2Tile tnext = c2_tile<S>(p, more ? tn : t);

        spf4 acc[MTW][NTW];
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int q = 0; q < NTW; ++q) acc[m][q] = spf4{0, 0, 0, 0};

        for (int chunk = 0; chunk < p.nchunks; ++chunk) {
            // every weight fragment of the chunk, queued behind this chunk's patch (already in flight) and ahead of the next one's
            sph8 wh[STEPS][NTW], wl[STEPS][NTW];
            const char* const wc = wlane + (size_t)chunk * STEPS * 2048;
#pragma unroll
            for (int s = 0; s < STEPS; ++s)
#pragma unroll
                for (int q = 0; q < NTW; ++q) split_wpair(wc + s * 2048 + q * nt_stride, wh[s][q], wl[s][q]);
            __builtin_amdgcn_sched_barrier(0);
            const bool last = chunk + 1 == p.nchunks;
            const bool stage = !(C2_KO & 1) || chunk == 0;  // the knock-out: a tile's first chunk only, one patch load per tile
            if (stage) {
                __syncthreads();  // every wave has finished reading the previous chunk's patch
#pragma unroll
                for (int k = 0; k < G::NIT; ++k) {
                    if (loff[k] < 0) continue;
                    if (goff[k] < 0 || !zlive) v0[k] = v1[k] = spf4{0, 0, 0, 0};
                    split8_store(patch + loff[k], PLANE, xsc, v0[k], v1[k]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (!(C2_KO & 1) || last) prefetch(last ? tnext : tl, last ? 0 : chunk + 1, last);
            __builtin_amdgcn_sched_barrier(0);
            if (stage) __syncthreads();
#pragma unroll
            for (int s = 0; s < STEPS; ++s) c2_kstep<G, MTW, NTW>(patch + tapoff[s], wh[s], wl[s], acc);
        }

        // ---- epilogue: lane holds output channels cb .. cb + 3 of pixel (row m, column px16) ---------------------------------------
        const int ox = tl.ox0 + px16;
#pragma unroll
        for (int q = 0; q < NTW; ++q) {
            const int cb = (nt0 + q) * 16 + 4 * g;
            if (cb >= p.Cout || ox >= p.Wo) continue;
            const int oy = tl.oy0 + wm * MTW;
            c2_finish_rows(p, c2_out_offset(p, tl.bb, tl.od, oy, ox, tl.cls, cb), c2_row_step(p), p.Ho - oy, cb, acc, q, kc[q], amax);
        }
        if (!more) break;
        t = tn;
        tl = tnext;
    }
    if (p.yamax) {
        amax = workgroup_max(amax, wmax, tid);
        if (tid == 0) raise_absmax_seen(p.yamax, amax, amax_seen);
    }
}

// The 3-D layers' plane-stationary march (3 x 3 x 3, padding 1, stride SD = 1 or 2, 8-channel chunks, 16-channel tile).  A
// workgroup owns one 16 x 16 pixel tile, one cout block and a run of up to p.march_td consecutive output planes od0 .. of one batch
// element, and walks the input planes z0 = SD od0 - 1, z0 + 1, ... that run needs, in order.  Each (plane, 8-channel chunk) is staged
// ONCE (conv2d_split_kernel stages it once per depth tap it serves: 3 times, 1.5 times for stride 2) and every activation fragment
// read from LDS meets the weights of every depth tap the plane serves:
//   stride 1: plane z is kd = 0 of output z + 1, kd = 1 of z, kd = 2 of z - 1: three accumulator sets, output o in set o % 3;
//   stride 2: plane 2 od + 1 is kd = 2 of od and kd = 0 of od + 1, plane 2 od is kd = 1 of od: two sets, output o in set o % 2.
// The march is unrolled by the period of those roles (3 planes, 4 planes), so that a set is a fixed block of registers and nothing
// moves.  An output gets its sums in the order of conv2d_split_kernel - kd outermost (the planes come in that order), then the
// channel chunk, then the K steps, hi hi, lo hi, hi lo into one accumulator - so y and max |y| are bit-identical; planes outside
// the volume are staged as the zero patch they are there, and depth taps that belong to a neighbouring run's outputs are skipped.
// As in the persistent form: grid and work from the parameters alone, every load unconditional, the weights of a chunk requested
// before the prefetch of the next patch (WRES: one channel chunk, all 27 taps' fragments resident for the whole run), one max-|y|
// atomic per workgroup.  SLOTS = 2: the patch alternates between two LDS slots and a chunk costs one barrier (conv0_split_kernel).
template <int R>
struct C3Rot {
    static constexpr int value = R;
};
template <int SD, int WAVES, int SLOTS, bool WRES>
__global__ void __launch_bounds__(256, WAVES) conv3d_split_march_kernel(C2Params p) {
    // max |y| seen so far and its slot wait for the end of the run in vector registers: the scalar file is full
    float amax_seen = absmax_seen(p.yamax);
    float* yamax = p.yamax;
    asm volatile("" : "+v"(amax_seen), "+v"(yamax));
    using G = C2Geom<3, 3, SD, 1, false>;
    constexpr int MTW = 4, STEPS = G::STEPS, PLANE = G::PLANE, NSETS = SD == 1 ? 3 : 2;
    extern __shared__ __attribute__((aligned(16))) char patch[];  // SLOTS x [term][patch] | 4 floats
    float* const wmax = reinterpret_cast<float*>(patch + SLOTS * 2 * PLANE);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = lane >> 4, px16 = lane & 15;

    // the work unit: cout block (innermost: neighbours share the patch), tile column and row, run, batch element
    int bx = blockIdx.x;
    const int nb = bx % p.nblocks; bx /= p.nblocks;
    const int tx = bx % p.tiles_x; bx /= p.tiles_x;
    const int ty = bx % p.tiles_y; bx /= p.tiles_y;
    const int od0 = (bx % p.march_runs) * p.march_td, bb = bx / p.march_runs;
    const int nout = min(p.march_td, p.Do - od0);            // output planes of this run
    const int nplanes = SD == 1 ? nout + 2 : 2 * nout + 1;   // input planes z0 .. z0 + nplanes - 1
    const int z0 = SD * od0 - 1;
    const int oy0 = ty * C2_TH, ox0 = tx * C2_TW, iy0 = oy0 * SD - p.pad_y, ix0 = ox0 * SD - p.pad_x;
    const int ncc = p.nchunks_c;

    float xsc, xsc_inv;
    split_xscale(p.xamax, xsc, xsc_inv);
    int loff[G::NIT], goff[G::NIT];  // LDS byte (-1: no item) and offset in the plane (floats, -1 = outside the image)
#pragma unroll
    for (int k = 0; k < G::NIT; ++k) {
        loff[k] = G::item_loff(tid + 256 * k);
        goff[k] = (int)G::item_goff(tid + 256 * k, iy0, ix0, p.Hi, p.Wi, p.xs);
    }
    int tapoff[STEPS];
    c2_tapoff<G, 3, SD, 1, STEPS, false>(tapoff, g, px16, wv * MTW);
    const size_t plane_floats = (size_t)p.Hi * p.Wi * p.xs;  // < 2^31 (launcher)
    const char* const wlane = p.wpk + (size_t)nb * p.nchunks * STEPS * 2048 + lane * 16;  // chunk kd ncc + c, step s: + (chunk STEPS + s) 2048
    const int cb = nb * 16 + 4 * g, ox = ox0 + px16;
    const C2Chan kc = c2_chan(p, cb, xsc_inv);
    // this lane's outputs of the run's first plane; consecutive planes are p.ys_img apart, rows ostep
    const size_t out0 = c2_out_offset(p, bb, od0, oy0 + wv * MTW, ox, 0, cb), ostep = c2_row_step(p);
    const int nrows = p.Ho - (oy0 + wv * MTW);
    const float* const xrun = p.x + (size_t)bb * p.Di * plane_floats;

    sph8 rh[WRES ? 3 : 1][STEPS], rl[WRES ? 3 : 1][STEPS];
    if constexpr (WRES) {
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
            for (int s = 0; s < STEPS; ++s) split_wpair(wlane + (kd * STEPS + s) * 2048, rh[kd][s], rl[kd][s]);
    }

    // the loads in flight: the patch of one (plane, chunk)
    spf4 v0[G::NIT], v1[G::NIT];
    int zlive;  // (uniform flags are ints: one scalar register each)
    auto prefetch = [&](int z, int c) __attribute__((always_inline)) { zlive = c2_prefetch(xrun, 0, z, p.Di, plane_floats, c * 8, goff, v0, v1); };
    prefetch(z0, 0);

    spf4 acc[MTW][NSETS];  // [pixel row][set]
#pragma unroll
    for (int m = 0; m < MTW; ++m)
#pragma unroll
        for (int q = 0; q < NSETS; ++q) acc[m][q] = spf4{0, 0, 0, 0};
    float amax = 0.f;
    int item = 0;  // (plane, chunk) pairs staged so far: the LDS slot alternates with it

    // plane j of the run in role R = j % 3 (stride 1), j % 4 (stride 2): which depth taps it serves and in which set their output lives
    auto plane = [&](auto rot, int j) __attribute__((always_inline)) {
        constexpr int R = decltype(rot)::value;
        // set of the output that takes this plane as kd = 0, 1, 2 (-1: the plane is no such tap of any output)
        constexpr int SET[3] = {SD == 1 ? R : (R % 2 == 0 ? (R / 2) % 2 : -1), SD == 1 ? (R + 2) % 3 : (R % 2 == 1 ? (R / 2) % 2 : -1),
                                SD == 1 ? (R + 1) % 3 : (R % 2 == 0 ? (R / 2 + 1) % 2 : -1)};
        // that output's index in the run; taps of a neighbouring run's outputs are left out
        const int o[3] = {SD == 1 ? j : j / 2, SD == 1 ? j - 1 : (j - 1) / 2, SD == 1 ? j - 2 : j / 2 - 1};
        int on[3], full = 1;
#pragma unroll
        for (int kd = 0; kd < 3; ++kd) {
            on[kd] = (SET[kd] >= 0 && o[kd] >= 0 && o[kd] < nout) ? 1 : 0;
            full &= on[kd] | (SET[kd] < 0 ? 1 : 0);
        }
        for (int c = 0; c < ncc; ++c) {
            // the weight fragments of the chunk's served taps, queued behind this chunk's patch and ahead of the next one's
            sph8 wh[3][STEPS], wl[3][STEPS];
#pragma unroll
            for (int kd = 0; kd < 3; ++kd) {
                if (SET[kd] < 0) continue;
#pragma unroll
                for (int s = 0; s < STEPS; ++s) {
                    if constexpr (WRES) {
                        wh[kd][s] = rh[kd][s]; wl[kd][s] = rl[kd][s];
                    } else {
                        split_wpair(wlane + (size_t)((kd * ncc + c) * STEPS + s) * 2048, wh[kd][s], wl[kd][s]);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            char* const slot = patch + (SLOTS == 2 ? (item & 1) * 2 * PLANE : 0);
            if (SLOTS == 1) __syncthreads();  // every wave has finished reading the previous chunk's patch
#pragma unroll
            for (int k = 0; k < G::NIT; ++k) {
                if (loff[k] < 0) continue;
                if (goff[k] < 0 || !zlive) v0[k] = v1[k] = spf4{0, 0, 0, 0};
                split8_store(slot + loff[k], PLANE, xsc, v0[k], v1[k]);
            }
            __builtin_amdgcn_sched_barrier(0);
            ++item;
            {   // the next (plane, chunk); the run's last one asks for itself again
                const bool lastc = c + 1 == ncc, lastp = j + 1 == nplanes;
                prefetch(z0 + j + ((lastc && !lastp) ? 1 : 0), lastc ? (lastp ? c : 0) : c + 1);
            }
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                // one K step: an activation fragment per pixel row against the served taps' weights
                c2_rows<G, MTW>(slot + tapoff[s], [&](int m, sph8 ch, sph8 cl) __attribute__((always_inline)) {
                    if (full) {  // the sets are independent: their MFMAs interleave, each set in its own order
#pragma unroll
                        for (int term = 0; term < 3; ++term)
#pragma unroll
                            for (int kd = 0; kd < 3; ++kd)
                                if (SET[kd] >= 0)
                                    acc[m][max(SET[kd], 0)] = __builtin_amdgcn_mfma_f32_16x16x32_f16(term == 1 ? wl[kd][s] : wh[kd][s], term == 2 ? cl : ch,
                                                                                                     acc[m][max(SET[kd], 0)], 0, 0, 0);
                    } else {
#pragma unroll
                        for (int kd = 0; kd < 3; ++kd)
                            if (on[kd]) {  // false for a tap the role does not serve
                                spf4& t = acc[m][max(SET[kd], 0)];
                                t = split_mfma3(wh[kd][s], wl[kd][s], ch, cl, t);
                            }
                    }
                });
            }
        }
        // the output this plane completes (its kd = 2): epilogue, and the set starts over
        if constexpr (SET[2] >= 0) {
            if (on[2]) {
                if (cb < p.Cout && ox < p.Wo) c2_finish_rows(p, out0 + (size_t)o[2] * p.ys_img, ostep, nrows, cb, acc, SET[2], kc, amax);
#pragma unroll
                for (int m = 0; m < MTW; ++m) acc[m][SET[2]] = spf4{0, 0, 0, 0};
            }
        }
    };
    for (int j = 0; j < nplanes; j += (SD == 1 ? 3 : 4)) {  // one turn of the roles
        plane(C3Rot<0>{}, j);
        if (j + 1 < nplanes) plane(C3Rot<1>{}, j + 1);
        if (j + 2 < nplanes) plane(C3Rot<2>{}, j + 2);
        if constexpr (SD == 2)
            if (j + 3 < nplanes) plane(C3Rot<3>{}, j + 3);
    }
    if (yamax) {
        amax = workgroup_max(amax, wmax, tid);
        if (tid == 0) raise_absmax_seen(yamax, amax, amax_seen);
    }
}

// split K, second kernel: partial sums added in the fixed order ks = 0, 1, ...; then the same epilogue.  One thread = 4 channels.
// (Measured and dropped: no second launch, the workgroup that draws the last ticket of a tile adds the partial sums up.  The
// agent-scope release every workgroup then needs before its ticket writes back its XCD's whole L2: the split layers ran 2-5x slower.)
__global__ void __launch_bounds__(256) c2_reduce_kernel(C2Params p) {
    __shared__ float wmax[4];
    // 32-bit index arithmetic (the launcher checks B Ho Wo Cout / 4 < 2^31): with 64-bit divisions in the decode this pass took
    // 2-3x the time of its reads.  blockIdx.y = parity class of a transposed layer.
    const int npix = p.B * p.Ho * p.Wo;
    const int c4n = (p.Cout + 3) / 4;
    const int cls = blockIdx.y;
    float xsc, xsc_inv;
    split_xscale_of(__float_as_uint(*p.xamax), xsc, xsc_inv);
    float amax = 0.f;
    // grid-stride: a workgroup ends with at most one atomic
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix * c4n; i += gridDim.x * 256) {
        const int pl = i / c4n;
        const int cb = (i - pl * c4n) * 4;
        // ksplit is a power of two >= 2: eight loads in flight, added in the fixed order ks = 0, 1, ...
        const float* pp = p.part + ((size_t)cls * p.ksplit * npix + pl) * p.ncp + cb;
        const size_t kstr = (size_t)npix * p.ncp;
        spf4 s = spf4{0, 0, 0, 0};
        int ks = 0;
        for (; ks + 8 <= p.ksplit; ks += 8) {
            spf4 v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = *reinterpret_cast<const spf4*>(pp + (size_t)(ks + q) * kstr);
#pragma unroll
            for (int q = 0; q < 8; ++q) s += v[q];
        }
        for (; ks + 2 <= p.ksplit; ks += 2) {
            const spf4 v0 = *reinterpret_cast<const spf4*>(pp + (size_t)ks * kstr), v1 = *reinterpret_cast<const spf4*>(pp + (size_t)(ks + 1) * kstr);
            s += v0;
            s += v1;
        }
        const int row = pl / p.Wo, ox = pl - row * p.Wo, b = row / p.Ho, oy = row - b * p.Ho;
        const int bb = p.Do == 1 ? b : b / p.Do, od = b - bb * p.Do;
        c2_finish(p, c2_out_offset(p, bb, od, oy, ox, cls, cb), cb, s, c2_chan(p, cb, xsc_inv), amax);
    }
    if (p.yamax) {
        amax = workgroup_max(amax, wmax, threadIdx.x);
        if (threadIdx.x == 0) raise_absmax(p.yamax, amax);
    }
}

// F.interpolate(pred, size = (2h, 2w), mode = "bilinear", align_corners = False) of the decoder (dispnet_decoder.py:131), written
// as C channels of a channel-last slice: x planar (B, C, h, w) -> y[b][oy][ox][0 .. C-1], pixels ys floats apart.  torch's own
// formula and operation order (source index max(0.5 (o + 0.5) - 0.5, 0), the two lambdas, rows blended after columns).
__global__ void __launch_bounds__(256) upsample2x_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, float* yamax, int B, int C, int h,
                                                              int w, int ys) {
    __shared__ float wmax[4];
    const long long n = (long long)B * 4 * h * w;
    float amax = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int ox = (int)(i % (2 * w)), oy = (int)((i / (2 * w)) % (2 * h)), b = (int)(i / (4LL * h * w));
        const float sy = fmaxf(0.5f * ((float)oy + 0.5f) - 0.5f, 0.f), sx = fmaxf(0.5f * ((float)ox + 0.5f) - 0.5f, 0.f);
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const float ly1 = sy - (float)y0, ly0 = 1.f - ly1, lx1 = sx - (float)x0, lx0 = 1.f - lx1;
        for (int c = 0; c < C; ++c) {
            const float* pl = x + ((size_t)b * C + c) * h * w;
            const float v = ly0 * (lx0 * pl[(size_t)y0 * w + x0] + lx1 * pl[(size_t)y0 * w + x1]) +
                            ly1 * (lx0 * pl[(size_t)y1 * w + x0] + lx1 * pl[(size_t)y1 * w + x1]);
            y[(size_t)i * ys + c] = v;
            amax = fmaxf(amax, finite_abs_or_zero(v));
        }
    }
    if (yamax) {
        amax = workgroup_max(amax, wmax, threadIdx.x);
        if (threadIdx.x == 0) raise_absmax(yamax, amax);
    }
}

// ---- 3-D layers of the regulariser (K4) on the same kernel ------------------------------------------------------------------------
// Conv3d (Cout, Cin, 3, 3, 3), padding 1, stride 1 or 2: the depth taps are chunks (chunk = kd * nchunks_c + c), the in-plane taps the
// 3 x 3 of the 2-D kernel.  ConvTranspose3d (Cin, Cout, 3, 3, 3), stride 2, padding 1, output_padding 1: output voxel 2 i + a takes,
// per dimension, kernel element 1 from input i (a = 0), or elements 2 and 0 from inputs i and i + 1 (a = 1): a 2 x 2 x 2 convolution
// over the input grid (tap t reads input i + t) with 8 Cout output channels (parity class k3 = 4 ad + 2 ay + ax, channel c) at
// k3 * Cout + c, zero weights where a class has no such tap.
__device__ __forceinline__ int c3_deconv_kidx(int a, int t) { return a == 0 ? (t == 0 ? 1 : -1) : (t == 0 ? 2 : 0); }

__global__ void c3_pack_kernel(const float* __restrict__ w, const float* __restrict__ eun, _Float16* __restrict__ packed, int Cin, int Cout,
                               int U8, int nchunks_c, int ntiles, int steps, int transposed, long long total) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int KD = transposed ? 2 : 3, KP = transposed ? 2 : 3;  // depth taps, in-plane taps per dimension
    const C2FragIdx f = c2_frag_decode(e, steps, KD * nchunks_c);
    const int j = f.j, term = f.term, unit = 4 * f.step + f.g;
    const int kd = f.chunk / nchunks_c, cc = f.chunk % nchunks_c;
    const int ce = (int)f.rest * 16 + f.row;
    const int tap = unit / U8, cin = cc * 8 * U8 + 8 * (unit % U8) + j;
    const int ncout = transposed ? 8 * Cout : Cout;
    float v = 0.f;
    if (tap < KP * KP && cin < Cin && ce < ncout) {
        const int ty = tap / KP, tx = tap % KP;
        if (transposed) {
            const int k3 = ce / Cout, c = ce % Cout;
            const int kz = c3_deconv_kidx(k3 >> 2, kd), ky = c3_deconv_kidx((k3 >> 1) & 1, ty), kx = c3_deconv_kidx(k3 & 1, tx);
            if (kz >= 0 && ky >= 0 && kx >= 0) v = w[((((size_t)cin * Cout + c) * 3 + kz) * 3 + ky) * 3 + kx];
        } else {
            v = w[((((size_t)ce * Cin + cin) * 3 + kd) * 3 + ty) * 3 + tx];
        }
        v = v / eun[ce];
    }
    _Float16 hi, lo;
    split_weight(v, 1.0f, hi, lo);
    packed[e] = term == 0 ? hi : lo;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct C2Shape {
    int KH, KW, S, U8, steps;
    bool transposed, nchw3;
};

// the layer kinds that are built.  mode 0: Conv2d, 1: ConvTranspose2d 4 x 4 stride 2 padding 1, 2: Conv2d on a (B, 3, H, W) image
static bool c2_shape(int KH, int KW, int stride, int mode, int cin_pad, C2Shape* s) {
    s->transposed = mode == 1;
    s->nchw3 = mode == 2;
    s->KH = KH; s->KW = KW; s->S = stride;
    if (mode == 1) {
        if (KH != 4 || KW != 4 || stride != 2 || cin_pad % 32) return false;
        s->KH = s->KW = 2; s->S = 1; s->U8 = 4;
    } else if (mode == 2) {
        if (KH != 7 || KW != 7 || stride != 2 || cin_pad != 8) return false;
        s->U8 = 1;
        s->steps = 7;
        return true;
    } else if (KH == 1 && KW == 1 && stride == 1) {
        if (cin_pad % 32) return false;
        s->U8 = 4;
    } else if (KH == 3 && KW == 3 && stride == 1) {
        s->U8 = cin_pad % 32 == 0 ? 4 : 1;
    } else if ((KH == 3 && KW == 3 && stride == 2) || (KH == 5 && KW == 5 && stride == 2)) {
        s->U8 = 1;
    } else {
        return false;
    }
    if (cin_pad % (8 * s->U8)) return false;
    s->steps = (s->KH * s->KW * s->U8 + 3) / 4;
    return true;
}

// output channels per workgroup: the widest tile that does not leave most of it empty
static int c2_bn(int cout) {
    if (const char* e = exp_env("MVD_C2_BN")) {  // experiments library: forced channel tile (tools/sweep_conv2d_plan.py, both of its sweeps)
        const int v = atoi(e);
        if (v == 16 || v == 32 || v == 64 || v == 128) return v;
    }
    return cout > 64 ? 128 : cout > 32 ? 64 : cout > 16 ? 32 : 16;
}
static int c2_ntiles(int cout) { return (cout + c2_bn(cout) - 1) / c2_bn(cout) * (c2_bn(cout) / 16); }  // 16-channel tiles, whole workgroups
static size_t c2_frag_bytes(const C2Shape& s, int cin_pad, int cout) {
    const size_t nchunks = (size_t)cin_pad / (8 * s.U8);
    return (s.transposed ? 4 : 1) * (size_t)c2_ntiles(cout) * nchunks * s.steps * 2048;
}
static int c2_cpad(int cout) { return (cout + 127) / 128 * 128; }  // eun entries: any BN reads whole float4s

// grid of one layer: output size, channel tile, and over how many workgroups the reduction is split (where the plain grid would
// leave most of the 256 CUs idle and there are chunks to share out)
struct C2Plan {
    int Ho, Wo, tiles_x, tiles_y, bn, nblocks, ncp, ncls, nchunks, ksplit;
    long long tiles;
    long long persist;  // 0: one tile per workgroup; else the grid of conv2d_split_persist_kernel
    int march_td;       // 3-D layers: 0, or the output planes per run of conv3d_split_march_kernel (which then replaces both forms)
    size_t part_bytes;
};

// The persistent form is built for the 3 x 3 (both chunk widths), 3 x 3 stride-2 and 5 x 5 stride-2 layers with up to 64 output
// channels per workgroup.  C2_PERSIST_WGS[kind][bn index] = workgroups per CU of its grid where it is faster than one tile per
// workgroup by more than the spread of the timing, layer by layer (profiles/c2_persistent_layers.txt) AND in the headline forward
// (profiles/c2_persistent_frame.txt); 0 where the layer stays on conv2d_split_kernel.  Only the 3 x 3 layers with 8-channel chunks
// and a 16-channel tile pass both: the 7- and 9-step chunks pay for all their weight fragments up front with the third wave per
// SIMD (20 - 55 % slower), and the stride-2 layers gain 10 % alone but nothing between their neighbours in the frame.
enum { C2_K33 = 0, C2_K33W = 1, C2_K33S2 = 2, C2_K55S2 = 3, C2_NOT_PERSISTENT = -1 };
static int c2_persist_kind(const C2Shape& s) {
    if (s.nchw3 || s.transposed) return C2_NOT_PERSISTENT;
    if (s.KH == 3 && s.KW == 3 && s.S == 1) return s.U8 == 4 ? C2_K33W : s.U8 == 1 ? C2_K33 : C2_NOT_PERSISTENT;
    if (s.KH == 3 && s.KW == 3 && s.S == 2 && s.U8 == 1) return C2_K33S2;
    if (s.KH == 5 && s.KW == 5 && s.S == 2 && s.U8 == 1) return C2_K55S2;
    return C2_NOT_PERSISTENT;
}
constexpr int C2_PERSIST_WGS[4][3] = {
    // bn 16, 32, 64
    {4, 0, 0},  // 3 x 3, 8-channel chunks: in the frame FeatureNet's conv3 80 -> 49 us, conv4 62 -> 47, the regulariser's conv2 132 -> 124
    {0, 0, 0},  // 3 x 3, 32-channel chunks
    {0, 0, 0},  // 3 x 3 stride 2: the regulariser's conv1 151 -> 155 us, conv5 54 -> 54 in the frame
    {0, 0, 0},  // 5 x 5 stride 2
};
// The 3-D layers' march along depth (conv3d_split_march_kernel) replaces both forms above for 3 x 3 x 3 layers with 8-channel
// chunks, a 16-channel tile and an unsplit reduction whose (tile, run) pairs give every CU a workgroup.  C3_MARCH_TD[stride - 1][one
// channel chunk, more] = output planes per run where the layer's median in the headline forward is below its minimum on the kernels
// above (profiles/c3_march_frame.txt), 0 where it stays on them.
constexpr int C3_MARCH_TD[2][2] = {
    // stride 1.  The regulariser's conv2 (16 -> 16, two chunks, 128 planes of 6 x 9 tiles): alone 120 - 130 us persistent, 127 - 139 on
    // runs of 16 (432 workgroups), 123 - 134 on runs of 15, 138 - 205 on runs of 8, 11, 13, 22 and 32: stays
    {0, 0},
    // stride 2.  The regulariser's conv1 (8 -> 16, one chunk: the weights stay in registers): 152.8 (min 152.0) -> 128.5 us in the
    // frame on runs of 16, alone 152 - 165 -> 124 - 133 (runs of 15 the same, 8 135 - 161, 32 178 - 186).  More chunks: not measured
    // at a shape that fills the device, and that instance spills 6 scalar registers
    {16, 0},
};
constexpr long long C3_MARCH_MIN_WGS = 256;
// experiments library, MVD_C3_MARCH: 0 off, 1 the rule, n > 1 runs of n planes at any shape (the channel tile narrowed to 16 for it)
static int c3_march_forced() {
    const char* e = exp_env("MVD_C3_MARCH");
    return e ? std::max(atoi(e), 0) : 1;
}
static long long c3_march_wgs(const C2Plan& q, int B, int Do, int td) {
    return (long long)q.tiles_x * q.tiles_y * q.nblocks * B * ((Do + td - 1) / td);
}
// B: batch elements, Do: output planes of each
static int c3_march_td(const C2Shape& s, const C2Plan& q, int B, int Do, int Hi, int Wi, int xs) {
    if (s.KH != 3 || s.U8 != 1 || q.bn != 16 || q.ksplit != 1 || (long long)Hi * Wi * xs > 0x7fffffffLL) return 0;
    if (C2_KO) return 0;  // the knock-outs are built into the kernels above
    const int forced = c3_march_forced();
    if (forced != 1) return std::min(forced, Do);
    const int td = std::min(C3_MARCH_TD[s.S - 1][q.nchunks == 3 ? 0 : 1], Do);
    return (td > 0 && c3_march_wgs(q, B, Do, td) >= C3_MARCH_MIN_WGS) ? td : 0;
}
// grid of the persistent form (0 = not taken): at most 256 CUs x the table's workgroups, a multiple of nblocks so that a workgroup
// keeps its cout block
static long long c2_persist_grid(const C2Shape& s, const C2Plan& q, int Hi, int Wi, int xs) {
    const int kind = c2_persist_kind(s);
    if (kind == C2_NOT_PERSISTENT || q.bn > 64 || q.ksplit != 1 || q.tiles > 0x7fffffffLL || (long long)Hi * Wi * xs > 0x7fffffffLL) return 0;
    const int wgs = C2_PERSIST_WGS[kind][q.bn == 16 ? 0 : q.bn == 32 ? 1 : 2];
    if (const char* e = exp_env("MVD_C2_PERSIST")) {  // experiments library: 0 off, 1 the rule, n > 1 a grid of exactly n workgroups
        const long long v = atoll(e);
        if (v <= 0) return 0;
        if (v > 1) return std::min<long long>(v, q.tiles);
    }
    if (wgs == 0) return 0;
    return std::min(q.tiles, (256LL * wgs + q.nblocks - 1) / q.nblocks * q.nblocks);
}
// over how many workgroups the reduction of a grid of `tiles` workgroups with `nchunks` chunks each is split
static int c2_ksplit(long long tiles, int nchunks) {
    int ksplit = 1;  // a grid of 128+ workgroups runs as it is: the second pass would cost more than the idle CUs
    if (tiles < 128)
        while (tiles * ksplit < 320 && ksplit < 32 && nchunks / (ksplit * 2) >= 2) ksplit *= 2;
    if (const char* e = exp_env("MVD_C2_KSPLIT")) {  // experiments library: forced split of the reduction
        const int v = atoi(e);
        if (v >= 1 && v <= 32 && (v & (v - 1)) == 0 && v <= nchunks) ksplit = v;
    }
    return ksplit;
}
// what both plans end with: the K split, its workspace (B = output images of the launch) and the persistent grid
static void c2_plan_finish(const C2Shape& s, C2Plan& q, int B, int Hi, int Wi, int xs) {
    q.ksplit = c2_ksplit(q.tiles, q.nchunks);
    q.part_bytes = q.ksplit > 1 ? (size_t)q.ksplit * q.ncls * B * q.Ho * q.Wo * q.ncp * sizeof(float) : 0;
    q.persist = c2_persist_grid(s, q, Hi, Wi, xs);
}
// what both plans start with: the tiles of `images` Ho x Wo output images (planes and parity classes count as images) with `bn`
// output channels per workgroup
static void c2_plan_tiles(C2Plan& q, int Ho, int Wo, long long images, int cout, int bn) {
    q.Ho = Ho; q.Wo = Wo; q.bn = bn;
    q.tiles_y = (Ho + C2_TH - 1) / C2_TH;
    q.tiles_x = (Wo + C2_TW - 1) / C2_TW;
    q.nblocks = (cout + bn - 1) / bn;
    q.ncp = q.nblocks * bn;
    q.tiles = (long long)q.tiles_x * q.tiles_y * images * q.nblocks;
}
static C2Plan c2_plan(const C2Shape& s, int B, int Hi, int Wi, int cin_pad, int xs, int cout, int KH, int KW, int stride) {
    C2Plan q{};
    q.ncls = s.transposed ? 4 : 1;
    if (s.transposed) c2_plan_tiles(q, Hi, Wi, 4LL * B, cout, c2_bn(cout));
    else c2_plan_tiles(q, (Hi + 2 * (KH / 2) - KH) / stride + 1, (Wi + 2 * (KW / 2) - KW) / stride + 1, B, cout, c2_bn(cout));
    q.nchunks = cin_pad / (8 * s.U8);
    c2_plan_finish(s, q, B, Hi, Wi, xs);
    return q;
}

// every launch of the three main kernels: `lds` bytes of dynamic LDS (above 48 KiB the kernel has to be told), 256 threads
template <class K>
static int c2_launch_lds(K kern, int lds, long long grid, const C2Params& p, hipStream_t st, const char* what) {
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return launch_status((std::string(what) + ": LDS attribute").c_str());
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, st, p);
    return launch_status(what);
}
template <int KH, int KW, int S, int U8, int WM, int NTW, bool NCHW3>
static int c2_launch(const C2Params& p, long long nblk, hipStream_t st) {
    constexpr int lds = 2 * C2Geom<KH, KW, S, U8, NCHW3>::PLANE + 16;
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    return c2_launch_lds(conv2d_split_kernel<KH, KW, S, U8, WM, NTW, NCHW3>, lds, nblk, p, st, "conv2d_split");
}
// the persistent form on a grid of `grid` workgroups; bounded to three waves per SIMD (168 registers) where a chunk's weight
// fragments (8 STEPS registers), the prefetched patch (8 NIT) and the accumulators (64 / WM) fit that without spilling: the
// 3-step chunks of the 3 x 3 layers, and of the stride-2 layers with a 16-channel tile.  (Four and five waves for the 16-channel
// tiles spill 34 - 57 registers.)
template <int KH, int KW, int S, int U8, int WM>
static int c2_launch_persist(const C2Params& p, long long grid, hipStream_t st) {
    using G = C2Geom<KH, KW, S, U8, false>;
    constexpr int WAVES = (G::STEPS == 3 && (G::NIT <= 2 || WM == 4)) ? 3 : 2;
    constexpr int lds = 2 * G::PLANE + 16;
    static_assert(lds <= 48 * 1024, "the persistent form: three workgroups per CU, no LDS attribute");
    return c2_launch_lds(conv2d_split_persist_kernel<KH, KW, S, U8, WM, 1, WAVES>, lds, grid, p, st, "conv2d_split: persistent");
}

// the 3-D march on `grid` (tile, cout block, run) workgroups: two LDS slots (one barrier per chunk), two waves per SIMD, and with a
// single channel chunk (Cin 8) all 27 taps' weight fragments resident
template <int SD, int SLOTS, bool WRES>
static int c3_launch_march_as(const C2Params& p, long long grid, hipStream_t st) {
    constexpr int lds = SLOTS * 2 * C2Geom<3, 3, SD, 1, false>::PLANE + 16;
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    return c2_launch_lds(conv3d_split_march_kernel<SD, 2, SLOTS, WRES>, lds, grid, p, st, "conv3d_split_march");
}
static int c3_launch_march(const C2Shape& s, const C2Params& p, long long grid, hipStream_t st) {
    const bool wres = p.nchunks_c == 1;
#ifdef MVD_EXPERIMENTS  // MVD_C3_SLOTS=1: one LDS slot, two barriers per chunk (measured and not shipped)
    if (const char* e = exp_env("MVD_C3_SLOTS"); e && atoi(e) == 1) {
        if (s.S == 2) return wres ? c3_launch_march_as<2, 1, true>(p, grid, st) : c3_launch_march_as<2, 1, false>(p, grid, st);
        return wres ? c3_launch_march_as<1, 1, true>(p, grid, st) : c3_launch_march_as<1, 1, false>(p, grid, st);
    }
#endif
    if (s.S == 2 && wres) return c3_launch_march_as<2, 2, true>(p, grid, st);
#ifdef MVD_EXPERIMENTS  // the kinds whose entry of C3_MARCH_TD is 0: reachable through MVD_C3_MARCH only
    if (s.S == 2) return c3_launch_march_as<2, 2, false>(p, grid, st);
    return wres ? c3_launch_march_as<1, 2, true>(p, grid, st) : c3_launch_march_as<1, 2, false>(p, grid, st);
#else
    return MVD_ERR_INVALID_ARG;
#endif
}

// tile of output channels per workgroup: bn = 16 WN NTW
template <int KH, int KW, int S, int U8, bool NCHW3>
static int c2_launch_bn(const C2Params& p, int bn, long long nblk, hipStream_t st) {
    switch (bn) {
        case 128: return c2_launch<KH, KW, S, U8, 1, 2, NCHW3>(p, nblk, st);
        case 64: return c2_launch<KH, KW, S, U8, 1, 1, NCHW3>(p, nblk, st);
        case 32: return c2_launch<KH, KW, S, U8, 2, 1, NCHW3>(p, nblk, st);
        case 16: return c2_launch<KH, KW, S, U8, 4, 1, NCHW3>(p, nblk, st);
    }
    return MVD_ERR_INVALID_ARG;
}
template <int KH, int KW, int S, int U8>
static int c2_launch_persist_bn(const C2Params& p, int bn, long long grid, hipStream_t st) {
    switch (bn) {
#ifdef MVD_EXPERIMENTS  // the tiles whose column of C2_PERSIST_WGS is all zeros
        case 64: return c2_launch_persist<KH, KW, S, U8, 1>(p, grid, st);
        case 32: return c2_launch_persist<KH, KW, S, U8, 2>(p, grid, st);
#endif
        case 16: return c2_launch_persist<KH, KW, S, U8, 4>(p, grid, st);
    }
    return MVD_ERR_INVALID_ARG;
}

// persist: the plan's persistent grid (0 = one tile per workgroup, nblk workgroups)
static int c2_dispatch(const C2Shape& s, C2Params& p, int bn, long long nblk, long long persist, hipStream_t st) {
    if (persist > 0 && p.ksplit == 1) {
        p.tiles = (int)nblk;
        switch (c2_persist_kind(s)) {
            case C2_K33: return c2_launch_persist_bn<3, 3, 1, 1>(p, bn, persist, st);
#ifdef MVD_EXPERIMENTS  // the kinds whose row of C2_PERSIST_WGS is all zeros: reachable through MVD_C2_PERSIST only
            case C2_K33W: return c2_launch_persist_bn<3, 3, 1, 4>(p, bn, persist, st);
            case C2_K33S2: return c2_launch_persist_bn<3, 3, 2, 1>(p, bn, persist, st);
            case C2_K55S2: return c2_launch_persist_bn<5, 5, 2, 1>(p, bn, persist, st);
#endif
        }
        return MVD_ERR_INVALID_ARG;
    }
    if (s.nchw3) return c2_launch_bn<7, 7, 2, 1, true>(p, bn, nblk, st);
    if (s.KH == 1) return c2_launch_bn<1, 1, 1, 4, false>(p, bn, nblk, st);
    if (s.KH == 2) return s.U8 == 4 ? c2_launch_bn<2, 2, 1, 4, false>(p, bn, nblk, st) : c2_launch_bn<2, 2, 1, 2, false>(p, bn, nblk, st);
    if (s.KH == 5) return c2_launch_bn<5, 5, 2, 1, false>(p, bn, nblk, st);
    if (s.S == 2) return c2_launch_bn<3, 3, 2, 1, false>(p, bn, nblk, st);
    if (s.U8 == 4) return c2_launch_bn<3, 3, 1, 4, false>(p, bn, nblk, st);
    return c2_launch_bn<3, 3, 1, 1, false>(p, bn, nblk, st);
}

// the tail of both entry points (`what`: the entry's name in messages; p.B, p.Cout, p.nchunks set): the plan's grid goes into the
// parameters, K split only with a workspace for it, the grid limit, the main kernel, and the reduce kernel behind a split
static int c2_run(const char* what, const C2Shape& s, C2Params& p, const C2Plan& q, void* workspace, size_t workspace_bytes, hipStream_t st) {
    p.Ho = q.Ho; p.Wo = q.Wo; p.ncls = q.ncls;
    p.tiles_x = q.tiles_x; p.tiles_y = q.tiles_y; p.nblocks = q.nblocks; p.ncp = q.ncp;
    int ksplit = q.ksplit;
    if (ksplit > 1 && (!workspace || workspace_bytes < q.part_bytes)) ksplit = 1;  // no workspace: the plain grid
    p.ksplit = ksplit;
    p.chunks_per_split = (p.nchunks + ksplit - 1) / ksplit;
    p.part = ksplit > 1 ? static_cast<float*>(workspace) : nullptr;
    const long long nblk = q.tiles * ksplit;
    MVD_REQUIRE(nblk <= 0x7fffffffLL, "%s: %lld workgroups exceed the grid limit", what, nblk);
    if (q.march_td > 0) {  // planned for an unsplit reduction only
        p.march_td = q.march_td;
        p.march_runs = (p.Do + q.march_td - 1) / q.march_td;
        return c3_launch_march(s, p, c3_march_wgs(q, p.B / p.Do, p.Do, q.march_td), st);
    }
    int rc = c2_dispatch(s, p, q.bn, nblk, q.persist, st);
    if (rc != MVD_OK || ksplit == 1) return rc;
    const long long n = (long long)p.B * p.Ho * p.Wo * ((p.Cout + 3) / 4);
    MVD_REQUIRE(n < 0x7fffffffLL, "%s: split reduction over %lld outputs", what, n);
    hipLaunchKernelGGL(c2_reduce_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 1024), (unsigned)p.ncls), dim3(256), 0, st, p);
    return launch_status((std::string(what) + ": reduce").c_str());
}

}  // namespace mvd

extern "C" {

size_t mvd_conv2d_split_packed_weight_bytes(int Cin_pad, int Cout, int KH, int KW, int stride, int mode) {
    mvd::C2Shape s;
    if (Cin_pad <= 0 || Cout <= 0 || !mvd::c2_shape(KH, KW, stride, mode, Cin_pad, &s)) return 0;
    return mvd::c2_frag_bytes(s, Cin_pad, Cout) + (size_t)mvd::c2_cpad(Cout) * sizeof(float);
}

int mvd_pack_conv2d_weights_split(const float* w, int Cin, int Cin_pad, int Cout, int KH, int KW, int stride, int mode, void* packed,
                                  mvd_stream_t stream) {
    MVD_REQUIRE(w && packed, "pack_conv2d_weights_split: NULL argument");
    mvd::C2Shape s;
    MVD_REQUIRE(Cin > 0 && Cin <= Cin_pad && Cout > 0 && mvd::c2_shape(KH, KW, stride, mode, Cin_pad, &s),
                "pack_conv2d_weights_split: layer %dx%d stride %d mode %d with %d (padded %d) -> %d channels is not built", KH, KW, stride, mode,
                Cin, Cin_pad, Cout);
    hipStream_t st = (hipStream_t)stream;
    const size_t fb = mvd::c2_frag_bytes(s, Cin_pad, Cout);
    float* eun = reinterpret_cast<float*>(static_cast<char*>(packed) + fb);
    mvd::split_wscale_launch(w, eun, Cin, Cout, KH * KW, s.transposed, Cout, mvd::c2_cpad(Cout), st);
    const long long total = (long long)(fb / 2);
    hipLaunchKernelGGL(mvd::c2_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, eun, (_Float16*)packed, Cin, Cout, s.KH,
                       s.KW, s.U8, Cin_pad / (8 * s.U8), mvd::c2_ntiles(Cout), s.steps, s.transposed ? 1 : s.nchw3 ? 2 : 0, total);
    return mvd::launch_status("pack_conv2d_weights_split");
}

size_t mvd_conv2d_split_workspace_bytes(int B, int Hi, int Wi, int Cin_pad, int Cout, int KH, int KW, int stride, int mode) {
    mvd::C2Shape s;
    if (B <= 0 || Hi <= 0 || Wi <= 0 || Cin_pad <= 0 || Cout <= 0 || !mvd::c2_shape(KH, KW, stride, mode, Cin_pad, &s)) return 0;
    return mvd::c2_plan(s, B, Hi, Wi, Cin_pad, Cin_pad, Cout, KH, KW, stride).part_bytes;
}

int mvd_conv2d_split_f32(const float* x, const float* x_absmax, const void* packed_w, const float* bias, float* y, float* y_absmax, int B,
                         int Hi, int Wi, int Cin_pad, int x_pixel_stride, int Cout, int y_pixel_stride, long long y_row_stride,
                         long long y_image_stride, long long y_channel_stride, int KH, int KW, int stride, int mode, int act, float slope,
                         void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    MVD_REQUIRE(x && x_absmax && packed_w && y, "conv2d_split: NULL argument");
    MVD_REQUIRE(B > 0 && Hi > 0 && Wi > 0, "conv2d_split: non-positive dimension");
    mvd::C2Shape s;
    MVD_REQUIRE(Cin_pad > 0 && Cout > 0 && mvd::c2_shape(KH, KW, stride, mode, Cin_pad, &s),
                "conv2d_split: layer %dx%d stride %d mode %d with %d -> %d channels is not built", KH, KW, stride, mode, Cin_pad, Cout);
    MVD_REQUIRE(mode == 2 || (x_pixel_stride >= Cin_pad && x_pixel_stride % 4 == 0), "conv2d_split: input pixel stride %d (channels %d)",
                x_pixel_stride, Cin_pad);
    if (y_channel_stride <= 0) y_channel_stride = 1;
    MVD_REQUIRE(y_channel_stride != 1 || y_pixel_stride >= Cout, "conv2d_split: output pixel stride %d below %d channels", y_pixel_stride, Cout);
    MVD_REQUIRE(y_pixel_stride >= 1 && y_row_stride >= 0 && y_image_stride >= 0, "conv2d_split: negative output stride");
    MVD_REQUIRE(act >= 0 && act <= 2, "conv2d_split: act=%d unknown", act);
    MVD_REQUIRE(mode == 2 || (((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0), "conv2d_split: x and y must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    mvd::C2Params p{};
    p.x = x; p.xamax = x_absmax; p.bias = bias; p.y = y; p.yamax = y_absmax;
    p.B = B; p.Hi = Hi; p.Wi = Wi; p.xs = x_pixel_stride; p.nchunks = Cin_pad / (8 * s.U8);
    p.Di = p.Do = p.Dy = p.KD = p.SD = 1; p.pad_d = 0; p.nchunks_c = p.nchunks; p.sub3d = 0; p.Cr = Cout;
    p.Cout = Cout; p.ys = y_pixel_stride; p.act = act; p.slope = slope;
    const size_t fb = mvd::c2_frag_bytes(s, Cin_pad, Cout);
    p.eun = reinterpret_cast<const float*>(static_cast<const char*>(packed_w) + fb);
    const mvd::C2Plan q = mvd::c2_plan(s, B, Hi, Wi, Cin_pad, x_pixel_stride, Cout, KH, KW, stride);
    if (s.transposed) {
        p.Hy = 2 * Hi; p.Wy = 2 * Wi; p.oy_mul = p.ox_mul = 2; p.pad_y = p.pad_x = 1;
    } else {
        p.Hy = q.Ho; p.Wy = q.Wo; p.oy_mul = p.ox_mul = 1; p.pad_y = KH / 2; p.pad_x = KW / 2;
    }
    MVD_REQUIRE(y_channel_stride != 1 || Cout < 4 || (y_pixel_stride % 4 == 0 && y_row_stride % 4 == 0 && y_image_stride % 4 == 0),
                "conv2d_split: channel-last output strides must be multiples of 4 floats");
    p.ycs = y_channel_stride;
    p.ys_row = y_row_stride > 0 ? y_row_stride : (long long)p.Wy * y_pixel_stride;
    p.ys_img = y_image_stride > 0 ? y_image_stride : (long long)p.Hy * p.ys_row;
    p.wpk = static_cast<const char*>(packed_w);
    p.cls_bytes = (long long)(fb / q.ncls);
    return mvd::c2_run("conv2d_split", s, p, q, workspace, workspace_bytes, st);
}

int mvd_upsample2x_nhwc_f32(const float* x, float* y, float* y_absmax, int B, int C, int h, int w, int y_pixel_stride, mvd_stream_t stream) {
    MVD_REQUIRE(x && y, "upsample2x_nhwc: NULL argument");
    MVD_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0 && y_pixel_stride >= C, "upsample2x_nhwc: bad dimension");
    const long long n = (long long)B * 4 * h * w;
    hipLaunchKernelGGL(mvd::upsample2x_nhwc_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 1024)), dim3(256), 0, (hipStream_t)stream, x, y,
                       y_absmax, B, C, h, w, y_pixel_stride);
    return mvd::launch_status("upsample2x_nhwc");
}

/* ---- 3-D layers ---- */
}  // extern "C"

namespace mvd {
// mode: MVD_CONV3D_STRIDE1 / MVD_CONV3D_STRIDE2 / MVD_DECONV3D_STRIDE2 (mvd.h)
static bool c3_shape(int Cin, int Cout, int mode, C2Shape* s, int* ncout) {
    if (Cin <= 0 || Cin % 8 || Cout <= 0 || Cout % 4 || mode < 0 || mode > 2) return false;
    s->transposed = false; s->nchw3 = false;
    if (mode == MVD_DECONV3D_STRIDE2) {
        if (Cin % 16) return false;
        s->KH = s->KW = 2; s->S = 1; s->U8 = Cin % 32 == 0 ? 4 : 2;
        *ncout = 8 * Cout;
    } else {
        s->KH = s->KW = 3; s->S = mode == MVD_CONV3D_STRIDE2 ? 2 : 1;
        s->U8 = (s->S == 1 && Cin % 32 == 0) ? 4 : 1;
        *ncout = Cout;
    }
    s->steps = (s->KH * s->KW * s->U8 + 3) / 4;
    return true;
}
static size_t c3_frag_bytes(const C2Shape& s, int Cin, int ncout, int mode) {
    const size_t KD = mode == MVD_DECONV3D_STRIDE2 ? 2 : 3;
    return (size_t)c2_ntiles(ncout) * KD * (Cin / (8 * s.U8)) * s.steps * 2048;
}
}  // namespace mvd

extern "C" {

size_t mvd_conv3d_igemm_packed_weight_bytes(int Cin, int Cout, int mode) {
    mvd::C2Shape s;
    int ncout;
    if (!mvd::c3_shape(Cin, Cout, mode, &s, &ncout)) return 0;
    return mvd::c3_frag_bytes(s, Cin, ncout, mode) + (size_t)mvd::c2_cpad(ncout) * sizeof(float);
}

int mvd_pack_conv3d_weights_igemm(const float* w, int Cin, int Cout, int mode, void* packed, mvd_stream_t stream) {
    MVD_REQUIRE(w && packed, "pack_conv3d_weights_igemm: NULL argument");
    mvd::C2Shape s;
    int ncout;
    MVD_REQUIRE(mvd::c3_shape(Cin, Cout, mode, &s, &ncout), "pack_conv3d_weights_igemm: %d -> %d channels, mode %d is not built", Cin, Cout, mode);
    hipStream_t st = (hipStream_t)stream;
    const size_t fb = mvd::c3_frag_bytes(s, Cin, ncout, mode);
    float* eun = reinterpret_cast<float*>(static_cast<char*>(packed) + fb);
    const int tr = mode == MVD_DECONV3D_STRIDE2 ? 1 : 0;
    // 2^k_c per (class, channel) row: max |w| over all of the channel's weights, shared by the 8 classes of the transposed form
    mvd::split_wscale_launch(w, eun, Cin, Cout, 27, tr != 0, ncout, mvd::c2_cpad(ncout), st);
    const long long total = (long long)(fb / 2);
    hipLaunchKernelGGL(mvd::c3_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, eun, (_Float16*)packed, Cin, Cout, s.U8,
                       Cin / (8 * s.U8), mvd::c2_ntiles(ncout), s.steps, tr, total);
    return mvd::launch_status("pack_conv3d_weights_igemm");
}

static mvd::C2Plan c3_plan(const mvd::C2Shape& s, int B, int Di, int Hi, int Wi, int Cin, int ncout, int mode, int* Do) {
    mvd::C2Plan q{};
    const int sd = mode == MVD_CONV3D_STRIDE2 ? 2 : 1;
    *Do = Di / sd; q.ncls = 1;
    int bn = mvd::c2_bn(ncout);  // the packing rule's tile: any narrower one reads the same 16-channel fragments
    mvd::c2_plan_tiles(q, Hi / sd, Wi / sd, (long long)B * *Do, ncout, bn);
    const long long planes = q.tiles / q.nblocks;
    // a stride-1 level with too many tiles for a split of K (128+) and fewer than two per CU (conv6 of a 256-plane volume: 192):
    // narrower channel tiles, more workgroups, each with a shorter chain of MFMAs per staged chunk (conv6 45 -> 43 us in the frame
    // on 16 channels; the stride-2 layers are slower that way).  Smaller grids keep their tile and split K as before.
    if (mode == MVD_CONV3D_STRIDE1 && !mvd::exp_env("MVD_C2_BN") && q.tiles >= 128)
        while (bn > 16 && planes * ((ncout + bn - 1) / bn) < 512) bn /= 2;
    if (mode != MVD_DECONV3D_STRIDE2 && s.U8 == 1 && mvd::c3_march_forced() > 1) bn = 16;  // experiments library: the march's tile
    if (bn != q.bn) mvd::c2_plan_tiles(q, q.Ho, q.Wo, (long long)B * *Do, ncout, bn);
    q.nchunks = (mode == MVD_DECONV3D_STRIDE2 ? 2 : 3) * (Cin / (8 * s.U8));
    mvd::c2_plan_finish(s, q, B * *Do, Hi, Wi, Cin);
    q.march_td = mode == MVD_DECONV3D_STRIDE2 ? 0 : mvd::c3_march_td(s, q, B, *Do, Hi, Wi, Cin);
    return q;
}

size_t mvd_conv3d_igemm_workspace_bytes(int B, int Di, int Hi, int Wi, int Cin, int Cout, int mode) {
    mvd::C2Shape s;
    int ncout, Do;
    if (B <= 0 || Di <= 0 || Hi <= 0 || Wi <= 0 || !mvd::c3_shape(Cin, Cout, mode, &s, &ncout)) return 0;
    return c3_plan(s, B, Di, Hi, Wi, Cin, ncout, mode, &Do).part_bytes;
}

int mvd_conv3d_bn_relu_igemm_f32(const float* x, const float* x_absmax, const void* packed_w, const float* scale, const float* shift,
                                 const float* skip, float* y, float* y_absmax, int B, int Di, int Hi, int Wi, int Cin, int Cout, int mode,
                                 int relu, void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    MVD_REQUIRE(x && x_absmax && packed_w && scale && shift && y, "conv3d_igemm: NULL argument");
    MVD_REQUIRE(B > 0 && Di > 0 && Hi > 0 && Wi > 0, "conv3d_igemm: non-positive dimension");
    mvd::C2Shape s;
    int ncout;
    MVD_REQUIRE(mvd::c3_shape(Cin, Cout, mode, &s, &ncout), "conv3d_igemm: %d -> %d channels, mode %d is not built", Cin, Cout, mode);
    MVD_REQUIRE(mode != MVD_CONV3D_STRIDE2 || (Di % 2 == 0 && Hi % 2 == 0 && Wi % 2 == 0), "conv3d_igemm stride 2: odd input dims %dx%dx%d", Di, Hi, Wi);
    MVD_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)skip) & 15) == 0, "conv3d_igemm: x, y and skip must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int Do;
    const mvd::C2Plan q = c3_plan(s, B, Di, Hi, Wi, Cin, ncout, mode, &Do);
    const bool tr = mode == MVD_DECONV3D_STRIDE2;
    mvd::C2Params p{};
    p.x = x; p.xamax = x_absmax; p.bias = shift; p.scale = scale; p.skip = skip; p.y = y; p.yamax = y_absmax;
    p.wpk = static_cast<const char*>(packed_w);
    p.eun = reinterpret_cast<const float*>(p.wpk + mvd::c3_frag_bytes(s, Cin, ncout, mode));
    p.B = B * Do; p.Hi = Hi; p.Wi = Wi; p.xs = Cin; p.nchunks = q.nchunks;
    p.Di = Di; p.Do = Do; p.KD = tr ? 2 : 3; p.SD = mode == MVD_CONV3D_STRIDE2 ? 2 : 1; p.pad_d = tr ? 0 : 1; p.nchunks_c = Cin / (8 * s.U8);
    p.sub3d = tr ? 1 : 0; p.Cr = Cout; p.Dy = tr ? 2 * Di : Do;
    p.Hy = tr ? 2 * Hi : q.Ho; p.Wy = tr ? 2 * Wi : q.Wo;
    p.oy_mul = p.ox_mul = 1; p.pad_y = p.pad_x = tr ? 0 : 1;
    p.Cout = ncout; p.ys = Cout; p.ycs = 1;
    p.ys_row = (long long)p.Wy * Cout; p.ys_img = (long long)p.Hy * p.ys_row;
    p.cls_bytes = 0;
    p.act = relu ? 2 : 0; p.slope = 0.f;
    MVD_REQUIRE(q.nblocks * (q.bn / 16) <= mvd::c2_ntiles(ncout), "conv3d_igemm: channel tile %d reads past the %d packed fragments", q.bn,
                mvd::c2_ntiles(ncout));
    return mvd::c2_run("conv3d_igemm", s, p, q, workspace, workspace_bytes, st);
}
}
