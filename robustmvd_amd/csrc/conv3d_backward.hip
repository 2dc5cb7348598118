// Backward of one CostRegNet layer (rmvd/models/blocks/mvsnet_components.py:25-41,69-123 under autograd, driven by
// rmvd/train/multi_view_depth_training.py:231-246) — the parts the forward kernels of conv3d.hip do not already cover:
//
//   1. the WEIGHT gradient of a 3x3x3 Conv3d (stride 1 / 2, padding 1) or ConvTranspose3d (stride 2, padding 1,
//      output_padding 1) on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation);
//   2. a stride-1 convolution with ONE input channel (the adjoint of `prob`, 1 -> 8), which conv3d.hip's implicit GEMM
//      has no instantiation for: a vector-ALU kernel, one thread per (voxel, 4 output channels).
//   (The data gradients of the other ten layers are forward layers with adjoint weights: ops.conv3d_adjoint.)
//
// Weight gradient.  All three modes are ONE reduction.  With a "small" tensor s (B,Ds,hs,ws,Cs) and a "big" tensor g
// (B,Dg,hg,wg,Cg), Dg = S*Ds ..., S in {1,2}:
//       gw[cs][cg][k] = sum_{b,o} s[b,o,cs] * gpad[b, S*o + k, cg]          (gpad = g zero-padded by 1, k = (kd,kh,kw))
//   Conv3d          : s = gy, g = x   -> gw is (Cout,Cin,3,3,3), the layer's own layout;
//   ConvTranspose3d : s = x,  g = gy  -> gw is (Cin,Cout,3,3,3), the layer's own layout again.
// Per tap it is a GEMM with a tiny output (Cs x Cg) and a huge reduction (the voxels):
//       D[cs, cg] += A[cs, voxel] * B[voxel, cg],   A = s (M = 16 channels, K = 4 voxels), B = g shifted by the tap.
//
// Tiling.  A workgroup (4 waves) owns a TH x TW tile of the small tensor's (h,w) grid and marches over DZ of its depth
// planes.  LDS holds a ring of three planes of g (tile + halo, ROWS x COLS pixels) and the current plane of s; a march step
// loads S new planes of g and one of s, so every plane of g is staged once per tile column (not once per depth tap).  The
// K dimension of an MFMA is 4 voxels that are neighbours along w.  The 27 taps are divided among the 4 waves (7,7,7,6):
// each wave keeps (Cs/16) x (Cg/16) accumulator tiles per tap in registers (32 x 32 channels: 16 VGPRs per tap) and reads
// the s fragment once per voxel group for all its taps.  Channel counts are zero-padded to multiples of 16 in LDS; more
// than 32 channels on a side are split over blockIdx.y in blocks of 32.
// LDS pixel strides are chosen so that the two voxels a 32-lane half of ds_read_b32 touches sit 16 banks apart.
//
// Deterministic: no atomics.  A workgroup walks the tiles item = blockIdx.x, blockIdx.x + gridDim.x, ... in that order, keeps
// summing into its registers and writes ONE partial gradient to the workspace; a second kernel adds the partials of all
// workgroups in index order.  Grid size and item order depend on the tensor sizes only.
#include "mvd_common.h"

namespace mvd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WG_TH = 4;
constexpr int WG_TAPS = 7;            // taps per wave: 27 over 4 waves
constexpr int WG_MAX_PARTIALS = 512;  // workgroups along x: two per CU

struct WGradParams {
    const float* sm;  // (B,Ds,hs,ws,Cs)
    const float* bg;  // (B,Dg,hg,wg,Cg)
    float* partial;   // [gridDim.y][gridDim.x][27][CSB][CGB]
    int B, Ds, hs, ws, Cs, Dg, hg, wg, Cg;
    int tiles_h, tiles_w, dchunks, DZ, items;
    int cg_blocks;
};

template <int COT, int CIT, int S>
struct WGradGeom {
    static constexpr int TW = S == 1 ? 16 : 8;
    static constexpr int ROWS = S * (WG_TH - 1) + 3, COLS = S * (TW - 1) + 3;
    static constexpr int CSB = 16 * COT, CGB = 16 * CIT;
    // ds_read_b32 banks: (a/4) % 32 within a 32-lane half = 2 voxels x 16 channels: voxel stride S*PSTR = 16 (mod 32)
    static constexpr int PSTR = S == 1 ? (CIT == 1 ? 16 : 48) : (CIT == 1 ? 24 : 40);
    static constexpr int SSTR = COT == 1 ? 16 : 48;
    static constexpr int PLANE = ROWS * COLS * PSTR;
    static constexpr size_t LDS_BYTES = (size_t)(3 * PLANE + WG_TH * TW * SSTR) * sizeof(float);
};

// pixel `px` (or zeros if null) of a channel-last tensor with C channels, channels c0 .. c0+CB-1, into LDS as float4s
template <int CB>
__device__ __forceinline__ void stage_pixel(const float* __restrict__ px, int C, int c0, int c4, float* __restrict__ dst) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int c = c0 + 4 * c4;
    if (px && c < C) {
        if ((C & 3) == 0) {
            v = *reinterpret_cast<const float4*>(px + c);
        } else {
            v.x = px[c];
            if (c + 1 < C) v.y = px[c + 1];
            if (c + 2 < C) v.z = px[c + 2];
            if (c + 3 < C) v.w = px[c + 3];
        }
    }
    *reinterpret_cast<float4*>(dst + 4 * c4) = v;
}

template <int COT, int CIT, int S>
__global__ void __launch_bounds__(256) conv3d_weight_grad_kernel(WGradParams p) {
    using G = WGradGeom<COT, CIT, S>;
    constexpr int TH = WG_TH, TW = G::TW, ROWS = G::ROWS, COLS = G::COLS, PSTR = G::PSTR, SSTR = G::SSTR, PLANE = G::PLANE;
    constexpr int CSB = G::CSB, CGB = G::CGB;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* __restrict__ gl = lds;               // [3][ROWS][COLS][PSTR]
    float* __restrict__ sl = lds + 3 * PLANE;   // [TH][TW][SSTR]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, k = lane >> 4;
    const int cs0 = ((int)blockIdx.y / p.cg_blocks) * CSB, cg0 = ((int)blockIdx.y % p.cg_blocks) * CGB;

    f32x4 acc[WG_TAPS][COT][CIT];
#pragma unroll
    for (int t = 0; t < WG_TAPS; ++t)
#pragma unroll
        for (int a = 0; a < COT; ++a)
#pragma unroll
            for (int b = 0; b < CIT; ++b) acc[t][a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int item = blockIdx.x; item < p.items; item += gridDim.x) {
        int r = item;
        const int tw = r % p.tiles_w; r /= p.tiles_w;
        const int th = r % p.tiles_h; r /= p.tiles_h;
        const int dc = r % p.dchunks;
        const int b = r / p.dchunks;
        const int r0 = th * TH, c0 = tw * TW;
        const int d0 = dc * p.DZ, d1 = min(d0 + p.DZ, p.Ds);
        const float* __restrict__ bgb = p.bg + (size_t)b * p.Dg * p.hg * p.wg * p.Cg;
        const float* __restrict__ smb = p.sm + (size_t)b * p.Ds * p.hs * p.ws * p.Cs;
        int next_plane = S * d0 - 1;  // first plane of g not yet in the ring (ring slot of plane q: (q + 1) % 3)

        for (int d = d0; d < d1; ++d) {
            __syncthreads();  // the previous step's reads are done
            for (; next_plane <= S * d + 1; ++next_plane) {
                const bool pok = next_plane >= 0 && next_plane < p.Dg;  // block-uniform
                float* __restrict__ dstp = gl + ((next_plane + 1) % 3) * PLANE;
                const float* __restrict__ srcp = bgb + (size_t)(pok ? next_plane : 0) * p.hg * p.wg * p.Cg;
                for (int e = tid; e < ROWS * COLS * (CGB / 4); e += 256) {
                    const int px = e / (CGB / 4), c4 = e - px * (CGB / 4);
                    const int row = px / COLS, col = px - row * COLS;
                    const int gr = S * r0 - 1 + row, gc = S * c0 - 1 + col;
                    const bool ok = pok && gr >= 0 && gr < p.hg && gc >= 0 && gc < p.wg;
                    stage_pixel<CGB>(ok ? srcp + ((size_t)gr * p.wg + gc) * p.Cg : nullptr, p.Cg, cg0, c4, dstp + px * PSTR);
                }
            }
            {
                const float* __restrict__ srcp = smb + (size_t)d * p.hs * p.ws * p.Cs;
                for (int e = tid; e < TH * TW * (CSB / 4); e += 256) {
                    const int px = e / (CSB / 4), c4 = e - px * (CSB / 4);
                    const int row = px / TW, col = px - row * TW;
                    const int gr = r0 + row, gc = c0 + col;
                    const bool ok = gr < p.hs && gc < p.ws;
                    stage_pixel<CSB>(ok ? srcp + ((size_t)gr * p.ws + gc) * p.Cs : nullptr, p.Cs, cs0, c4, sl + px * SSTR);
                }
            }
            __syncthreads();

            int toff[WG_TAPS];
#pragma unroll
            for (int t = 0; t < WG_TAPS; ++t) {
                const int tap = min(wave + 4 * t, 26);
                const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
                toff[t] = ((S * d + kd) % 3) * PLANE + (kh * COLS + kw) * PSTR + j;
            }
            for (int row = 0; row < TH; ++row) {
#pragma unroll
                for (int c4 = 0; c4 < TW / 4; ++c4) {
                    const int col = c4 * 4 + k;
                    float af[COT];
#pragma unroll
                    for (int a = 0; a < COT; ++a) af[a] = sl[(row * TW + col) * SSTR + a * 16 + j];
                    const int base = (S * row * COLS + S * col) * PSTR;
#pragma unroll
                    for (int t = 0; t < WG_TAPS; ++t) {
                        if (wave + 4 * t < 27) {  // wave-uniform
                            float bf[CIT];
#pragma unroll
                            for (int bq = 0; bq < CIT; ++bq) bf[bq] = gl[toff[t] + base + bq * 16];
#pragma unroll
                            for (int a = 0; a < COT; ++a)
#pragma unroll
                                for (int bq = 0; bq < CIT; ++bq)
                                    acc[t][a][bq] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[a], bf[bq], acc[t][a][bq], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }

    // the workgroup's partial gradient: lane holds rows 4k .. 4k+3 (small-tensor channels) of column j (big-tensor channel)
    float* __restrict__ out = p.partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 27 * CSB * CGB;
#pragma unroll
    for (int t = 0; t < WG_TAPS; ++t) {
        const int tap = wave + 4 * t;
        if (tap < 27) {
#pragma unroll
            for (int a = 0; a < COT; ++a)
#pragma unroll
                for (int bq = 0; bq < CIT; ++bq)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        out[((size_t)tap * CSB + a * 16 + 4 * k + i) * CGB + bq * 16 + j] = acc[t][a][bq][i];
        }
    }
}

// gw[cs][cg][tap] = sum over the workgroups' partials, in index order (a fixed order: bit-identical from run to run)
__global__ void __launch_bounds__(256) conv3d_weight_grad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ gw, int P,
                                                                         int Cs, int Cg, int CSB, int CGB, int cg_blocks, int nby) {
    const int per = 27 * CSB * CGB;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nby * per) return;
    const int by = e / per, f = e - by * per;
    const int cgl = f % CGB, csl = (f / CGB) % CSB, tap = f / (CGB * CSB);
    const int cs = (by / cg_blocks) * CSB + csl, cg = (by % cg_blocks) * CGB + cgl;
    if (cs >= Cs || cg >= Cg) return;
    const float* __restrict__ src = partial + (size_t)by * P * per + f;
    float sum = 0.f;
#pragma unroll 16
    for (int q = 0; q < P; ++q) sum += src[(size_t)q * per];
    gw[((size_t)cs * Cg + cg) * 27 + tap] = sum;
}

struct WGradPlan {
    WGradParams p;
    int S, COT, CIT, cs_blocks, P;
    size_t bytes;
};

// fills the plan; returns nullptr or the reason the arguments are unsupported
static const char* wgrad_plan(int B, int Di, int hi, int wi, int Cin, int Cout, int mode, WGradPlan& pl) {
    if (B <= 0 || Di <= 0 || hi <= 0 || wi <= 0) return "non-positive dimension";
    if (Cin < 1 || Cin > 64 || Cout < 1 || Cout > 64) return "Cin and Cout must be in 1..64";
    WGradParams& p = pl.p;
    p = WGradParams{};
    p.B = B;
    if (mode == MVD_CONV3D_STRIDE1 || mode == MVD_CONV3D_STRIDE2) {
        pl.S = mode == MVD_CONV3D_STRIDE1 ? 1 : 2;
        if (pl.S == 2 && (Di % 2 || hi % 2 || wi % 2)) return "stride 2 needs even input dims";
        p.Ds = Di / pl.S; p.hs = hi / pl.S; p.ws = wi / pl.S; p.Cs = Cout;
        p.Dg = Di; p.hg = hi; p.wg = wi; p.Cg = Cin;
    } else if (mode == MVD_DECONV3D_STRIDE2) {
        if (Di > 0x3fffffff || hi > 0x3fffffff || wi > 0x3fffffff) return "dimension too large";
        pl.S = 2;
        p.Ds = Di; p.hs = hi; p.ws = wi; p.Cs = Cin;
        p.Dg = 2 * Di; p.hg = 2 * hi; p.wg = 2 * wi; p.Cg = Cout;
    } else {
        return "unknown mode";
    }
    if ((long long)p.hg * p.wg * p.Cg > 0x7fffffffLL) return "plane too large";
    const int csp = (p.Cs + 15) / 16, cgp = (p.Cg + 15) / 16;  // 16-channel tiles
    pl.COT = csp > 1 ? 2 : 1; pl.cs_blocks = (csp + 1) / 2;
    pl.CIT = cgp > 1 ? 2 : 1; p.cg_blocks = (cgp + 1) / 2;
    const int TW = pl.S == 1 ? 16 : 8;
    p.tiles_h = (p.hs + WG_TH - 1) / WG_TH;
    p.tiles_w = (p.ws + TW - 1) / TW;
    const long long tiles = (long long)B * p.tiles_h * p.tiles_w;
    p.DZ = 8;  // shorter marches when the volume would otherwise leave compute units idle
    while (p.DZ > 1 && tiles * ((p.Ds + p.DZ - 1) / p.DZ) < WG_MAX_PARTIALS) p.DZ /= 2;
    p.dchunks = (p.Ds + p.DZ - 1) / p.DZ;
    const long long items = tiles * p.dchunks;
    if (items > 0x7fffffffLL) return "volume too large";
    p.items = (int)items;
    pl.P = (int)(items < WG_MAX_PARTIALS ? items : WG_MAX_PARTIALS);
    pl.bytes = align_up((size_t)pl.cs_blocks * p.cg_blocks * pl.P * 27 * (16 * pl.COT) * (16 * pl.CIT) * sizeof(float), 256);
    return nullptr;
}

template <int COT, int CIT, int S>
static int launch_wgrad(const WGradPlan& pl, hipStream_t st) {
    using G = WGradGeom<COT, CIT, S>;
    static_assert(G::LDS_BYTES <= 160 * 1024, "weight-gradient tiles exceed LDS");
    auto kern = conv3d_weight_grad_kernel<COT, CIT, S>;
    if (G::LDS_BYTES > 64 * 1024 &&
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES) != hipSuccess)
        return launch_status("conv3d_weight_grad: LDS attribute");
    hipLaunchKernelGGL(kern, dim3((unsigned)pl.P, (unsigned)(pl.cs_blocks * pl.p.cg_blocks)), dim3(256), G::LDS_BYTES, st, pl.p);
    return launch_status("conv3d_weight_grad");
}

// ---------------------------------------------------------------------------------------------------------------
// Stride-1 3x3x3 convolution with ONE input channel (the adjoint of `prob`): x (B,D,h,w) -> y (B,D,h,w,Cout), Cout a multiple
// of 4.  Thread = (voxel, 4 output channels); the 27 neighbours come from L1/L2 (the volume has one float per voxel), the
// weights [tap][Cout] from the scalar/vector cache.  Same epilogue as conv3d.hip: y = relu?(acc * scale + shift) (+ skip).
__global__ void __launch_bounds__(256) conv3d_c1_kernel(const float* __restrict__ x, const float* __restrict__ wpk,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        const float* __restrict__ skip, float* __restrict__ y, int B, int D, int h, int w,
                                                        int Cout, int relu) {
    const int Q = Cout / 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)B * D * h * w * Q) return;
    const int q = (int)(t % Q);
    long long v = t / Q;
    const int xx = (int)(v % w); v /= w;
    const int yy = (int)(v % h); v /= h;
    const int zz = (int)(v % D);
    const int b = (int)(v / D);
    const float* __restrict__ xb = x + (size_t)b * D * h * w;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kd = 0; kd < 3; ++kd)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int z = zz + kd - 1, r = yy + kh - 1, c = xx + kw - 1;
                const bool ok = z >= 0 && z < D && r >= 0 && r < h && c >= 0 && c < w;
                const float xv = ok ? xb[((size_t)z * h + r) * w + c] : 0.f;
                const float4 wv = *reinterpret_cast<const float4*>(wpk + ((kd * 3 + kh) * 3 + kw) * Cout + 4 * q);
                acc.x = fmaf(xv, wv.x, acc.x); acc.y = fmaf(xv, wv.y, acc.y);
                acc.z = fmaf(xv, wv.z, acc.z); acc.w = fmaf(xv, wv.w, acc.w);
            }
    const float4 sc = *reinterpret_cast<const float4*>(scale + 4 * q), sh = *reinterpret_cast<const float4*>(shift + 4 * q);
    float4 o = make_float4(fmaf(acc.x, sc.x, sh.x), fmaf(acc.y, sc.y, sh.y), fmaf(acc.z, sc.z, sh.z), fmaf(acc.w, sc.w, sh.w));
    if (relu) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
    const size_t oi = (size_t)(t / Q) * Cout + 4 * q;
    if (skip) {
        const float4 s = *reinterpret_cast<const float4*>(skip + oi);
        o.x += s.x; o.y += s.y; o.z += s.z; o.w += s.w;
    }
    *reinterpret_cast<float4*>(y + oi) = o;
}

__global__ void pack_c1_kernel(const float* __restrict__ w, float* __restrict__ packed, int Cout) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;  // packed [tap][cout] <- w (Cout, 1, 27)
    if (e < 27 * Cout) packed[e] = w[(e % Cout) * 27 + e / Cout];
}

bool conv3d_c1_ok(int Cout) { return Cout >= 4 && Cout <= 64 && Cout % 4 == 0; }

int conv3d_c1_pack(const float* w, int Cout, float* packed, hipStream_t st) {
    hipLaunchKernelGGL(pack_c1_kernel, dim3((unsigned)((27 * Cout + 255) / 256)), dim3(256), 0, st, w, packed, Cout);
    return launch_status("pack_conv3d_weights");
}

int conv3d_c1_launch(const float* x, const float* packed_w, const float* scale, const float* shift, const float* skip, float* y, int B,
                     int D, int h, int w, int Cout, int relu, hipStream_t st) {
    const long long nblk = ((long long)B * D * h * w * (Cout / 4) + 255) / 256;
    if (nblk > 0x7fffffffLL) {
        set_error("conv3d: %lld workgroups exceed the grid limit", nblk);
        return MVD_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(conv3d_c1_kernel, dim3((unsigned)nblk), dim3(256), 0, st, x, packed_w, scale, shift, skip, y, B, D, h, w, Cout, relu);
    return launch_status("conv3d_c1");
}

}  // namespace mvd

extern "C" {

size_t mvd_conv3d_weight_grad_workspace_bytes(int B, int Di, int hi, int wi, int Cin, int Cout, int mode) {
    mvd::WGradPlan pl;
    return mvd::wgrad_plan(B, Di, hi, wi, Cin, Cout, mode, pl) ? 0 : pl.bytes;
}

size_t mvd_conv3d_weight_grad_plan_field(int B, int Di, int hi, int wi, int Cin, int Cout, int mode, int field) {
    mvd::WGradPlan pl;
    if (mvd::wgrad_plan(B, Di, hi, wi, Cin, Cout, mode, pl)) return 0;
    switch (field) {
        case MVD_WGRAD_PLAN_DZ: return (size_t)pl.p.DZ;
        case MVD_WGRAD_PLAN_ITEMS: return (size_t)pl.p.items;
        case MVD_WGRAD_PLAN_PARTIALS: return (size_t)pl.P;
        case MVD_WGRAD_PLAN_COT: return (size_t)pl.COT;
        case MVD_WGRAD_PLAN_CIT: return (size_t)pl.CIT;
        case MVD_WGRAD_PLAN_S: return (size_t)pl.S;
        case MVD_WGRAD_PLAN_CS_BLOCKS: return (size_t)pl.cs_blocks;
        case MVD_WGRAD_PLAN_CG_BLOCKS: return (size_t)pl.p.cg_blocks;
        default: return 0;
    }
}

int mvd_conv3d_weight_grad_f32(const float* x, const float* gy, float* gw, int B, int Di, int hi, int wi, int Cin, int Cout, int mode,
                               void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(x && gy && gw, "conv3d_weight_grad: NULL argument");
    WGradPlan pl;
    const char* why = wgrad_plan(B, Di, hi, wi, Cin, Cout, mode, pl);
    MVD_REQUIRE(!why, "conv3d_weight_grad: %s (B=%d, %dx%dx%d, Cin=%d, Cout=%d, mode=%d)", why, B, Di, hi, wi, Cin, Cout, mode);
    if (!workspace || workspace_bytes < pl.bytes) {
        set_error("conv3d_weight_grad: workspace %zu B < required %zu B", workspace_bytes, pl.bytes);
        return MVD_ERR_WORKSPACE;
    }
    const bool deconv = mode == MVD_DECONV3D_STRIDE2;
    pl.p.sm = deconv ? x : gy;
    pl.p.bg = deconv ? gy : x;
    pl.p.partial = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    timing_begin(st);
    int rc;
    switch (pl.COT * 4 + pl.CIT * 2 + pl.S) {
        case 1 * 4 + 1 * 2 + 1: rc = launch_wgrad<1, 1, 1>(pl, st); break;
        case 1 * 4 + 2 * 2 + 1: rc = launch_wgrad<1, 2, 1>(pl, st); break;
        case 2 * 4 + 1 * 2 + 1: rc = launch_wgrad<2, 1, 1>(pl, st); break;
        case 2 * 4 + 2 * 2 + 1: rc = launch_wgrad<2, 2, 1>(pl, st); break;
        case 1 * 4 + 1 * 2 + 2: rc = launch_wgrad<1, 1, 2>(pl, st); break;
        case 1 * 4 + 2 * 2 + 2: rc = launch_wgrad<1, 2, 2>(pl, st); break;
        case 2 * 4 + 1 * 2 + 2: rc = launch_wgrad<2, 1, 2>(pl, st); break;
        default: rc = launch_wgrad<2, 2, 2>(pl, st); break;
    }
    if (rc == MVD_OK) {
        const int CSB = 16 * pl.COT, CGB = 16 * pl.CIT, nby = pl.cs_blocks * pl.p.cg_blocks;
        const unsigned nb = (unsigned)((nby * 27 * CSB * CGB + 255) / 256);
        hipLaunchKernelGGL(conv3d_weight_grad_reduce_kernel, dim3(nb), dim3(256), 0, st, pl.p.partial, gw, pl.P, pl.p.Cs, pl.p.Cg, CSB,
                           CGB, pl.p.cg_blocks, nby);
        rc = launch_status("conv3d_weight_grad_reduce");
    }
    timing_end(st);
    return rc;
}
}
