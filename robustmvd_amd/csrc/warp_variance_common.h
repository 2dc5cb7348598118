// K3 forward, what its kernels share: warp_variance.hip (entry points, gather kernel), warp_variance_tile.hip (tile kernel) and
// warp_variance_exp.hip (experimental variants, compiled only into the -DMVD_EXPERIMENTS library).  The arithmetic that the
// backward and the sweep kernels use as well -- sample_position<EXACT>, cell_weights, variance_finish -- is in
// sweep_homography.h; here are the pieces only the forward kernels have: the XCD-first block decode, the quad broadcast, the tap
// loads of a 2 x 2 cell, the blend of a cell into the running sums, the re-gather pattern and its dispatch, and the three-set
// schedule for four planes.
#pragma once
#include <type_traits>
#include "mvd_common.h"
#include "sweep_homography.h"

namespace mvd {

struct WarpParams {
    ViewPtrs src;           // V x (B,h+3,w+3,C) zero-bordered channel-last source features
    ViewPtrs proj;          // V x (B,4,4) source projection matrices
    const float* key;       // (B,h+3,w+3,C) zero-bordered channel-last key features (unused when WARP_ONLY)
    const float* M;         // (V,B,12) composed transforms
    const float* key_proj_inv;  // (B,4,4)
    const float* depth;     // (B,D)
    float* out;
    int B, D, h, w, V;
    int layout;             // MVD_LAYOUT_*
    int tiles_x, tiles_y, tiles_per_xcd;  // filled by the launchers
    int exact_grid;  // 1: sampling positions follow the reference's operation chain rounding for rounding
    float* absmax;   // optional (device, one float, zeroed by the launcher): receives max |out| (tile kernel; fp32 volume)
};

// The 1-D grid decoded XCD-first (blocks i and i+8 share an XCD, MI355X_MICROARCH.md): xcd | chunk fastest, then tile within the
// XCD's band of tiles, then batch.  Each XCD owns a contiguous band of key tiles for ALL depth chunks, so its private 4 MiB L2
// only sees the matching band of each source image.  `tile` can lie past the last tile: every kernel keeps its own early return.
struct BlockWork { int chunk, tile, b; };
__device__ __forceinline__ BlockWork decode_xcd_first(unsigned block, int chunks, int tiles_per_xcd) {
    const int xcd = block & 7;
    int j = block >> 3;
    BlockWork k;
    k.chunk = j % chunks; j /= chunks;
    const int tile_in = j % tiles_per_xcd;
    k.b = j / tiles_per_xcd;
    k.tile = xcd * tiles_per_xcd + tile_in;
    return k;
}

// every lane receives the value of lane I of its quad (DPP quad_perm:[I,I,I,I])
template <int I>
__device__ __forceinline__ unsigned quad_bcast(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, I * 0x55, 0xf, 0xf, true); }
template <int I>
__device__ __forceinline__ float quad_bcast(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), I * 0x55, 0xf, 0xf, true)); }

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// One plane of one source view: bilinear blend of the cell's 4 taps (4 channels per lane), then the running sum and sum
// of squares of mvsnet.py:131-134.
__device__ __forceinline__ void accumulate_cell(float4& a1, float4& a2, const float (&w)[4], const u32x4 (&t)[4]) {
    float4 acc = make_float4(0, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        acc.x = fmaf(__uint_as_float(t[k].x), w[k], acc.x);
        acc.y = fmaf(__uint_as_float(t[k].y), w[k], acc.y);
        acc.z = fmaf(__uint_as_float(t[k].z), w[k], acc.z);
        acc.w = fmaf(__uint_as_float(t[k].w), w[k], acc.w);
    }
    a1.x += acc.x; a1.y += acc.y; a1.z += acc.z; a1.w += acc.w;
    a2.x = fmaf(acc.x, acc.x, a2.x); a2.y = fmaf(acc.y, acc.y, a2.y);
    a2.z = fmaf(acc.z, acc.z, a2.z); a2.w = fmaf(acc.w, acc.w, a2.w);
}

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
// by VALUE on purpose: __builtin_bit_cast applied directly to a vector component (t.y) reads the vector's first dword
__device__ __forceinline__ f16x2 as_h2(unsigned v) { return __builtin_bit_cast(f16x2, v); }
__device__ __forceinline__ unsigned as_u32(f16x2 v) { return __builtin_bit_cast(unsigned, v); }

// fp16 taps (4 channels = 8 bytes per lane), fp32 weights and accumulation: fmaf((float)half, w, acc) is one
// v_fma_mix_f32 (exact f16 -> f32 conversion inside the FMA), so the result equals the fp32 kernel's on the same
// (fp16-representable) feature values, operation for operation
__device__ __forceinline__ void accumulate_cell(float4& a1, float4& a2, const float (&w)[4], const u32x2 (&t)[4]) {
    float4 acc = make_float4(0, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const f16x2 lo = as_h2(t[k].x), hi = as_h2(t[k].y);
        acc.x = fmaf((float)lo.x, w[k], acc.x);
        acc.y = fmaf((float)lo.y, w[k], acc.y);
        acc.z = fmaf((float)hi.x, w[k], acc.z);
        acc.w = fmaf((float)hi.y, w[k], acc.w);
    }
    a1.x += acc.x; a1.y += acc.y; a1.z += acc.z; a1.w += acc.w;
    a2.x = fmaf(acc.x, acc.x, a2.x); a2.y = fmaf(acc.y, acc.y, a2.y);
    a2.z = fmaf(acc.z, acc.z, a2.z); a2.w = fmaf(acc.w, acc.w, a2.w);
}

// (the b64 builtins traffic in GCC-style vectors; an implicit conversion to an ext_vector_type silently narrows the load
// to one dword with this compiler, so the lanes are moved explicitly)
typedef unsigned int u32x2n __attribute__((vector_size(8)));
__device__ __forceinline__ u32x2 load_b64(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    const u32x2n r = __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff, soff, 0);
    return u32x2{r[0], r[1]};
}
__device__ __forceinline__ void store_b64(u32x2 v, __amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
    const u32x2n r = {v.x, v.y};
    __builtin_amdgcn_raw_buffer_store_b64(r, rsrc, voff, 0, 0);
}

__device__ __forceinline__ void load_tap(u32x4& t, __amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    t = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0);
}
__device__ __forceinline__ void load_tap(u32x2& t, __amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) { t = load_b64(rsrc, voff, soff); }

// The four taps of a 2 x 2 cell (fp32: u32x4, fp16: u32x2 per lane) through a buffer descriptor: nw at byte offset `o`, ne one pixel
// (`pix` bytes: folds into the instruction's immediate) further, sw / se one padded row (`rowb` bytes) further.  The row pitch is
// either added into the vector offset (the gather kernel's form) or rides in the scalar offset operand (no per-lane address
// arithmetic besides `o` itself: the tile, located and marching kernels).
enum class RowPitch { in_voffset, in_soffset };
template <RowPitch PITCH, class TAP>
__device__ __forceinline__ void gather_cell(TAP (&f)[4], __amdgpu_buffer_rsrc_t rsrc, unsigned o, unsigned rowb, unsigned pix) {
    const unsigned vrow = PITCH == RowPitch::in_voffset ? rowb : 0u, srow = PITCH == RowPitch::in_soffset ? rowb : 0u;
    load_tap(f[0], rsrc, o, 0u);
    load_tap(f[1], rsrc, o + pix, 0u);
    load_tap(f[2], rsrc, o + vrow, srow);
    load_tap(f[3], rsrc, o + vrow + pix, srow);
}

// The wave's re-gather pattern over four planes: bit i-1 set = some lane's 2 x 2 cell differs between plane i-1 and plane i
__device__ __forceinline__ unsigned cell_change_mask(const unsigned (&off)[4]) {
    return (__builtin_amdgcn_ballot_w64(off[1] != off[0]) != 0 ? 1u : 0u) | (__builtin_amdgcn_ballot_w64(off[2] != off[1]) != 0 ? 2u : 0u) |
           (__builtin_amdgcn_ballot_w64(off[3] != off[2]) != 0 ? 4u : 0u);
}
// calls f(std::integral_constant<int, mask>): a pattern known at compile time lets every load be issued up front and waited for
// with exact counts
template <class F>
__device__ __forceinline__ void dispatch_mask(unsigned mask, const F& f) {
    switch (mask) {
        case 0: f(std::integral_constant<int, 0>{}); break;
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        default: f(std::integral_constant<int, 7>{}); break;
    }
}

// Four planes of one view for re-gather pattern MASK with at most three cells in flight (48 tap registers instead of 64): when all
// four planes re-gather, plane 3's loads are issued after plane 0's arithmetic, into the registers it frees.  `weights(I)` (I an
// integral_constant) returns plane I's four weights right where its arithmetic needs them; `gather(f, o)` loads the cell at `o`.
template <int MASK, class Weights, class Gather>
__device__ __forceinline__ void gather_blend_4planes_3sets(float4 (&s1)[4], float4 (&s2)[4], const unsigned (&off)[4],
                                                           const Weights& weights, const Gather& gather) {
    constexpr bool G1 = MASK & 1, G2 = (MASK >> 1) & 1, G3 = (MASK >> 2) & 1;
    auto blend = [&](auto I, const u32x4 (&f)[4]) {
        const float4 wq = weights(I);
        const float w[4] = {wq.x, wq.y, wq.z, wq.w};
        accumulate_cell(s1[I], s2[I], w, f);
    };
    std::integral_constant<int, 0> i0; std::integral_constant<int, 1> i1; std::integral_constant<int, 2> i2; std::integral_constant<int, 3> i3;
    u32x4 a[4], b[4], c[4];  // three register sets
    gather(a, off[0]);
    if constexpr (MASK == 7) {
        gather(b, off[1]);
        gather(c, off[2]);
        blend(i0, a);
        gather(a, off[3]);  // into the set plane 0 just released
        blend(i1, b);
        blend(i2, c);
        blend(i3, a);
    } else {
        // at most two of planes 1..3 re-gather: sets b and c take them in order
        if constexpr (G1) gather(b, off[1]);
        if constexpr (G2) gather(G1 ? c : b, off[2]);
        if constexpr (G3) gather((G1 || G2) ? c : b, off[3]);
        blend(i0, a);
        const u32x4 (&p1)[4] = G1 ? b : a;
        blend(i1, p1);
        const u32x4 (&p2)[4] = G2 ? (G1 ? c : b) : p1;
        blend(i2, p2);
        const u32x4 (&p3)[4] = G3 ? ((G1 || G2) ? c : b) : p2;
        blend(i3, p3);
    }
}

// LDS-footprint tile kernel (warp_variance_tile.hip): C = 32, channel-last volume
bool warp_tile_supported(const WarpParams& p, bool f16);
int launch_warp_tile(const WarpParams& p0, hipStream_t st, int tw, int win, int nch, int sets, bool f16, bool exact);

// gather kernel (warp_variance.hip): any C, either layout.  launch_gather launches one compiled form (LPP lanes per pixel, DPB
// planes per workgroup), launch_warp_gather the product's form for C channels
typedef void (*WarpKernel)(WarpParams);
int launch_gather(const WarpParams& p0, int lpp, int dpb, WarpKernel kernel, hipStream_t st);
int launch_warp_gather(const WarpParams& p, int C, bool warp_only, hipStream_t st);

// How the gather kernel reuses a plane's 2 x 2 cell when the next plane samples the same one (4 planes per workgroup)
enum class Reuse {
    none,               // every plane gathers its own cell (MVD_K3_CFG "dpb,minw")
    per_lane,           // exec-masked re-gather of the lanes whose cell moved, per-lane select of the registers ("r...")
    wave_uniform,       // re-gather for the whole wave where any lane's cell moved, pattern dispatched at compile time ("u...")
    wave_uniform_late,  // the same with three cells in flight and the weights broadcast where they are used ("v...")
};

#ifdef MVD_EXPERIMENTS
// One of the gather kernel's experimental forms (C = 32, folded grid)
struct GatherForm {
    Reuse reuse;
    int dpb, minw;
    WarpKernel kernel;
};
// The kernel MVD_K3_CFG = cfg selects for a complete WarpParams (warp_variance_exp.hip); returns an mvd_status
int warp_variance_experiment(const char* cfg, const WarpParams& p, int C, bool warp_only, bool f16, hipStream_t st,
                             const GatherForm* forms, int nforms);
#endif

}  // namespace mvd
