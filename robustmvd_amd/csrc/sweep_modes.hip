// Other consumers of the plane sweep as reduction modes of one generic kernel:
//   MVD_REDUCE_VARIANCE        MVSNet's variance over key + V sources             rmvd/models/mvsnet.py:124-135
//   MVD_REDUCE_VARIANCE_KEYSQ  CVP-MVSNet's cost volume as the reference computes it: `volume_sum = ref_volume;
//                              volume_sq_sum = ref_volume.pow_(2)` alias one tensor, so the running SUM starts from key^2 too
//                              (rmvd/models/cvp_mvsnet.py:129-130, blocks/cvp_mvsnet_components.py:393-394)
//   MVD_REDUCE_GROUPCORR       Vis-MVSNet's group-wise correlation, one volume per source view
//                              (rmvd/models/blocks/utils.py:71-89 called from blocks/vis_mvsnet_singlestage.py:242)
// with the two things those consumers vary: PER-PIXEL depth hypotheses (B,D,h,w) (cvp proj_cost, cvp_mvsnet_components.py:
// 375-456; vis depth_start n1hw) and the pixel-centre convention of the warp (`pix_offset`, `scale`, `bias`:
// homo_warp / homo_warping sample at (X/Z) * W/(W-1) - 0.5 from integer pixel positions, blocks/utils.py:246-264;
// homography_warping samples at X/Z - 0.5 from positions x + 0.5, blocks/utils.py:154-186).
// Per view the caller passes the 3x4 matrix [R | t] with (X,Y,Z) = R (x+o, y+o, 1)^T d + t.
//
// Generic and simple by design (the tuned K3 tile kernel is the hot path): thread = (pixel, unit), unit = channel quad
// (variance modes) or channel group (group correlation); pixels are the fast index so that stores into the
// reference's (B,C,D,h,w) layout are coalesced.  Gathers come from zero-bordered channel-last copies like K3's.
#include "sweep_homography.h"

namespace mvd {
int repack_padded_launch(const float* src, float* dst, int B, int C, int h, int w, hipStream_t st);
size_t padded_slot_bytes_public(int B, int C, int h, int w);

struct ReduceParams {
    ViewPtrs src;        // V x (B,h+3,w+3,C) zero-bordered channel-last
    ViewPtrs M;          // V x (B,3,4)
    ViewOutPtrs out;     // variance: out[0] (B,C,D,h,w); group correlation: out[v] (B,G,D,h,w)
    const float* key;    // (B,h+3,w+3,C)
    const float* depth;  // (B,D) or (B,D,h,w)
    int depth_per_pixel;
    float pix_offset, scale_x, scale_y, bias;
    float xlo, xhi, ylo, yhi;  // sweep_groupcorr_nhwc_kernel only: the reference's own clamp of the sample index, within [-1, w] x [-1, h]
    int mode, groups;
    int B, C, D, h, w, V;
};

// One bilinear sample of 4 channels (c0 .. c0+3) of source view v at the position plane `depth` puts key pixel (fx, fy) at.
__device__ __forceinline__ float4 reduce_sample(const ReduceParams& p, int v, int b, float fx, float fy, float depth, int c0, int W2,
                                                size_t img) {
    const SamplePos P = sample_position_div(p.M.p[v] + (size_t)b * 12, fx, fy, depth, p.scale_x, p.scale_y, p.bias, (float)p.w, (float)p.h);
    return sample_blend(p.src.p[v] + b * img, sample_cell(P, W2, p.C, c0), W2, p.C);
}

// The same reduction with the lanes of a pixel side by side (unit fastest: a pixel's units read whole 128-byte lines of a tap,
// the plain kernel's lanes = pixels read 16 bytes of each) and the results of a plane turned through LDS, so that a channel's
// 256 / units consecutive pixels leave as one run.  units = a power of two <= 64 (C / 4, or the number of groups).
// grid (ceil(h w / ppw), B), ppw = 256 / units pixels per workgroup.
__global__ void __launch_bounds__(256) sweep_reduce_tile_kernel(ReduceParams p, int units) {
    __shared__ __attribute__((aligned(16))) float tile[2][1024];
    const int h = p.h, w = p.w, C = p.C, D = p.D, V = p.V;
    const bool corr = p.mode == MVD_REDUCE_GROUPCORR;
    const int qpu = corr ? C / p.groups / 4 : 1;
    const int ppw = 256 / units;
    const int tid = threadIdx.x, unit = tid % units, lp = tid / units;
    const int b = blockIdx.y;
    const long long npix = (long long)h * w, pix0 = (long long)blockIdx.x * ppw;
    const long long pix = min(pix0 + lp, npix - 1);  // lanes beyond the map repeat its last pixel; their results are not stored
    const int x = (int)(pix % w), y = (int)(pix / w);
    const int W2 = w + 3;
    const size_t img = (size_t)(h + 3) * W2 * C;
    const float fx = (float)x + p.pix_offset, fy = (float)y + p.pix_offset;
    const float inv_nv = 1.0f / (float)(V + 1);
    const size_t dplane = (size_t)h * w;
    const bool vec4 = (dplane % 4 == 0) && ppw >= 4 && ((size_t)p.out.p[0] & 15) == 0;
    int buf = 0;

    for (int d = 0; d < D; ++d) {
        const float depth = p.depth_per_pixel ? p.depth[(((size_t)b * D + d) * h + y) * w + x] : p.depth[(size_t)b * D + d];
        if (!corr) {
            const int c0 = unit * 4;
            const float4 k = *reinterpret_cast<const float4*>(p.key + b * img + ((size_t)(y + 1) * W2 + (x + 1)) * C + c0);
            VarianceSums sums(k, p.mode == MVD_REDUCE_VARIANCE_KEYSQ);
            for (int v = 0; v < V; ++v) sums.add(reduce_sample(p, v, b, fx, fy, depth, c0, W2, img));
            const float4 r = sums.finish(inv_nv);
            float* t = tile[buf] + (c0 * ppw + lp);  // [channel][pixel]
            t[0] = r.x; t[ppw] = r.y; t[2 * ppw] = r.z; t[3 * ppw] = r.w;
            __syncthreads();
            // 1024 results = C channels x ppw pixels: thread -> 4 consecutive pixels of one channel
            if (vec4) {
                const int l4 = ppw / 4, ch = tid / l4, p4 = (tid % l4) * 4;
                const long long po = pix0 + p4;
                float* o = p.out.p[0] + (((size_t)b * C + ch) * D + d) * dplane + po;
                const float4 r = *reinterpret_cast<const float4*>(tile[buf] + ch * ppw + p4);
                if (po < npix) *reinterpret_cast<float4*>(o) = r;  // npix and po are multiples of 4: the four pixels are inside together
            } else {
                for (int e = tid; e < 1024; e += 256) {
                    const int ch = e / ppw, pp = e % ppw;
                    if (pix0 + pp < npix) p.out.p[0][(((size_t)b * C + ch) * D + d) * dplane + pix0 + pp] = tile[buf][e];
                }
            }
            buf ^= 1;
        } else {
            for (int v = 0; v < V; ++v) {
                float acc = 0.0f;
                for (int qq = 0; qq < qpu; ++qq) {
                    const int c0 = (unit * qpu + qq) * 4;
                    const float4 k = *reinterpret_cast<const float4*>(p.key + b * img + ((size_t)(y + 1) * W2 + (x + 1)) * C + c0);
                    const float4 sv = reduce_sample(p, v, b, fx, fy, depth, c0, W2, img);
                    const float dot = fmaf(k.w, sv.w, fmaf(k.z, sv.z, fmaf(k.y, sv.y, k.x * sv.x)));
                    acc = (qq == 0 ? 0.0f : acc) + dot;
                }
                tile[buf][unit * ppw + lp] = acc;  // [group][pixel]
                __syncthreads();
                const int g = tid / ppw, pp = tid % ppw;
                if (pix0 + pp < npix) p.out.p[v][(((size_t)b * p.groups + g) * D + d) * dplane + pix0 + pp] = tile[buf][tid];
                buf ^= 1;
            }
        }
    }
}

__global__ void __launch_bounds__(256) sweep_reduce_kernel(ReduceParams p) {
    const int h = p.h, w = p.w, C = p.C, D = p.D, V = p.V;
    const bool corr = p.mode == MVD_REDUCE_GROUPCORR;
    const int units = corr ? p.groups : C / 4;      // units per pixel
    const int qpu = corr ? C / p.groups / 4 : 1;    // channel quads per unit
    const long long npix = (long long)h * w;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)p.B * units * npix) return;
    const long long pix = t % npix;
    const int unit = (int)((t / npix) % units), b = (int)(t / (npix * units));
    const int x = (int)(pix % w), y = (int)(pix / w);
    const int W2 = w + 3;
    const size_t img = (size_t)(h + 3) * W2 * C;
    const float fx = (float)x + p.pix_offset, fy = (float)y + p.pix_offset;
    const float inv_nv = 1.0f / (float)(V + 1);
    const size_t dplane = (size_t)h * w;

    for (int d = 0; d < D; ++d) {
        const float depth = p.depth_per_pixel ? p.depth[(((size_t)b * D + d) * h + y) * w + x] : p.depth[(size_t)b * D + d];
        for (int qq = 0; qq < qpu; ++qq) {
            const int c0 = (unit * qpu + qq) * 4;
            const float4 k = *reinterpret_cast<const float4*>(p.key + b * img + ((size_t)(y + 1) * W2 + (x + 1)) * C + c0);
            VarianceSums sums(k, p.mode == MVD_REDUCE_VARIANCE_KEYSQ);
            for (int v = 0; v < V; ++v) {
                const float4 sv = reduce_sample(p, v, b, fx, fy, depth, c0, W2, img);
                if (corr) {
                    const float dot = fmaf(k.w, sv.w, fmaf(k.z, sv.z, fmaf(k.y, sv.y, k.x * sv.x)));
                    float* o = p.out.p[v] + (((size_t)b * p.groups + unit) * D + d) * dplane + pix;
                    *o = (qq == 0 ? 0.0f : *o) + dot;
                } else {
                    sums.add(sv);
                }
            }
            if (!corr) {
                const float4 r = sums.finish(inv_nv);
                float* o = p.out.p[0] + (((size_t)b * C + c0) * D + d) * dplane + pix;
                o[0] = r.x;
                o[(size_t)D * dplane] = r.y;
                o[2 * (size_t)D * dplane] = r.z;
                o[3 * (size_t)D * dplane] = r.w;
            }
        }
    }
}

// The variance modes on the layouts the engine uses between its own kernels (mvd_sweep_reduce_nhwc_f32): the key map dense
// channel-last (B,h,w,C) in p.key, the source maps zero-bordered channel-last as above (a 2-D layer wrote them: no repack), the
// volume channel-last (B,D,h,w,C) in p.out.p[0], what the 3-D convolutions read.
// Thread = (pixel, channel quad), quad fastest, units = C / 4 quads per pixel, ppw = 256 / units pixels per workgroup (threads beyond
// ppw * units idle when units does not divide 256).  A pixel's lanes read one tap's C floats as one run (64 B at C = 16) and thread t of
// a workgroup stores the float4 at plane + pix0 * C + 4 t: a plane's stores of consecutive pixels leave as whole lines, without a
// turn through LDS.  grid (ceil(h w / ppw), planes / NHWC_DPB rounded up, B): the coarse level (48 planes on a small map) fills the
// device through the plane chunks, a refinement level (8 planes) reads its key quad once.
constexpr int NHWC_DPB = 8;

__global__ void __launch_bounds__(256) sweep_reduce_nhwc_kernel(ReduceParams p, int units) {
    const int h = p.h, w = p.w, C = p.C, D = p.D, V = p.V;
    const int ppw = 256 / units;
    const int tid = threadIdx.x, unit = tid % units, lp = tid / units;
    const int b = blockIdx.z;
    const long long npix = (long long)h * w, pix = (long long)blockIdx.x * ppw + lp;
    if (lp >= ppw || pix >= npix) return;
    const int x = (int)(pix % w), y = (int)(pix / w);
    const int W2 = w + 3;
    const size_t img = (size_t)(h + 3) * W2 * C;
    const float fx = (float)x + p.pix_offset, fy = (float)y + p.pix_offset;
    const float inv_nv = 1.0f / (float)(V + 1);
    const int c0 = unit * 4;
    const float4 k = *reinterpret_cast<const float4*>(p.key + ((size_t)b * npix + pix) * C + c0);
    const int d0 = blockIdx.y * NHWC_DPB, d1 = min(D, d0 + NHWC_DPB);
    for (int d = d0; d < d1; ++d) {
        const float depth = p.depth_per_pixel ? p.depth[((size_t)b * D + d) * npix + pix] : p.depth[(size_t)b * D + d];
        VarianceSums sums(k, p.mode == MVD_REDUCE_VARIANCE_KEYSQ);
        for (int v = 0; v < V; ++v) sums.add(reduce_sample(p, v, b, fx, fy, depth, c0, W2, img));
        *reinterpret_cast<float4*>(p.out.p[0] + (((size_t)b * D + d) * npix + pix) * C + c0) = sums.finish(inv_nv);
    }
}

// Group correlation on the same layouts (mvd_sweep_groupcorr_nhwc_f32): the key map dense channel-last in p.key, the source maps
// zero-bordered channel-last, one volume per source view channel-last (B,D,h,w,G) in p.out.p[v], what Vis-MVSNet's pair regulariser reads.
// Thread = (pixel, group), group fastest, ppw = 256 / G pixels per workgroup (threads beyond ppw * G idle when G does not divide 256):
// thread t of a workgroup stores the float at plane + pix0 * G + t, so a wave's 64 lanes store 256 consecutive bytes of a plane.
// The sample position is reduce_sample's (sample_position_div, clamped to [-1, w] x [-1, h]) clamped once more to [xlo, xhi] x [ylo, yhi]:
// the reference clamps its normalised grid to +-1.1 before grid_sample (blocks/utils.py:168), i.e. the index to
// [-0.05 w - 0.5, 1.05 w - 0.5], which on a map narrower than 10 pixels lies INSIDE [-1, w]: a sample far outside such a map still
// takes a tenth of the rim pixel.  On wider maps, and without the clamp, the bounds are -1 and w and the second clamp is the identity.
// QPU = C / G / 4 key quads stay in registers across the planes of a chunk (QPU = 0: any count, the quads are read again per
// plane).  The dot products are the tile kernel's: the fmaf chain w, z, y, x per quad, quads added in order from 0.0f.
// grid as the variance kernel's: (ceil(h w / ppw), planes / NHWC_DPB rounded up, B): stage 1 (64 planes on a small map) fills the device.
template <int QPU>
__global__ void __launch_bounds__(256) sweep_groupcorr_nhwc_kernel(ReduceParams p) {
    const int h = p.h, w = p.w, C = p.C, D = p.D, V = p.V, G = p.groups;
    const int qpu = QPU ? QPU : C / G / 4;
    const int ppw = 256 / G;
    const int tid = threadIdx.x, g = tid % G, lp = tid / G;
    const int b = blockIdx.z;
    const long long npix = (long long)h * w, pix = (long long)blockIdx.x * ppw + lp;
    if (lp >= ppw || pix >= npix) return;
    const int x = (int)(pix % w), y = (int)(pix / w);
    const int W2 = w + 3;
    const size_t img = (size_t)(h + 3) * W2 * C;
    const float fx = (float)x + p.pix_offset, fy = (float)y + p.pix_offset;
    const int cg = g * qpu * 4;  // the group's first channel
    const float* kp = p.key + ((size_t)b * npix + pix) * C + cg;
    float4 k[QPU ? QPU : 1];
#pragma unroll
    for (int qq = 0; qq < QPU; ++qq) k[qq] = *reinterpret_cast<const float4*>(kp + 4 * qq);
    const int d0 = blockIdx.y * NHWC_DPB, d1 = min(D, d0 + NHWC_DPB);
    for (int d = d0; d < d1; ++d) {
        const float depth = p.depth_per_pixel ? p.depth[((size_t)b * D + d) * npix + pix] : p.depth[(size_t)b * D + d];
        for (int v = 0; v < V; ++v) {
            float acc = 0.0f;
#pragma unroll
            for (int qq = 0; qq < qpu; ++qq) {
                float4 kq;
                if constexpr (QPU > 0) kq = k[qq];
                else kq = *reinterpret_cast<const float4*>(kp + 4 * qq);
                SamplePos P = sample_position_div(p.M.p[v] + (size_t)b * 12, fx, fy, depth, p.scale_x, p.scale_y, p.bias, (float)w, (float)h);
                P.ix = __builtin_amdgcn_fmed3f(P.ix, p.xlo, p.xhi);
                P.iy = __builtin_amdgcn_fmed3f(P.iy, p.ylo, p.yhi);
                const float4 sv = sample_blend(p.src.p[v] + b * img, sample_cell(P, W2, C, cg + 4 * qq), W2, C);
                const float dot = fmaf(kq.w, sv.w, fmaf(kq.z, sv.z, fmaf(kq.y, sv.y, kq.x * sv.x)));
                acc = (qq == 0 ? 0.0f : acc) + dot;
            }
            p.out.p[v][(((size_t)b * D + d) * npix + pix) * G + g] = acc;
        }
    }
}

}  // namespace mvd

extern "C" {

int mvd_sweep_groupcorr_nhwc_f32(const float* key_feat, const float* const* src_feat, const float* const* M, const float* depth,
                                 int depth_per_pixel, float pix_offset, float scale_x, float scale_y, float bias, float grid_clamp,
                                 int groups, int B, int C, int D, int h, int w, int V, float* const* out, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(key_feat && src_feat && M && depth && out, "sweep_groupcorr_nhwc: NULL argument");
    MVD_REQUIRE(B > 0 && B <= 65535 && D > 0 && h > 1 && w > 1 && V >= 1 && V <= MVD_MAX_VIEWS, "sweep_groupcorr_nhwc: bad dimensions");
    MVD_REQUIRE(C >= 4 && C <= 64 && C % 4 == 0, "sweep_groupcorr_nhwc: C=%d must be a multiple of 4 up to 64", C);
    MVD_REQUIRE(groups > 0 && C % groups == 0 && (C / groups) % 4 == 0, "sweep_groupcorr_nhwc: C/groups = %d/%d must be a multiple of 4", C, groups);
    MVD_REQUIRE(((uintptr_t)key_feat & 15) == 0, "sweep_groupcorr_nhwc: key_feat must be 16-byte aligned");
    ReduceParams p{};
    for (int v = 0; v < V; ++v) {
        MVD_REQUIRE(src_feat[v] && M[v] && out[v], "sweep_groupcorr_nhwc: NULL view %d", v);
        MVD_REQUIRE(((uintptr_t)src_feat[v] & 15) == 0, "sweep_groupcorr_nhwc: src_feat[%d] must be 16-byte aligned", v);
        // out[0] like every map; the further volumes may be the slices that follow it in one buffer, which are only float-aligned
        // when B D h w groups is no multiple of 4 (the kernel stores them one float at a time)
        MVD_REQUIRE(((uintptr_t)out[v] & (v == 0 ? 15 : 3)) == 0, "sweep_groupcorr_nhwc: out[%d] must be %d-byte aligned", v, v == 0 ? 16 : 4);
        p.src.p[v] = src_feat[v];
        p.M.p[v] = M[v];
        p.out.p[v] = out[v];
    }
    p.key = key_feat;
    p.depth = depth; p.depth_per_pixel = depth_per_pixel;
    p.pix_offset = pix_offset; p.scale_x = scale_x; p.scale_y = scale_y; p.bias = bias;
    p.mode = MVD_REDUCE_GROUPCORR; p.groups = groups;
    p.xlo = -1.0f; p.xhi = (float)w; p.ylo = -1.0f; p.yhi = (float)h;
    if (grid_clamp > 0.0f) {  // grid_sample's un-normalisation ((g + 1) size - 1) / 2 of g = -+grid_clamp, in float32 like the reference's
        p.xlo = fmaxf(p.xlo, ((1.0f - grid_clamp) * (float)w - 1.0f) / 2.0f);
        p.xhi = fminf(p.xhi, ((1.0f + grid_clamp) * (float)w - 1.0f) / 2.0f);
        p.ylo = fmaxf(p.ylo, ((1.0f - grid_clamp) * (float)h - 1.0f) / 2.0f);
        p.yhi = fminf(p.yhi, ((1.0f + grid_clamp) * (float)h - 1.0f) / 2.0f);
        MVD_REQUIRE(p.xlo <= p.xhi && p.ylo <= p.yhi, "sweep_groupcorr_nhwc: grid_clamp=%f leaves no map", (double)grid_clamp);
    }
    p.B = B; p.C = C; p.D = D; p.h = h; p.w = w; p.V = V;
    const int ppw = 256 / groups;  // groups <= C / 4 <= 16
    const long long nbx = ((long long)h * w + ppw - 1) / ppw;
    const int nby = (D + NHWC_DPB - 1) / NHWC_DPB;
    MVD_REQUIRE(nbx <= 0x7fffffffLL && nby <= 65535, "sweep_groupcorr_nhwc: grid too large");
    const dim3 grid((unsigned)nbx, (unsigned)nby, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    switch (C / groups / 4) {
        case 1: hipLaunchKernelGGL(sweep_groupcorr_nhwc_kernel<1>, grid, dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL(sweep_groupcorr_nhwc_kernel<2>, grid, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL(sweep_groupcorr_nhwc_kernel<0>, grid, dim3(256), 0, st, p); break;
    }
    return launch_status("sweep_groupcorr_nhwc");
}

int mvd_sweep_reduce_nhwc_f32(const float* key_feat, const float* const* src_feat, const float* const* M, const float* depth,
                              int depth_per_pixel, float pix_offset, float scale_x, float scale_y, float bias, int mode, int B, int C,
                              int D, int h, int w, int V, float* out, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(key_feat && src_feat && M && depth && out, "sweep_reduce_nhwc: NULL argument");
    MVD_REQUIRE(B > 0 && B <= 65535 && D > 0 && h > 1 && w > 1 && V >= 1 && V <= MVD_MAX_VIEWS, "sweep_reduce_nhwc: bad dimensions");
    MVD_REQUIRE(C >= 4 && C <= 64 && C % 4 == 0, "sweep_reduce_nhwc: C=%d must be a multiple of 4 up to 64", C);
    MVD_REQUIRE(mode == MVD_REDUCE_VARIANCE || mode == MVD_REDUCE_VARIANCE_KEYSQ, "sweep_reduce_nhwc: mode %d (the variance modes only)", mode);
    MVD_REQUIRE((((uintptr_t)key_feat | (uintptr_t)out) & 15) == 0, "sweep_reduce_nhwc: key_feat and out must be 16-byte aligned");
    ReduceParams p{};
    for (int v = 0; v < V; ++v) {
        MVD_REQUIRE(src_feat[v] && M[v], "sweep_reduce_nhwc: NULL view %d", v);
        MVD_REQUIRE(((uintptr_t)src_feat[v] & 15) == 0, "sweep_reduce_nhwc: src_feat[%d] must be 16-byte aligned", v);
        p.src.p[v] = src_feat[v];
        p.M.p[v] = M[v];
    }
    p.key = key_feat;
    p.out.p[0] = out;
    p.depth = depth; p.depth_per_pixel = depth_per_pixel;
    p.pix_offset = pix_offset; p.scale_x = scale_x; p.scale_y = scale_y; p.bias = bias;
    p.mode = mode; p.groups = 1;
    p.B = B; p.C = C; p.D = D; p.h = h; p.w = w; p.V = V;
    const int units = C / 4, ppw = 256 / units;
    const long long nbx = ((long long)h * w + ppw - 1) / ppw;
    const int nby = (D + NHWC_DPB - 1) / NHWC_DPB;
    MVD_REQUIRE(nbx <= 0x7fffffffLL && nby <= 65535, "sweep_reduce_nhwc: grid too large");
    hipLaunchKernelGGL(sweep_reduce_nhwc_kernel, dim3((unsigned)nbx, (unsigned)nby, (unsigned)B), dim3(256), 0, (hipStream_t)stream, p, units);
    return launch_status("sweep_reduce_nhwc");
}

size_t mvd_sweep_reduce_workspace_bytes(int B, int C, int h, int w, int V) {
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || V < 0) return 0;
    return (size_t)(V + 1) * mvd::padded_slot_bytes_public(B, C, h, w);
}

int mvd_sweep_reduce_f32(const float* key_feat, const float* const* src_feat, const float* const* M, const float* depth,
                         int depth_per_pixel, float pix_offset, float scale_x, float scale_y, float bias, int mode, int groups,
                         int B, int C, int D, int h, int w, int V, float* const* out, void* workspace, size_t workspace_bytes,
                         mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(key_feat && src_feat && M && depth && out, "sweep_reduce: NULL argument");
    MVD_REQUIRE(B > 0 && D > 0 && h > 1 && w > 1 && V >= 1 && V <= MVD_MAX_VIEWS, "sweep_reduce: bad dimensions");
    MVD_REQUIRE(C >= 4 && C % 4 == 0, "sweep_reduce: C=%d must be a positive multiple of 4", C);
    MVD_REQUIRE(mode == MVD_REDUCE_VARIANCE || mode == MVD_REDUCE_VARIANCE_KEYSQ || mode == MVD_REDUCE_GROUPCORR, "sweep_reduce: mode %d", mode);
    if (mode == MVD_REDUCE_GROUPCORR)
        MVD_REQUIRE(groups > 0 && C % groups == 0 && (C / groups) % 4 == 0, "sweep_reduce: C/groups = %d/%d must be a multiple of 4", C, groups);
    const size_t need = mvd_sweep_reduce_workspace_bytes(B, C, h, w, V);
    if (!workspace || workspace_bytes < need) {
        set_error("sweep_reduce: workspace %zu B < required %zu B", workspace_bytes, need);
        return MVD_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t slot = padded_slot_bytes_public(B, C, h, w);
    char* ws = (char*)workspace;
    ReduceParams p{};
    int rc = repack_padded_launch(key_feat, (float*)ws, B, C, h, w, st);
    if (rc) return rc;
    p.key = (float*)ws;
    ws += slot;
    const int nout = mode == MVD_REDUCE_GROUPCORR ? V : 1;
    for (int v = 0; v < V; ++v) {
        MVD_REQUIRE(src_feat[v] && M[v], "sweep_reduce: NULL view %d", v);
        rc = repack_padded_launch(src_feat[v], (float*)ws, B, C, h, w, st);
        if (rc) return rc;
        p.src.p[v] = (float*)ws;
        ws += slot;
        p.M.p[v] = M[v];
    }
    for (int v = 0; v < nout; ++v) {
        MVD_REQUIRE(out[v], "sweep_reduce: NULL output %d", v);
        p.out.p[v] = out[v];
    }
    p.depth = depth; p.depth_per_pixel = depth_per_pixel;
    p.pix_offset = pix_offset; p.scale_x = scale_x; p.scale_y = scale_y; p.bias = bias;
    p.mode = mode; p.groups = groups;
    p.B = B; p.C = C; p.D = D; p.h = h; p.w = w; p.V = V;
    const int units = mode == MVD_REDUCE_GROUPCORR ? groups : C / 4;
    const long long nthr = (long long)B * units * h * w, nblk = (nthr + 255) / 256;
    MVD_REQUIRE(nblk <= 0x7fffffffLL, "sweep_reduce: grid too large");
    // (experiments library, MVD_REDUCE_PLAIN: the pixel-per-lane kernel for every shape — the variants test compares the two)
    if (units >= 2 && units <= 64 && (units & (units - 1)) == 0 && B <= 65535 && !exp_env("MVD_REDUCE_PLAIN")) {
        const int ppw = 256 / units;
        const long long nbx = ((long long)h * w + ppw - 1) / ppw;
        MVD_REQUIRE(nbx <= 0x7fffffffLL, "sweep_reduce: grid too large");
        hipLaunchKernelGGL(sweep_reduce_tile_kernel, dim3((unsigned)nbx, (unsigned)B), dim3(256), 0, st, p, units);
        return launch_status("sweep_reduce_tile");
    }
    hipLaunchKernelGGL(sweep_reduce_kernel, dim3((unsigned)nblk), dim3(256), 0, st, p);
    return launch_status("sweep_reduce");
}
}
