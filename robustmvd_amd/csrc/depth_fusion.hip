// Multi-view depth fusion: the cross-check of per-view depth maps against each other and the point cloud of the survivors.
// The reference has NO counterpart (it ends at the per-view depth map), so there is no file:line to cite: the definition is the
// comment of these entries in include/mvd.h, restated in float64 numpy by robustmvd_amd/depth_fusion.py's fuse_numpy.
//   mvd_geo_consistency_f32   per key pixel and source: project forward, blend the source depth, project back, test; the bit set of
//                             the consistent sources, the mean of the agreeing depths and the mask
//   mvd_compact_points_f32    the masked pixels in row-major order, back-projected to world coordinates, with their colour
//                             (the compaction of compact.h; only the back-projection and the colour gather are here)
// No atomics and fixed summation orders: two calls give the same bits.  The only LDS is the 1 KiB of the one-workgroup scan.
#include "compact.h"

namespace mvd {

// ---- geometric consistency ---------------------------------------------------------------------------------------------------------
// One lane per key pixel.  The workgroup is a 32 x 8 pixel tile, a wave 32 x 2 of it: a wave's key reads and stores are two full 128-byte
// lines, and the projections of neighbouring pixels are neighbours in the source, so a wave's 4 x 64 taps fall in about three rows
// of some 33 pixels and the eight waves of a tile share most of them in the CU's L1.  A row strip of 256 pixels would touch two source
// rows of ~257 pixels per wave and share nothing between waves.
constexpr int GC_TX = 32, GC_TY = 8;
constexpr int GC_MAT = 24;  // floats per source in the matrix table: A (9), b (3), A' (9), b' (3)

struct Probe {      // the forward projection of one key pixel into one source and the four taps around it
    float u, v;     // source position
    float fx, fy;   // bilinear weights of the right / lower taps
    float t00, t01, t10, t11;
    bool valid;     // d valid, in front of the source and inside its image (the taps are tested later)
};

// m is indexed with constants from a wave-uniform base: scalar loads.  (u,v) is formed from Q / d = A (x,y,1) + b / d, the same ratio
// with the same sign of its third component: for a source with the key's own intrinsics and pose (A = I, b = 0) it returns (x,y)
// itself, where round(d x) / d can leave the image by one ulp in the last column or row.
__device__ __forceinline__ Probe probe(const float* __restrict__ m, const float* __restrict__ src, float inv_d, bool d_ok, float x,
                                       float y, int H, int W) {
    Probe p;
    const float rx = fmaf(m[0], x, fmaf(m[1], y, m[2]));
    const float ry = fmaf(m[3], x, fmaf(m[4], y, m[5]));
    const float rz = fmaf(m[6], x, fmaf(m[7], y, m[8]));
    const float qx = fmaf(m[9], inv_d, rx), qy = fmaf(m[10], inv_d, ry), qz = fmaf(m[11], inv_d, rz);
    p.u = qx / qz;
    p.v = qy / qz;
    // a NaN fails every comparison
    p.valid = d_ok && qz > 0.f && p.u >= 0.f && p.u <= (float)(W - 1) && p.v >= 0.f && p.v <= (float)(H - 1);
    const int x0 = p.valid ? min((int)p.u, W - 2) : 0;  // u, v >= 0: the conversion is the floor
    const int y0 = p.valid ? min((int)p.v, H - 2) : 0;
    p.fx = p.u - (float)x0;
    p.fy = p.v - (float)y0;
    const float* t = src + (long long)y0 * W + x0;  // an invalid lane reads the cell at the origin, which exists (H, W >= 2)
    p.t00 = t[0];
    p.t01 = t[1];
    p.t10 = t[W];
    p.t11 = t[W + 1];
    return p;
}

__device__ __forceinline__ bool positive_finite(float f) { return f > 0.f && finite_f32(f); }

__global__ void __launch_bounds__(GC_TX * GC_TY) geo_consistency_kernel(const float* __restrict__ key, ViewPtrs srcs,
                                                                        const float* __restrict__ mats,
                                                                        const float* __restrict__ unc, int V, int H, int W,
                                                                        float max_err, float max_rel, int min_views, float max_unc,
                                                                        unsigned* __restrict__ bits_out, float* __restrict__ fused_out,
                                                                        unsigned char* __restrict__ mask_out,
                                                                        unsigned char* __restrict__ count_out) {
    const int px = blockIdx.x * GC_TX + threadIdx.x, py = blockIdx.y * GC_TY + threadIdx.y;
    if (px >= W || py >= H) return;  // partial tiles at the right and bottom edges; nothing below is cross-lane
    const long long pix = (long long)py * W + px;
    const float d = key[pix];
    const bool d_ok = positive_finite(d);
    const float x = (float)px, y = (float)py, inv_d = 1.0f / d;

    unsigned bits = 0u;
    int count = 0;
    float sum = d;
    // the taps of source s + 1 are in flight while source s is finished
    Probe cur = probe(mats, srcs.p[0], inv_d, d_ok, x, y, H, W);
    for (int s = 0; s < V; ++s) {
        Probe nxt = cur;
        if (s + 1 < V) nxt = probe(mats + (s + 1) * GC_MAT, srcs.p[s + 1], inv_d, d_ok, x, y, H, W);
        const float* __restrict__ m = mats + s * GC_MAT + 12;
        const bool taps_ok = positive_finite(cur.t00) && positive_finite(cur.t01) && positive_finite(cur.t10) && positive_finite(cur.t11);
        const float gx = 1.0f - cur.fx, gy = 1.0f - cur.fy;
        const float ds = fmaf(gx * gy, cur.t00, fmaf(cur.fx * gy, cur.t01, fmaf(gx * cur.fy, cur.t10, (cur.fx * cur.fy) * cur.t11)));
        const float rx = fmaf(m[0], cur.u, fmaf(m[1], cur.v, m[2]));
        const float ry = fmaf(m[3], cur.u, fmaf(m[4], cur.v, m[5]));
        const float rz = fmaf(m[6], cur.u, fmaf(m[7], cur.v, m[8]));
        const float qx = fmaf(ds, rx, m[9]), qy = fmaf(ds, ry, m[10]), dz = fmaf(ds, rz, m[11]);
        const float ex = qx / dz - x, ey = qy / dz - y;
        const float err = sqrtf(fmaf(ex, ex, ey * ey));
        const float rel = fabsf(dz - d) / d;
        const bool ok = cur.valid && taps_ok && err < max_err && rel < max_rel;
        if (ok) {
            bits |= 1u << s;
            sum += dz;
            ++count;
        }
        cur = nxt;
    }
    bits_out[pix] = bits;
    fused_out[pix] = d_ok ? sum / (float)(count + 1) : 0.f;
    bool keep = count >= min_views;
    if (unc) keep = keep && unc[pix] <= max_unc;  // false for a NaN
    mask_out[pix] = keep ? 1 : 0;
    if (count_out) count_out[pix] = (unsigned char)count;
}

// ---- point cloud -------------------------------------------------------------------------------------------------------------------
// The compaction of compact.h over the mask: its count, its scan, and the walk below, which back-projects every set pixel into its
// slot and gathers its colour.
struct MaskSet {
    const unsigned char* mask;
    __device__ bool operator()(long long p) const { return mask[p] != 0; }
};

__global__ void __launch_bounds__(CP_THREADS) compact_scatter_kernel(const unsigned char* __restrict__ mask,
                                                                     const float* __restrict__ depth, const float* __restrict__ image,
                                                                     const float* __restrict__ bp, const unsigned* __restrict__ offsets,
                                                                     int W, long long N, float* __restrict__ xyz,
                                                                     float* __restrict__ rgb) {
    compact_walk(MaskSet{mask}, offsets, N, [&](long long p, long long slot) {
        const int py = (int)p / W;  // N < 2^31 (checked by the entry): a 32-bit division
        const float x = (float)((int)p - py * W), y = (float)py, d = depth[p];
        float* o = xyz + 3 * slot;
        o[0] = fmaf(d, fmaf(bp[0], x, fmaf(bp[1], y, bp[2])), bp[9]);
        o[1] = fmaf(d, fmaf(bp[3], x, fmaf(bp[4], y, bp[5])), bp[10]);
        o[2] = fmaf(d, fmaf(bp[6], x, fmaf(bp[7], y, bp[8])), bp[11]);
        if (rgb) {
            float* c = rgb + 3 * slot;
            c[0] = image[p];
            c[1] = image[N + p];
            c[2] = image[2 * N + p];
        }
    });
}

}  // namespace mvd

extern "C" int mvd_geo_consistency_f32(const float* key_depth, const float* const* src_depth, const float* matrices,
                                       const float* uncertainty, int V, int H, int W, float max_reproj_error, float max_rel_depth_diff,
                                       int min_consistent_views, float max_uncertainty, unsigned* view_bits, float* fused,
                                       unsigned char* mask, unsigned char* num_consistent, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(key_depth && src_depth && matrices && view_bits && fused && mask, "geo_consistency: NULL argument");
    MVD_REQUIRE(V >= 1 && V <= MVD_MAX_VIEWS, "geo_consistency: %d sources, supported 1..%d", V, MVD_MAX_VIEWS);
    MVD_REQUIRE(H >= 2 && W >= 2, "geo_consistency: the maps must be at least 2 x 2, got %d x %d", H, W);
    MVD_REQUIRE((long long)H * W <= 0x7fffffffLL, "geo_consistency: map too large");
    ViewPtrs srcs{};
    for (int s = 0; s < V; ++s) {
        MVD_REQUIRE(src_depth[s], "geo_consistency: src_depth[%d] is NULL", s);
        srcs.p[s] = src_depth[s];
    }
    const dim3 grid((unsigned)((W + GC_TX - 1) / GC_TX), (unsigned)((H + GC_TY - 1) / GC_TY));
    MVD_REQUIRE(grid.y <= 65535u, "geo_consistency: map too tall");
    hipLaunchKernelGGL(geo_consistency_kernel, grid, dim3(GC_TX, GC_TY), 0, (hipStream_t)stream, key_depth, srcs, matrices, uncertainty, V,
                       H, W, max_reproj_error, max_rel_depth_diff, min_consistent_views, max_uncertainty, view_bits, fused, mask,
                       num_consistent);
    return launch_status("geo_consistency");
}

extern "C" size_t mvd_compact_points_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return mvd::compact_offsets_bytes((long long)H * W);
}

extern "C" int mvd_compact_points_f32(const unsigned char* mask, const float* depth, const float* image, const float* backproject, int H,
                                      int W, float* xyz, float* rgb, long long* count, void* workspace, size_t workspace_bytes,
                                      mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(mask && depth && backproject && xyz && count, "compact_points: NULL argument");
    MVD_REQUIRE(H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL, "compact_points: bad dimension");
    MVD_REQUIRE(!image == !rgb, "compact_points: image and rgb go together");
    MVD_REQUIRE(((uintptr_t)count & 7) == 0, "compact_points: count must be 8-byte aligned");
    MVD_REQUIRE(workspace && workspace_bytes >= mvd_compact_points_workspace_bytes(H, W), "compact_points: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const long long N = (long long)H * W;
    const unsigned nwg = compact_workgroups(N);
    unsigned* counts = static_cast<unsigned*>(workspace);
    hipLaunchKernelGGL(compact_count_kernel<MaskSet>, dim3(nwg), dim3(CP_THREADS), 0, st, MaskSet{mask}, N, counts);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(CP_THREADS), 0, st, counts, compact_chunks(N), count);
    hipLaunchKernelGGL(compact_scatter_kernel, dim3(nwg), dim3(CP_THREADS), 0, st, mask, depth, image, backproject, counts, W, N, xyz, rgb);
    return launch_status("compact_points");
}
