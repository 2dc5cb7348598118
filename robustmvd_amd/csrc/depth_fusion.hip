// Multi-view depth fusion: the cross-check of per-view depth maps against each other and the point cloud of the survivors.
// The reference has NO counterpart (it ends at the per-view depth map), so there is no file:line to cite: the definition is the
// comment of these entries in include/mvd.h, restated in float64 numpy by robustmvd_amd/depth_fusion.py's fuse_numpy.
//   mvd_geo_consistency_f32   per key pixel and source: project forward, blend the source depth, project back, test; the bit set of
//                             the consistent sources, the mean of the agreeing depths and the mask
//   mvd_compact_points_f32    the masked pixels in row-major order, back-projected to world coordinates, with their colour
//                             (the compaction of compact.h; only the back-projection and the colour gather are here)
//   mvd_depth_normals_f32     per pixel the world-frame normal of the depth map's surface, from a five-point stencil
//   mvd_geo_merge_f32         mvd_geo_consistency_f32 for a scene fused view by view: a pixel that an earlier view has merged into
//                             one of its points is not emitted again, an emitted pixel claims its consistent source pixels and
//                             carries the mean colour and normal of itself and of them (depth_fusion.py's merge_numpy)
//   mvd_compact_points_attr_f32   mvd_compact_points_f32 with a second gathered attribute (the normals)
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

// The forward projection, one copy: the verdict loop's probe and the merge kernel's second loop both call it, so that the pixel a
// consistent pair claims is the rounding of the very (u,v) its verdict was formed at.  Returns Q.z / d.
// m is indexed with constants from a wave-uniform base: scalar loads.  (u,v) is formed from Q / d = A (x,y,1) + b / d, the same ratio
// with the same sign of its third component: for a source with the key's own intrinsics and pose (A = I, b = 0) it returns (x,y)
// itself, where round(d x) / d can leave the image by one ulp in the last column or row.
__device__ __forceinline__ float project(const float* __restrict__ m, float inv_d, float x, float y, float& u, float& v) {
    const float rx = fmaf(m[0], x, fmaf(m[1], y, m[2]));
    const float ry = fmaf(m[3], x, fmaf(m[4], y, m[5]));
    const float rz = fmaf(m[6], x, fmaf(m[7], y, m[8]));
    const float qx = fmaf(m[9], inv_d, rx), qy = fmaf(m[10], inv_d, ry), qz = fmaf(m[11], inv_d, rz);
    u = qx / qz;
    v = qy / qz;
    return qz;
}

__device__ __forceinline__ Probe probe(const float* __restrict__ m, const float* __restrict__ src, float inv_d, bool d_ok, float x,
                                       float y, int H, int W) {
    Probe p;
    const float qz = project(m, inv_d, x, y, p.u, p.v);
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

// The verdicts of one key pixel against its V sources: the one copy behind geo_consistency_kernel and geo_merge_kernel, whose
// view_bits, fused and num_consistent are therefore the same bits on the same inputs.
struct Verdict {
    unsigned bits;  // bit s: source s is consistent
    int count;      // popcount(bits)
    float fused;    // (d + the consistent d') / (count + 1), 0 where d is invalid
    float inv_d;    // 1 / d, for a second forward projection
};

__device__ __forceinline__ Verdict verdicts(const float* __restrict__ key, const ViewPtrs& srcs, const float* __restrict__ mats, int V,
                                            int H, int W, long long pix, float x, float y, float max_err, float max_rel) {
    const float d = key[pix];
    const bool d_ok = positive_finite(d);
    const float inv_d = 1.0f / d;

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
    return Verdict{bits, count, d_ok ? sum / (float)(count + 1) : 0.f, inv_d};
}

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
    const Verdict r = verdicts(key, srcs, mats, V, H, W, pix, (float)px, (float)py, max_err, max_rel);
    bits_out[pix] = r.bits;
    fused_out[pix] = r.fused;
    bool keep = r.count >= min_views;
    if (unc) keep = keep && unc[pix] <= max_unc;  // false for a NaN
    mask_out[pix] = keep ? 1 : 0;
    if (count_out) count_out[pix] = (unsigned char)r.count;
}

// ---- merge -------------------------------------------------------------------------------------------------------------------------
// geo_consistency_kernel's verdicts, then for a pixel that is emitted (mask set and not claimed by an earlier view) a second loop over
// its consistent sources: the forward projection again (no taps), the byte 1 into that source's claimed map at the pixel nearest to
// (u,v) (rintf: half to even; one of the four taps of the verdict, so inside the image), and that pixel's colour and normal into the
// sums, in source order.  The loop runs s = 0 .. V-1 with the bit as a predicate, so that the per-source pointers stay scalar loads.
// Several lanes, of this launch's workgroups or of one wave, may store into the same byte: all of them store 1, no lane of this launch
// reads a source's claimed map (the entry refuses key_claimed among src_claimed), so two calls give the same bits without an atomic.
struct BytePtrs {
    unsigned char* p[MVD_MAX_VIEWS];
};

__global__ void __launch_bounds__(GC_TX * GC_TY) geo_merge_kernel(
    const float* __restrict__ key, ViewPtrs srcs, const float* __restrict__ mats, const float* __restrict__ unc, int V, int H, int W,
    float max_err, float max_rel, int min_views, float max_unc, const unsigned char* __restrict__ key_claimed, BytePtrs src_claimed,
    const float* __restrict__ key_image, ViewPtrs src_image, const float* __restrict__ key_normal, ViewPtrs src_normal,
    unsigned* __restrict__ bits_out, float* __restrict__ fused_out, unsigned char* __restrict__ mask_out,
    unsigned char* __restrict__ count_out, float* __restrict__ rgb_out, float* __restrict__ normal_out) {
    const int px = blockIdx.x * GC_TX + threadIdx.x, py = blockIdx.y * GC_TY + threadIdx.y;
    if (px >= W || py >= H) return;
    const long long pix = (long long)py * W + px, N = (long long)H * W;
    const float x = (float)px, y = (float)py;
    const unsigned char claimed = key_claimed[pix];  // asked for before the verdicts: in flight with the first taps
    const Verdict r = verdicts(key, srcs, mats, V, H, W, pix, x, y, max_err, max_rel);
    bits_out[pix] = r.bits;
    fused_out[pix] = r.fused;
    bool keep = r.count >= min_views;
    if (unc) keep = keep && unc[pix] <= max_unc;  // false for a NaN
    keep = keep && claimed == 0;
    mask_out[pix] = keep ? 1 : 0;
    if (count_out) count_out[pix] = (unsigned char)r.count;

    float c0 = 0.f, c1 = 0.f, c2 = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
    if (keep) {
        if (key_image) {
            c0 = key_image[pix];
            c1 = key_image[N + pix];
            c2 = key_image[2 * N + pix];
        }
        if (key_normal) {
            n0 = key_normal[pix];
            n1 = key_normal[N + pix];
            n2 = key_normal[2 * N + pix];
        }
        for (int s = 0; s < V; ++s) {
            if (!((r.bits >> s) & 1u)) continue;
            float u, v;
            project(mats + s * GC_MAT, r.inv_d, x, y, u, v);
            // a consistent pair has 0 <= u <= W-1 and 0 <= v <= H-1; the clamp costs two instructions and keeps the store inside the map
            // whatever the verdict was
            const int tx = min(max((int)rintf(u), 0), W - 1), ty = min(max((int)rintf(v), 0), H - 1);
            const long long t = (long long)ty * W + tx;
            src_claimed.p[s][t] = 1;
            if (key_image) {
                const float* __restrict__ im = src_image.p[s];
                c0 += im[t];
                c1 += im[N + t];
                c2 += im[2 * N + t];
            }
            if (key_normal) {
                const float* __restrict__ nm = src_normal.p[s];
                n0 += nm[t];
                n1 += nm[N + t];
                n2 += nm[2 * N + t];
            }
        }
        const float members = (float)(r.count + 1);
        c0 /= members;
        c1 /= members;
        c2 /= members;
        const float len = sqrtf(n0 * n0 + n1 * n1 + n2 * n2);
        const bool n_ok = positive_finite(len);
        n0 = n_ok ? n0 / len : 0.f;
        n1 = n_ok ? n1 / len : 0.f;
        n2 = n_ok ? n2 / len : 0.f;
    }
    if (rgb_out) {
        rgb_out[pix] = c0;
        rgb_out[N + pix] = c1;
        rgb_out[2 * N + pix] = c2;
    }
    if (normal_out) {
        normal_out[pix] = n0;
        normal_out[N + pix] = n1;
        normal_out[2 * N + pix] = n2;
    }
}

// ---- normals -----------------------------------------------------------------------------------------------------------------------
// One lane per pixel on geo_consistency_kernel's 32 x 8 tile: a wave is 32 x 2 pixels, so its five-point stencil reads four rows of at
// most 34 floats, a few 128-byte lines that the tile's other waves read too.  P(x,y) = d B (x,y,1) without the translation c, which
// cancels in the differences (and would cost digits at world coordinates far from the origin); n = (P(x+1,y) - P(x-1,y)) x
// (P(x,y+1) - P(x,y-1)), normalised, turned towards the camera (n . B (x,y,1) <= 0).  (0,0,0) on the image border, where one of the
// five depths is not finite or <= 0, and where the cross product's length is zero or not finite.
__device__ __forceinline__ void ray(const float* __restrict__ bp, float x, float y, float r[3]) {
    r[0] = fmaf(bp[0], x, fmaf(bp[1], y, bp[2]));
    r[1] = fmaf(bp[3], x, fmaf(bp[4], y, bp[5]));
    r[2] = fmaf(bp[6], x, fmaf(bp[7], y, bp[8]));
}

__global__ void __launch_bounds__(GC_TX * GC_TY) depth_normals_kernel(const float* __restrict__ depth, const float* __restrict__ bp, int H,
                                                                      int W, float* __restrict__ normals) {
    const int px = blockIdx.x * GC_TX + threadIdx.x, py = blockIdx.y * GC_TY + threadIdx.y;
    if (px >= W || py >= H) return;
    const long long pix = (long long)py * W + px, N = (long long)H * W;
    const bool inner = px > 0 && px < W - 1 && py > 0 && py < H - 1;
    // a border lane reads its own pixel five times: every address exists
    const long long dx = inner ? 1 : 0, dy = inner ? W : 0;
    const float d = depth[pix], dl = depth[pix - dx], dr = depth[pix + dx], du = depth[pix - dy], dd = depth[pix + dy];
    const float x = (float)px, y = (float)py;
    float rc[3], rl[3], rr[3], ru[3], rd[3];
    ray(bp, x, y, rc);
    ray(bp, x - 1.f, y, rl);
    ray(bp, x + 1.f, y, rr);
    ray(bp, x, y - 1.f, ru);
    ray(bp, x, y + 1.f, rd);
    float a[3], b[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a[i] = dr * rr[i] - dl * rl[i];
        b[i] = dd * rd[i] - du * ru[i];
    }
    float n0 = a[1] * b[2] - a[2] * b[1], n1 = a[2] * b[0] - a[0] * b[2], n2 = a[0] * b[1] - a[1] * b[0];
    const float len = sqrtf(n0 * n0 + n1 * n1 + n2 * n2);
    const bool ok = inner && positive_finite(d) && positive_finite(dl) && positive_finite(dr) && positive_finite(du) &&
                    positive_finite(dd) && positive_finite(len);
    const float towards = n0 * rc[0] + n1 * rc[1] + n2 * rc[2];
    const float scale = towards > 0.f ? -len : len;
    normals[pix] = ok ? n0 / scale : 0.f;
    normals[N + pix] = ok ? n1 / scale : 0.f;
    normals[2 * N + pix] = ok ? n2 / scale : 0.f;
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
                                                                     float* __restrict__ rgb, const float* __restrict__ attr,
                                                                     float* __restrict__ attr_out) {
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
        if (attr_out) {  // the second planar attribute (the normals), gathered like the colour
            float* a = attr_out + 3 * slot;
            a[0] = attr[p];
            a[1] = attr[N + p];
            a[2] = attr[2 * N + p];
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

extern "C" int mvd_depth_normals_f32(const float* depth, const float* backproject, int H, int W, float* normals, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(depth && backproject && normals, "depth_normals: NULL argument");
    MVD_REQUIRE(H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL, "depth_normals: bad dimension");
    const dim3 grid((unsigned)((W + GC_TX - 1) / GC_TX), (unsigned)((H + GC_TY - 1) / GC_TY));
    MVD_REQUIRE(grid.y <= 65535u, "depth_normals: map too tall");
    hipLaunchKernelGGL(depth_normals_kernel, grid, dim3(GC_TX, GC_TY), 0, (hipStream_t)stream, depth, backproject, H, W, normals);
    return launch_status("depth_normals");
}

extern "C" int mvd_geo_merge_f32(const float* key_depth, const float* const* src_depth, const float* matrices, const float* uncertainty,
                                 int V, int H, int W, float max_reproj_error, float max_rel_depth_diff, int min_consistent_views,
                                 float max_uncertainty, const unsigned char* key_claimed, unsigned char* const* src_claimed,
                                 const float* key_image, const float* const* src_image, const float* key_normal,
                                 const float* const* src_normal, unsigned* view_bits, float* fused, unsigned char* mask,
                                 unsigned char* num_consistent, float* merged_rgb, float* merged_normal, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(key_depth && src_depth && matrices && view_bits && fused && mask && key_claimed && src_claimed,
                "geo_merge: NULL argument");
    MVD_REQUIRE(V >= 1 && V <= MVD_MAX_VIEWS, "geo_merge: %d sources, supported 1..%d", V, MVD_MAX_VIEWS);
    MVD_REQUIRE(H >= 2 && W >= 2, "geo_merge: the maps must be at least 2 x 2, got %d x %d", H, W);
    MVD_REQUIRE((long long)H * W <= 0x7fffffffLL, "geo_merge: map too large");
    MVD_REQUIRE(!key_image == !src_image && !key_image == !merged_rgb, "geo_merge: key_image, src_image and merged_rgb go together");
    MVD_REQUIRE(!key_normal == !src_normal && !key_normal == !merged_normal,
                "geo_merge: key_normal, src_normal and merged_normal go together");
    ViewPtrs srcs{}, images{}, normals{};
    BytePtrs claims{};
    for (int s = 0; s < V; ++s) {
        MVD_REQUIRE(src_depth[s] && src_claimed[s], "geo_merge: src_depth[%d] or src_claimed[%d] is NULL", s, s);
        // the key's map is read while the sources' maps are written: one map in both roles would make the mask depend on the order
        // in which the lanes run
        MVD_REQUIRE(src_claimed[s] != key_claimed, "geo_merge: src_claimed[%d] is key_claimed (a view among its own sources)", s);
        MVD_REQUIRE(!key_image || src_image[s], "geo_merge: src_image[%d] is NULL", s);
        MVD_REQUIRE(!key_normal || src_normal[s], "geo_merge: src_normal[%d] is NULL", s);
        srcs.p[s] = src_depth[s];
        claims.p[s] = src_claimed[s];
        if (key_image) images.p[s] = src_image[s];
        if (key_normal) normals.p[s] = src_normal[s];
    }
    const dim3 grid((unsigned)((W + GC_TX - 1) / GC_TX), (unsigned)((H + GC_TY - 1) / GC_TY));
    MVD_REQUIRE(grid.y <= 65535u, "geo_merge: map too tall");
    hipLaunchKernelGGL(geo_merge_kernel, grid, dim3(GC_TX, GC_TY), 0, (hipStream_t)stream, key_depth, srcs, matrices, uncertainty, V, H, W,
                       max_reproj_error, max_rel_depth_diff, min_consistent_views, max_uncertainty, key_claimed, claims, key_image, images,
                       key_normal, normals, view_bits, fused, mask, num_consistent, merged_rgb, merged_normal);
    return launch_status("geo_merge");
}

extern "C" size_t mvd_compact_points_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return mvd::compact_offsets_bytes((long long)H * W);
}

extern "C" int mvd_compact_points_f32(const unsigned char* mask, const float* depth, const float* image, const float* backproject, int H,
                                      int W, float* xyz, float* rgb, long long* count, void* workspace, size_t workspace_bytes,
                                      mvd_stream_t stream) {
    return mvd_compact_points_attr_f32(mask, depth, image, nullptr, backproject, H, W, xyz, rgb, nullptr, count, workspace,
                                       workspace_bytes, stream);
}

extern "C" int mvd_compact_points_attr_f32(const unsigned char* mask, const float* depth, const float* image, const float* attr,
                                           const float* backproject, int H, int W, float* xyz, float* rgb, float* attr_out,
                                           long long* count, void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(mask && depth && backproject && xyz && count, "compact_points: NULL argument");
    MVD_REQUIRE(H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL, "compact_points: bad dimension");
    MVD_REQUIRE(!image == !rgb, "compact_points: image and rgb go together");
    MVD_REQUIRE(!attr == !attr_out, "compact_points: attr and attr_out go together");
    MVD_REQUIRE(((uintptr_t)count & 7) == 0, "compact_points: count must be 8-byte aligned");
    MVD_REQUIRE(workspace && workspace_bytes >= mvd_compact_points_workspace_bytes(H, W), "compact_points: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const long long N = (long long)H * W;
    const unsigned nwg = compact_workgroups(N);
    unsigned* counts = static_cast<unsigned*>(workspace);
    hipLaunchKernelGGL(compact_count_kernel<MaskSet>, dim3(nwg), dim3(CP_THREADS), 0, st, MaskSet{mask}, N, counts);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(CP_THREADS), 0, st, counts, compact_chunks(N), count);
    hipLaunchKernelGGL(compact_scatter_kernel, dim3(nwg), dim3(CP_THREADS), 0, st, mask, depth, image, backproject, counts, W, N, xyz, rgb,
                       attr, attr_out);
    return launch_status("compact_points");
}
