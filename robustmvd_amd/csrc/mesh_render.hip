// Mesh rendering: a triangle mesh rasterised into up to MVD_MAX_VIEWS pinhole views of one size: per view a depth map, a triangle-index
// map and on request barycentric, colour and normal maps.  The reference has NO counterpart, so there is no file:line to cite: the
// definition is the comment of mvd_mesh_render_f32 in include/mvd.h, restated in float64 numpy by robustmvd_amd/render.py
// (render_numpy).
//   project     vertex x view: the screen record (x, y, z, valid) into the workspace.  A record is a function of the vertex and the view
//               alone: every triangle that shares the vertex reads the same bits.
//   rasterise   The key buffer (V,H,W), 64-bit, starts at all ones; key = (float bits of z) << 32 | triangle index, z > 0, so the
//               smallest key is the nearest triangle and among equal depths the lowest index.  The winner is kept with a no-return
//               64-bit unsigned atomicMin on global memory: the minimum does not depend on the order of arrival, so two runs give the
//               same bits.  No float atomic anywhere.
//               setup kernel: one lane per (view, triangle).  A triangle whose clamped box holds at most max_small pixels is
//               rasterised right there by its lane; a larger one is flagged with the number of waves it is to get, the flags are
//               compacted into a list (compact.h: the chunk sums through the two-level scan, no atomic decides a position), and the
//               large kernel rasterises the list cooperatively: 64 consecutive pixels of the box per wave step, MR_MIN_STEPS steps
//               or more per wave and up to MR_SLICES waves per box, so that no wave walks a whole image (216 steps at 768 x 1152).
//   resolve     per pixel: depth from the key's own bits (exactly what the rasteriser compared), the index, and from the screen records
//               the barycentrics again with the same cover function; the optional maps; 16-byte stores where H W is a multiple of 4.
// One definition of the edge function and of the cover test (mesh_edge, mesh_cover), used by the lane path, the wave path and resolve.
// The file is compiled with -ffp-contract=off (csrc/Makefile) and says so itself below: the edge value is evaluated as written.
#include "compact.h"

#pragma clang fp contract(off)

namespace mvd {

constexpr int MR_THREADS = 256;
constexpr int MR_SLICES = 64;      // the most waves that share the steps of one large box
constexpr int MR_MIN_STEPS = 16;   // a wave of the large kernel gets at least this many steps of 64 pixels (the last of a box fewer)
constexpr int MR_LARGE_WGS = 256;  // workgroups (x) of the large kernel; each wave strides over the list

struct MeshView {
    int H, W;
    long long HW;
};

// ---- project ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MR_THREADS) mesh_project_kernel(const float* __restrict__ vertices, long long M,
                                                                  const float* __restrict__ mats, float near_plane,
                                                                  float4* __restrict__ records) {
    const long long m = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    const int v = blockIdx.y;
    if (m >= M) return;
    const float* __restrict__ P = mats + 12 * v;  // v is uniform: scalar loads
    const float X = vertices[3 * m], Y = vertices[3 * m + 1], Z = vertices[3 * m + 2];
    const float qx = P[0] * X + P[1] * Y + P[2] * Z + P[3];
    const float qy = P[4] * X + P[5] * Y + P[6] * Z + P[7];
    const float qz = P[8] * X + P[9] * Y + P[10] * Z + P[11];
    const float x = qx / qz, y = qy / qz;  // correctly rounded divisions: the numpy float32 chain's bits
    const bool valid = qz > near_plane && finite_f32(x) && finite_f32(y);  // a NaN fails every comparison
    records[(long long)v * M + m] = make_float4(x, y, qz, valid ? 1.0f : 0.0f);
}

// ---- the one edge function and cover test ------------------------------------------------------------------------------------------
// e_ab(p) for the vertex pair a < b (by index), as written, one rounding per operation
__device__ __forceinline__ float mesh_edge(const float4& a, const float4& b, float px, float py) {
    return (b.x - a.x) * (py - a.y) - (b.y - a.y) * (px - a.x);
}
// the oriented edge (i,j): +e_ij where i < j, -e_ji otherwise, so that two triangles that share it compute the same bits
__device__ __forceinline__ float mesh_oriented_edge(int i, int j, const float4& ri, const float4& rj, float px, float py) {
    return i < j ? mesh_edge(ri, rj, px, py) : -mesh_edge(rj, ri, px, py);
}

struct MeshTriangle {
    int i0, i1, i2;
    float4 r0, r1, r2;  // the screen records
    float sgn;          // sign(A)
    int x0, x1, y0, y1;  // the clamped box; empty (x0 > x1) for a skipped triangle
    __device__ long long pixels() const { return x0 > x1 || y0 > y1 ? 0ll : (long long)(x1 - x0 + 1) * (y1 - y0 + 1); }
};

struct MeshCover {
    float b0, b1, b2;  // barycentrics
    float u0, u1, u2;  // b_k / z_k
    float z;
};

// steps 3 of the definition: the triangle's records, orientation and clamped box
__device__ __forceinline__ MeshTriangle mesh_setup(const int* __restrict__ triangles, const float4* __restrict__ rec, long long t,
                                                   long long M, const MeshView& g, int cull) {
    MeshTriangle s;
    s.i0 = triangles[3 * t], s.i1 = triangles[3 * t + 1], s.i2 = triangles[3 * t + 2];
    // the caller checks the index range; an index outside it still reads no memory outside the records: the triangle is skipped
    const bool inside = (unsigned)s.i0 < (unsigned long long)M && (unsigned)s.i1 < (unsigned long long)M && (unsigned)s.i2 < (unsigned long long)M;
    const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
    s.r0 = inside ? rec[s.i0] : none, s.r1 = inside ? rec[s.i1] : none, s.r2 = inside ? rec[s.i2] : none;
    const float A = (s.r1.x - s.r0.x) * (s.r2.y - s.r0.y) - (s.r1.y - s.r0.y) * (s.r2.x - s.r0.x);
    bool ok = s.r0.w != 0.f && s.r1.w != 0.f && s.r2.w != 0.f && (A < 0.f || A > 0.f);
    if (cull == 1) ok = ok && !(A > 0.f);
    if (cull == 2) ok = ok && !(A < 0.f);
    s.sgn = A < 0.f ? -1.0f : 1.0f;
    // clamped as floats first: a box far outside the image stays representable
    const float fx0 = fminf(fmaxf(ceilf(fminf(fminf(s.r0.x, s.r1.x), s.r2.x)), 0.f), (float)g.W);
    const float fx1 = fminf(fmaxf(floorf(fmaxf(fmaxf(s.r0.x, s.r1.x), s.r2.x)), -1.f), (float)(g.W - 1));
    const float fy0 = fminf(fmaxf(ceilf(fminf(fminf(s.r0.y, s.r1.y), s.r2.y)), 0.f), (float)g.H);
    const float fy1 = fminf(fmaxf(floorf(fmaxf(fmaxf(s.r0.y, s.r1.y), s.r2.y)), -1.f), (float)(g.H - 1));
    ok = ok && fx0 <= fx1 && fy0 <= fy1;  // false for NaN
    s.x0 = ok ? (int)fx0 : 1, s.x1 = ok ? (int)fx1 : 0, s.y0 = ok ? (int)fy0 : 1, s.y1 = ok ? (int)fy1 : 0;
    return s;
}

// steps 4 and 5: covered?  and if so the barycentrics and the depth
__device__ __forceinline__ bool mesh_cover(const MeshTriangle& s, float px, float py, MeshCover& c) {
    const float w0 = s.sgn * mesh_oriented_edge(s.i1, s.i2, s.r1, s.r2, px, py);
    const float w1 = s.sgn * mesh_oriented_edge(s.i2, s.i0, s.r2, s.r0, px, py);
    const float w2 = s.sgn * mesh_oriented_edge(s.i0, s.i1, s.r0, s.r1, px, py);
    const float sum = (w0 + w1) + w2;
    if (!(w0 >= 0.f && w1 >= 0.f && w2 >= 0.f && sum > 0.f)) return false;
    c.b0 = w0 / sum, c.b1 = w1 / sum, c.b2 = w2 / sum;
    c.u0 = c.b0 / s.r0.z, c.u1 = c.b1 / s.r1.z, c.u2 = c.b2 / s.r2.z;
    c.z = 1.0f / ((c.u0 + c.u1) + c.u2);
    return finite_f32(c.z);
}

// Keys only fall, so a value read with a plain load is never below the current one: a lane whose key is not smaller than what it reads
// has lost already and may skip the atomic (SKIP).  Measured, that does not pay: with the load the rasterise stage takes 1.26 to
// 1.36 times as long on a one-pixel-per-triangle mesh and 1.16 to 1.21 times with a full-image quad behind it
// (profiles/mesh_render.txt), so the product path issues the atomic at once and SKIP stays as MVD_RENDER_LOAD_FIRST for measurements.
template <bool SKIP>
__device__ __forceinline__ void mesh_offer(unsigned long long* __restrict__ slot, float z, long long t) {
    const unsigned long long key = (unsigned long long)__float_as_uint(z) << 32 | (unsigned long long)(unsigned)t;
    if (SKIP && __builtin_nontemporal_load(slot) <= key) return;
    atomicMin(slot, key);  // the result is not used: the no-return form
}

// ---- rasterise: setup, and the small triangles on their lanes -----------------------------------------------------------------------
// Element p = v T + t of the n = V T < 2^32 (view, triangle) pairs, in compact.h's chunks.  flags[p]: 0, or for a triangle left to the
// large kernel the number of waves that share it, 1 .. MR_SLICES.
__device__ __forceinline__ unsigned mesh_slices(long long pixels) {
    const long long steps = (pixels + 63) / 64;
    return (unsigned)min((long long)MR_SLICES, (steps + MR_MIN_STEPS - 1) / MR_MIN_STEPS);
}

template <bool SKIP>
__global__ void __launch_bounds__(CP_THREADS) mesh_setup_kernel(const int* __restrict__ triangles, long long T, long long M,
                                                                const float4* __restrict__ records, MeshView g, long long n, int cull,
                                                                int max_small, unsigned long long* __restrict__ keys,
                                                                unsigned char* __restrict__ flags, unsigned* __restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const long long chunk = compact_wave_chunk();
    if (chunk * CP_CHUNK >= n) return;  // the whole wave
    unsigned large[CP_SUB];
#pragma unroll
    for (int k = 0; k < CP_SUB; ++k) {
        const long long p = chunk * CP_CHUNK + 64 * k + lane;
        large[k] = 0u;
        if (p >= n) continue;
        const long long v = (unsigned)p / (unsigned)T, t = p - v * T;  // n < 2^32: a 32-bit division
        const MeshTriangle s = mesh_setup(triangles, records + v * M, t, M, g, cull);
        const long long pixels = s.pixels();
        large[k] = pixels > (long long)max_small ? 1u : 0u;
        flags[p] = (unsigned char)(large[k] ? mesh_slices(pixels) : 0u);
        if (pixels == 0 || large[k]) continue;
        unsigned long long* __restrict__ row = keys + v * g.HW + (long long)s.y0 * g.W;
        for (int y = s.y0; y <= s.y1; ++y, row += g.W) {
            for (int x = s.x0; x <= s.x1; ++x) {
                MeshCover c;
                if (mesh_cover(s, (float)x, (float)y, c)) mesh_offer<SKIP>(row + x, c.z, t);
            }
        }
    }
    compact_store_chunk_sum(large, n, sums);
}

struct MeshLargeFlag {
    const unsigned char* flags;
    __device__ unsigned operator()(long long p) const { return flags[p] ? 1u : 0u; }
};

__global__ void __launch_bounds__(CP_THREADS) mesh_list_kernel(const unsigned char* __restrict__ flags, const unsigned* __restrict__ offsets,
                                                               long long n, unsigned* __restrict__ list,
                                                               unsigned char* __restrict__ slices) {
    compact_walk_counted(MeshLargeFlag{flags}, offsets, n, [&](long long p, long long slot, unsigned) {
        list[slot] = (unsigned)p;
        slices[slot] = flags[p];
    });
}

// ---- rasterise: the large triangles, a wave per (list entry, slice) ---------------------------------------------------------------------
// blockIdx.y is the slice.  A wave whose slice the entry does not use learns that from the entry's byte alone.
template <bool SKIP>
__global__ void __launch_bounds__(MR_THREADS) mesh_large_kernel(const int* __restrict__ triangles, long long T, long long M,
                                                                const float4* __restrict__ records, MeshView g, int cull,
                                                                const unsigned* __restrict__ list,
                                                                const unsigned char* __restrict__ slices,
                                                                const long long* __restrict__ total,
                                                                unsigned long long* __restrict__ keys) {
    const int lane = threadIdx.x & 63, slice = blockIdx.y;
    const long long L = total[0];
    const long long waves = (long long)gridDim.x * (MR_THREADS / 64);
    for (long long l = (long long)blockIdx.x * (MR_THREADS / 64) + (threadIdx.x >> 6); l < L; l += waves) {
        const int share = min((int)slices[l], MR_SLICES);  // wave-uniform, like everything up to the step loop
        if (slice >= share) continue;
        const long long p = list[l];
        const long long v = (unsigned)p / (unsigned)T, t = p - v * T;
        const MeshTriangle s = mesh_setup(triangles, records + v * M, t, M, g, cull);
        const long long pixels = s.pixels();  // > 0: the setup kernel flagged it from the same records
        const long long steps = (pixels + 63) / 64;
        const long long first = steps * slice / share, last = steps * (slice + 1) / share;
        const int bw = s.x1 - s.x0 + 1;
        unsigned long long* __restrict__ view = keys + v * g.HW;
        for (long long step = first; step < last; ++step) {
            const long long q = step * 64 + lane;
            if (q >= pixels) continue;
            const int yy = (int)(q / bw), xx = (int)(q - (long long)yy * bw);
            const int x = s.x0 + xx, y = s.y0 + yy;  // inside the clamped box: inside the image
            MeshCover c;
            if (mesh_cover(s, (float)x, (float)y, c)) mesh_offer<SKIP>(view + (long long)y * g.W + x, c.z, t);
        }
    }
}

// ---- resolve ---------------------------------------------------------------------------------------------------------------------
constexpr int MR_PIX = 4;  // consecutive pixels of the (V,H,W) index per lane

struct MeshMaps {
    float* depth;   // (V,H,W)
    int* triangle;  // (V,H,W)
    float* bary;    // (V,3,H,W) or NULL
    float* colors;  // (V,3,H,W) or NULL
    float* normals;  // (V,3,H,W) or NULL
};

__device__ __forceinline__ void mesh_store3(float* __restrict__ map, long long v, long long pix, long long HW, bool vec,
                                            const float (&val)[3][MR_PIX], int cnt) {
    if (!map) return;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float* __restrict__ o = map + (3 * v + ch) * HW + pix;
        if (vec) {
            *reinterpret_cast<float4*>(o) = make_float4(val[ch][0], val[ch][1], val[ch][2], val[ch][3]);
        } else {
#pragma unroll
            for (int e = 0; e < MR_PIX; ++e) {
                if (e < cnt) o[e] = val[ch][e];
            }
        }
    }
}

__global__ void __launch_bounds__(MR_THREADS) mesh_resolve_kernel(const unsigned long long* __restrict__ keys,
                                                                  const int* __restrict__ triangles, long long T, long long M,
                                                                  const float4* __restrict__ records, const float* __restrict__ vertices,
                                                                  const float* __restrict__ vcolors, MeshView g, long long total,
                                                                  int cull, MeshMaps out) {
    const long long p0 = ((long long)blockIdx.x * MR_THREADS + threadIdx.x) * MR_PIX;
    if (p0 >= total) return;
    const bool vec = (g.HW & 3) == 0;  // then the four pixels are in one view and every plane's offset is a multiple of 16 bytes
    float depth[MR_PIX], bary[3][MR_PIX], col[3][MR_PIX], nrm[3][MR_PIX];
    int index[MR_PIX];
    const bool attrs = out.bary || out.colors;
#pragma unroll
    for (int e = 0; e < MR_PIX; ++e) {
        depth[e] = 0.f, index[e] = -1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) bary[ch][e] = col[ch][e] = nrm[ch][e] = 0.f;
        const long long p = p0 + e;
        if (p >= total) continue;
        const unsigned long long key = keys[p];
        if (key == ~0ull) continue;
        const long long t = (long long)(unsigned)key;
        if (t >= T) continue;  // never with this call's own keys; a stale workspace must not make a lane read outside
        depth[e] = __uint_as_float((unsigned)(key >> 32));
        index[e] = (int)t;
        const long long v = p / g.HW, pix = p - v * g.HW;
        if (attrs) {
            const int y = (int)(pix / g.W), x = (int)(pix - (long long)y * g.W);
            const MeshTriangle s = mesh_setup(triangles, records + v * M, t, M, g, cull);
            MeshCover c;
            if (mesh_cover(s, (float)x, (float)y, c)) {  // the winner covered this pixel with these bits
                bary[0][e] = c.b0, bary[1][e] = c.b1, bary[2][e] = c.b2;
                if (out.colors) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        col[ch][e] = c.z * ((c.u0 * vcolors[3ll * s.i0 + ch] + c.u1 * vcolors[3ll * s.i1 + ch])
                                            + c.u2 * vcolors[3ll * s.i2 + ch]);
                    }
                }
            }
        }
        if (out.normals) {
            const int i0 = triangles[3 * t], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];  // in range: the triangle won
            float a[3], b[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float o = vertices[3ll * i0 + ch];
                a[ch] = vertices[3ll * i1 + ch] - o, b[ch] = vertices[3ll * i2 + ch] - o;
            }
            const float nx = a[1] * b[2] - a[2] * b[1], ny = a[2] * b[0] - a[0] * b[2], nz = a[0] * b[1] - a[1] * b[0];
            const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
            if (len > 0.f && finite_f32(len)) nrm[0][e] = nx / len, nrm[1][e] = ny / len, nrm[2][e] = nz / len;
        }
    }
    const int cnt = (int)min((long long)MR_PIX, total - p0);
    if (cnt == MR_PIX) {  // total = V H W and p0 are multiples of 4 or not together; the maps are 16-byte aligned
        *reinterpret_cast<float4*>(out.depth + p0) = make_float4(depth[0], depth[1], depth[2], depth[3]);
        *reinterpret_cast<int4*>(out.triangle + p0) = make_int4(index[0], index[1], index[2], index[3]);
    } else {
#pragma unroll
        for (int e = 0; e < MR_PIX; ++e) {
            if (e < cnt) out.depth[p0 + e] = depth[e], out.triangle[p0 + e] = index[e];
        }
    }
    if (vec) {
        const long long v = p0 / g.HW, pix = p0 - v * g.HW;
        mesh_store3(out.bary, v, pix, g.HW, true, bary, cnt);
        mesh_store3(out.colors, v, pix, g.HW, true, col, cnt);
        mesh_store3(out.normals, v, pix, g.HW, true, nrm, cnt);
    } else {  // the four pixels may lie in two views: one at a time
#pragma unroll
        for (int e = 0; e < MR_PIX; ++e) {
            if (e >= cnt) continue;
            const long long v = (p0 + e) / g.HW, pix = (p0 + e) - v * g.HW;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                if (out.bary) out.bary[(3 * v + ch) * g.HW + pix] = bary[ch][e];
                if (out.colors) out.colors[(3 * v + ch) * g.HW + pix] = col[ch][e];
                if (out.normals) out.normals[(3 * v + ch) * g.HW + pix] = nrm[ch][e];
            }
        }
    }
}

// the workspace: records | keys | chunk sums | total | block sums | flags | list | the list's slice counts, each 256-byte aligned
struct MeshWorkspace {
    size_t records, keys, sums, total, block, flags, list, slices, bytes;
};

static MeshWorkspace mesh_workspace(long long M, long long T, int V, int H, int W) {
    const long long n = (long long)V * T;
    MeshWorkspace w;
    size_t at = 0;
    w.records = at, at += align_up((size_t)V * (size_t)M * sizeof(float4), 256);
    w.keys = at, at += align_up((size_t)V * H * W * sizeof(unsigned long long), 256);
    w.sums = at, at += compact_offsets_bytes(n);
    w.total = at, at += 256;
    w.block = at, at += compact_block_bytes(n);
    w.flags = at, at += align_up((size_t)n, 256);
    w.list = at, at += align_up((size_t)n * sizeof(unsigned), 256);
    w.slices = at, at += align_up((size_t)n, 256);
    w.bytes = at;
    return w;
}

}  // namespace mvd

extern "C" size_t mvd_mesh_render_workspace_bytes(long long M, long long T, int V, int H, int W) {
    if (M < 0 || T < 0 || V <= 0 || H <= 0 || W <= 0) return 0;
    return mvd::mesh_workspace(M, T, V, H, W).bytes;
}

extern "C" int mvd_mesh_render_f32(const float* vertices, long long M, const int* triangles, long long T, const float* colors,
                                   const float* matrices, int V, int H, int W, float near_plane, int cull, int max_small, int flags,
                                   float* depth, int* triangle, float* bary, float* out_colors, float* normals, void* workspace,
                                   size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(matrices && depth && triangle, "mesh_render: NULL argument");
    MVD_REQUIRE(V >= 1 && V <= MVD_MAX_VIEWS, "mesh_render: %d views, supported 1..%d", V, MVD_MAX_VIEWS);
    MVD_REQUIRE(H >= 1 && W >= 1 && (long long)H * W * V <= 0x7fffffffLL, "mesh_render: H W V = %lld must be in 1 .. 2^31 - 1",
                (long long)H * W * V);
    MVD_REQUIRE(M >= 0 && M <= 0x7fffffffLL && T >= 0 && T <= 0x7fffffffLL, "mesh_render: M = %lld and T = %lld must be in 0 .. 2^31 - 1",
                M, T);
    MVD_REQUIRE((long long)V * T <= 0xffffffffLL, "mesh_render: V T = %lld must be below 2^32 (render fewer views per call)",
                (long long)V * T);
    MVD_REQUIRE((vertices || M == 0) && (triangles || T == 0) && (M > 0 || T == 0), "mesh_render: vertices / triangles missing");
    MVD_REQUIRE(cull >= 0 && cull <= 2, "mesh_render: cull must be 0 (none), 1 (back) or 2 (front)");
    MVD_REQUIRE(max_small >= 0, "mesh_render: max_small must not be negative");
    MVD_REQUIRE(!out_colors || colors, "mesh_render: a colour map needs vertex colours");
    MVD_REQUIRE((((uintptr_t)depth | (uintptr_t)triangle | (uintptr_t)bary | (uintptr_t)out_colors | (uintptr_t)normals) & 15) == 0,
                "mesh_render: the maps must be 16-byte aligned");
    const MeshWorkspace w = mesh_workspace(M, T, V, H, W);
    MVD_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= w.bytes,
                "mesh_render: workspace too small or not 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    float4* records = reinterpret_cast<float4*>(ws + w.records);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + w.keys);
    unsigned* sums = reinterpret_cast<unsigned*>(ws + w.sums);
    long long* total = reinterpret_cast<long long*>(ws + w.total);
    unsigned* block = reinterpret_cast<unsigned*>(ws + w.block);
    unsigned char* flag = ws + w.flags;
    unsigned* list = reinterpret_cast<unsigned*>(ws + w.list);
    unsigned char* slices = ws + w.slices;
    const MeshView g{H, W, (long long)H * W};
    const long long n = (long long)V * T, pixels = g.HW * V;
    const bool skip = (flags & MVD_RENDER_LOAD_FIRST) != 0;

    if (!(flags & MVD_RENDER_KEEP_PROJECT) && M > 0) {
        hipLaunchKernelGGL(mesh_project_kernel, dim3((unsigned)((M + MR_THREADS - 1) / MR_THREADS), V), dim3(MR_THREADS), 0, st, vertices,
                           M, matrices, near_plane, records);
    }
    if (!(flags & MVD_RENDER_KEEP_KEYS)) {
        if (hipMemsetAsync(keys, 0xff, (size_t)pixels * sizeof(unsigned long long), st) != hipSuccess) return launch_status("mesh_render");
        if (n > 0) {
            const unsigned nwg = compact_workgroups(n);
            if (skip) {
                hipLaunchKernelGGL(mesh_setup_kernel<true>, dim3(nwg), dim3(CP_THREADS), 0, st, triangles, T, M, records, g, n, cull,
                                   max_small, keys, flag, sums);
            } else {
                hipLaunchKernelGGL(mesh_setup_kernel<false>, dim3(nwg), dim3(CP_THREADS), 0, st, triangles, T, M, records, g, n, cull,
                                   max_small, keys, flag, sums);
            }
            compact_scan_blocks(sums, n, block, total, st);
            hipLaunchKernelGGL(mesh_list_kernel, dim3(nwg), dim3(CP_THREADS), 0, st, flag, sums, n, list, slices);
            // the list's length stays on the device: every wave reads it and strides over the list
            const unsigned wgs = (unsigned)min((long long)MR_LARGE_WGS, (n + MR_THREADS / 64 - 1) / (MR_THREADS / 64));
            if (skip) {
                hipLaunchKernelGGL(mesh_large_kernel<true>, dim3(wgs, MR_SLICES), dim3(MR_THREADS), 0, st, triangles, T, M, records, g, cull,
                                   list, slices, total, keys);
            } else {
                hipLaunchKernelGGL(mesh_large_kernel<false>, dim3(wgs, MR_SLICES), dim3(MR_THREADS), 0, st, triangles, T, M, records, g,
                                   cull, list, slices, total, keys);
            }
        }
    }
    if (!(flags & MVD_RENDER_NO_RESOLVE)) {
        const MeshMaps maps{depth, triangle, bary, out_colors, normals};
        const long long groups = (pixels + MR_PIX - 1) / MR_PIX;
        hipLaunchKernelGGL(mesh_resolve_kernel, dim3((unsigned)((groups + MR_THREADS - 1) / MR_THREADS)), dim3(MR_THREADS), 0, st, keys,
                           triangles, T, M, records, vertices, colors, g, pixels, cull, maps);
    }
    return launch_status("mesh_render");
}
