// TSDF volume fusion and mesh extraction: the views' depth maps averaged into a truncated signed distance volume, and that volume's
// surface as a triangle mesh by marching tetrahedra.  The reference has NO counterpart, so there is no file:line to cite: the
// definition is the comment of these entries in include/mvd.h, restated in float64 numpy by robustmvd_amd/tsdf.py (integrate_numpy,
// extract_numpy).
//   mvd_tsdf_integrate_f32   up to MVD_MAX_VIEWS views into the volume in one launch: the state is read once, kept in registers across
//                            the views and written once, and only where a view updated it
//   mvd_tsdf_extract_f32     classification (per voxel: the 7-bit mask of its vertex-bearing edges and its cell's triangle count, one
//                            byte each, and the chunk sums of both), compact.h's two-level scan over the two sums, emission of the vertices,
//                            colours and triangles into their exact positions
// No atomics anywhere: a voxel belongs to one lane, a slot to one element.  Two calls give the same bits.
#include "compact.h"
#include "tsdf_tables.h"

namespace mvd {

__device__ __forceinline__ bool tsdf_positive_finite(float f) { return f > 0.f && finite_f32(f); }

// ---- integration -------------------------------------------------------------------------------------------------------------------
// One lane owns TI_VOX voxels that are consecutive in the linear index (k ny + j) nx + i, so consecutive lanes run along x: their state
// is one dense stream, read and written as 16-byte vectors whatever nx is (the group may run over the end of a row; each voxel gets
// its own (i,j,k) by integer carry), and their projections are neighbours in every depth map.  The last group of a volume whose size
// is no multiple of four goes through scalar loads and stores, as do the colour planes when their offsets N, 2N are not 16-byte
// multiples.  Per view the matrix comes from scalar loads (v is wave-uniform) and (Qx,Qy,Qz) from the integer indices directly.  A
// wave none of whose voxels projects into a view's image skips that view's gathers and updates (the ballot below).
// The update chain of one voxel is the same instructions whatever V is: V views in one launch give the bits of V launches of one.
constexpr int TI_THREADS = 256;
constexpr int TI_VOX = 4;

__global__ void __launch_bounds__(TI_THREADS) tsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                                    float* __restrict__ color, int nx, int ny, long long N,
                                                                    ViewPtrs depth, ViewPtrs wmap, ViewPtrs image,
                                                                    const float* __restrict__ mats, int V, int H, int W, float trunc,
                                                                    float max_weight, int has_wmap, int has_image) {
    const long long p0 = ((long long)blockIdx.x * TI_THREADS + threadIdx.x) * TI_VOX;
    if (p0 >= N) return;  // the ballot below counts the lanes that are left
    const int cnt = (int)min((long long)TI_VOX, N - p0);
    const bool vec = cnt == TI_VOX, vec_c = vec && (N & 3) == 0;

    float F[TI_VOX], Wt[TI_VOX], C[3][TI_VOX];
    if (vec) {
        const float4 f = *reinterpret_cast<const float4*>(tsdf + p0), w = *reinterpret_cast<const float4*>(weight + p0);
        F[0] = f.x, F[1] = f.y, F[2] = f.z, F[3] = f.w;
        Wt[0] = w.x, Wt[1] = w.y, Wt[2] = w.z, Wt[3] = w.w;
    } else {
#pragma unroll
        for (int e = 0; e < TI_VOX; ++e) {
            F[e] = e < cnt ? tsdf[p0 + e] : 0.f;
            Wt[e] = e < cnt ? weight[p0 + e] : 0.f;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (has_image && vec_c) {
            const float4 v = *reinterpret_cast<const float4*>(color + c * N + p0);
            C[c][0] = v.x, C[c][1] = v.y, C[c][2] = v.z, C[c][3] = v.w;
        } else {
#pragma unroll
            for (int e = 0; e < TI_VOX; ++e) C[c][e] = has_image && e < cnt ? color[c * N + p0 + e] : 0.f;
        }
    }

    float fi[TI_VOX], fj[TI_VOX], fk[TI_VOX];
    {
        const int row = (int)(p0 / nx);  // N < 2^31: 32-bit divisions
        int i = (int)p0 - row * nx, k = row / ny, j = row - k * ny;
#pragma unroll
        for (int e = 0; e < TI_VOX; ++e) {
            fi[e] = (float)i, fj[e] = (float)j, fk[e] = (float)k;
            if (++i == nx) {
                i = 0;
                if (++j == ny) j = 0, ++k;
            }
        }
    }

    const float inv_trunc = 1.0f / trunc, xmax = (float)(W - 1), ymax = (float)(H - 1);
    const long long HW = (long long)H * W;
    unsigned touched = 0u;
    for (int v = 0; v < V; ++v) {
        const float* __restrict__ m = mats + 12 * v;
        bool in[TI_VOX], any = false;
        int pix[TI_VOX];
        float qz[TI_VOX];
#pragma unroll
        for (int e = 0; e < TI_VOX; ++e) {
            const float qx = fmaf(m[0], fi[e], fmaf(m[1], fj[e], fmaf(m[2], fk[e], m[3])));
            const float qy = fmaf(m[4], fi[e], fmaf(m[5], fj[e], fmaf(m[6], fk[e], m[7])));
            qz[e] = fmaf(m[8], fi[e], fmaf(m[9], fj[e], fmaf(m[10], fk[e], m[11])));
            const float r = __builtin_amdgcn_rcpf(qz[e]);  // 1 ulp: one more rounding of u and v, which the tests' bands allow for
            const float px = rintf(qx * r), py = rintf(qy * r);  // half to even
            // a NaN fails every comparison
            in[e] = e < cnt && qz[e] > 0.f && px >= 0.f && px <= xmax && py >= 0.f && py <= ymax;
            pix[e] = in[e] ? (int)py * W + (int)px : 0;  // a lane outside reads pixel 0, which exists
            any = any || in[e];
        }
        if (__ballot(any) == 0ull) continue;  // wave-uniform
        const float* __restrict__ d = depth.p[v];
        const float* __restrict__ w = wmap.p[v];
        const float* __restrict__ im = image.p[v];
        float dm[TI_VOX], wm[TI_VOX], cm[3][TI_VOX];
#pragma unroll
        for (int e = 0; e < TI_VOX; ++e) {
            dm[e] = d[pix[e]];
            wm[e] = has_wmap ? w[pix[e]] : 1.0f;
            if (has_image) {
#pragma unroll
                for (int c = 0; c < 3; ++c) cm[c][e] = im[c * HW + pix[e]];
            }
        }
#pragma unroll
        for (int e = 0; e < TI_VOX; ++e) {
            const float sdf = dm[e] - qz[e];
            if (in[e] && tsdf_positive_finite(dm[e]) && tsdf_positive_finite(wm[e]) && sdf >= -trunc) {
                const float f = fminf(1.0f, sdf * inv_trunc);
                const float Wn = Wt[e] + wm[e];
                F[e] = (F[e] * Wt[e] + f * wm[e]) / Wn;
                if (has_image) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) C[c][e] = (C[c][e] * Wt[e] + cm[c][e] * wm[e]) / Wn;
                }
                Wt[e] = max_weight > 0.f ? fminf(Wn, max_weight) : Wn;
                touched |= 1u << e;
            }
        }
    }

    if (!touched) return;  // a group no view updated is not stored
    if (vec) {  // the voxels of the group that no view updated get the bits they had
        *reinterpret_cast<float4*>(tsdf + p0) = make_float4(F[0], F[1], F[2], F[3]);
        *reinterpret_cast<float4*>(weight + p0) = make_float4(Wt[0], Wt[1], Wt[2], Wt[3]);
    } else {
#pragma unroll
        for (int e = 0; e < TI_VOX; ++e) {
            if ((touched >> e) & 1u) tsdf[p0 + e] = F[e], weight[p0 + e] = Wt[e];
        }
    }
    if (!has_image) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (vec_c) {
            *reinterpret_cast<float4*>(color + c * N + p0) = make_float4(C[c][0], C[c][1], C[c][2], C[c][3]);
        } else {
#pragma unroll
            for (int e = 0; e < TI_VOX; ++e) {
                if ((touched >> e) & 1u) color[c * N + p0 + e] = C[c][e];
            }
        }
    }
}

// ---- extraction: classification ----------------------------------------------------------------------------------------------------
// Corner c = dx | dy << 1 | dz << 2 of the cell of voxel p.  A lane loads tsdf and weight of its own voxel and of the three voxels above it
// in y, z and yz (8 loads) and forms their observed and inside bits; the four corners at x + 1 are the lane above's own four (one
// shuffle), which lane 63 loads itself.  Edge kind q ends at corner TSDF_KIND_CORNER(q).
struct TsdfGrid {
    int nx, ny, nz;
    long long N;
    __device__ long long row(long long p, int r) const { return p + (r & 1 ? nx : 0) + (r & 2 ? (long long)nx * ny : 0); }
};

// observed bits 0..3 and inside bits 4..7 of the voxels p + (0, dy, dz), r = dy | dz << 1; a voxel outside the grid is unobserved
__device__ __forceinline__ unsigned tsdf_column_bits(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsdfGrid& g,
                                                     long long p, bool ey, bool ez, float min_weight) {
    unsigned bits = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool there = (!(r & 1) || ey) && (!(r & 2) || ez);
        const long long q = there ? g.row(p, r) : p;
        const float f = tsdf[q], w = weight[q];
        bits |= (there && w >= min_weight ? 1u : 0u) << r;
        bits |= (f < 0.f ? 1u : 0u) << (4 + r);
    }
    return bits;
}

// columns (own, x + 1) -> bit c of the result: corner c is observed; bit 8 + c: it is inside
__device__ __forceinline__ unsigned tsdf_corner_bits(unsigned own, unsigned next) {
    unsigned out = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        out |= ((own >> r) & 1u) << (2 * r) | ((next >> r) & 1u) << (2 * r + 1);
        out |= ((own >> (4 + r)) & 1u) << (8 + 2 * r) | ((next >> (4 + r)) & 1u) << (9 + 2 * r);
    }
    return out;
}

__device__ __forceinline__ int tsdf_kind_corner(int q) { return q < 3 ? 1 << q : q + (q > 3); }  // kinds 0..6 -> 1 2 4 3 5 6 7

// the inside mask of tetrahedron t from the corners' inside bits: v0 = corner 0, v1 = e_a, v2 = e_a + e_b, v3 = corner 7
__device__ __forceinline__ unsigned tsdf_tetra_mask(unsigned ins, int t) {
    constexpr int v1[6] = {1, 1, 2, 2, 4, 4}, v2[6] = {3, 5, 3, 6, 5, 6};  // (a,b,c) in lexicographic order
    return (ins & 1u) | ((ins >> v1[t]) & 1u) << 1 | ((ins >> v2[t]) & 1u) << 2 | ((ins >> 7) & 1u) << 3;
}

__device__ __forceinline__ unsigned tsdf_case_triangles(unsigned m) {
    const int n = __popc(m);
    return n == 2 ? 2u : (n == 0 || n == 4) ? 0u : 1u;
}

__global__ void __launch_bounds__(CP_THREADS) tsdf_classify_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                   TsdfGrid g, float min_weight, unsigned char* __restrict__ vmask,
                                                                   unsigned char* __restrict__ tcount, unsigned* __restrict__ vsums,
                                                                   unsigned* __restrict__ tsums) {
    const int lane = threadIdx.x & 63;
    const long long chunk = compact_wave_chunk();
    if (chunk * CP_CHUNK >= g.N) return;  // the whole wave
    unsigned nv[CP_SUB], nt[CP_SUB];
#pragma unroll
    for (int s = 0; s < CP_SUB; ++s) {
        const long long p = chunk * CP_CHUNK + 64 * s + lane;
        const bool live = p < g.N;
        const long long pc = live ? p : g.N - 1;  // a lane past the end classifies the last voxel and stores nothing
        const int row = (int)(pc / g.nx);
        const int i = (int)pc - row * g.nx, k = row / g.ny, j = row - k * g.ny;
        const bool ex = i + 1 < g.nx, ey = j + 1 < g.ny, ez = k + 1 < g.nz;
        // an unobserved voxel owns no vertex and its cell no triangle: 64 of them in a row (empty space, most of a volume) cost one load each
        if (__ballot(weight[pc] >= min_weight) == 0ull) {  // wave-uniform
            if (live) vmask[p] = 0, tcount[p] = 0;
            nv[s] = nt[s] = 0u;
            continue;
        }
        const unsigned own = tsdf_column_bits(tsdf, weight, g, pc, ey, ez, min_weight);
        unsigned next = __shfl_down(own, 1);  // lane + 1 holds voxel p + 1
        if (lane == 63 && ex) next = tsdf_column_bits(tsdf, weight, g, pc + 1, ey, ez, min_weight);
        if (!ex) next = 0u;
        const unsigned corners = tsdf_corner_bits(own, next), obs = corners & 0xffu, ins = corners >> 8;
        unsigned mask = 0u, tris = 0u;
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            const int c = tsdf_kind_corner(q);
            if ((obs & 1u) && ((obs >> c) & 1u) && (((ins >> c) ^ ins) & 1u)) mask |= 1u << q;
        }
        if (obs == 0xffu) {  // which needs ex, ey and ez
#pragma unroll
            for (int t = 0; t < 6; ++t) tris += tsdf_case_triangles(tsdf_tetra_mask(ins, t));
        }
        if (live) {
            vmask[p] = (unsigned char)mask;
            tcount[p] = (unsigned char)tris;
        }
        nv[s] = live ? (unsigned)__popc(mask) : 0u;
        nt[s] = live ? tris : 0u;
    }
    compact_store_chunk_sum(nv, g.N, vsums);
    compact_store_chunk_sum(nt, g.N, tsums);
}

// ---- extraction: emission ----------------------------------------------------------------------------------------------------------
struct TsdfVertexCount {
    const unsigned char* vmask;
    __device__ unsigned operator()(long long p) const { return (unsigned)__popc((unsigned)vmask[p]); }
};
struct TsdfTriangleCount {
    const unsigned char* tcount;
    __device__ unsigned operator()(long long p) const { return tcount[p]; }
};

// The index of the first vertex of voxel q: its chunk's offset plus the vertices of the chunk's earlier voxels, a prefix over their byte
// masks read as 16-byte vectors (a mask has 7 bits, so the popcount of a word is the sum of its bytes' counts).  vmask is 16-byte
// aligned and padded to whole chunks.
__device__ __forceinline__ unsigned tsdf_popc128(uint4 w) { return __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w); }

__device__ __forceinline__ long long tsdf_vertex_base(const unsigned char* __restrict__ vmask, const unsigned* __restrict__ voffs,
                                                      long long q) {
    const long long start = q & ~(long long)(CP_CHUNK - 1);
    const int n = (int)(q - start);
    const uint4* __restrict__ words = reinterpret_cast<const uint4*>(vmask + start);
    unsigned sum = 0u;
    for (int b = 0; b < (n >> 4); ++b) sum += tsdf_popc128(words[b]);
    const int rem = n & 15;
    if (rem) {
        const uint4 w = words[n >> 4];
        const unsigned long long lo = (unsigned long long)w.y << 32 | w.x, hi = (unsigned long long)w.w << 32 | w.z;
        // the first rem bytes
        sum += rem >= 8 ? __popcll(lo) + (rem > 8 ? __popcll(hi & ((1ull << (8 * (rem - 8))) - 1ull)) : 0)
                        : __popcll(lo & ((1ull << (8 * rem)) - 1ull));
    }
    return (long long)voffs[q >> 8] + sum;
}
static_assert(CP_CHUNK == 256, "tsdf_vertex_base: q >> 8 is the chunk");

__global__ void __launch_bounds__(CP_THREADS) tsdf_emit_kernel(const float* __restrict__ tsdf, const float* __restrict__ color, TsdfGrid g,
                                                               float ox, float oy, float oz, float s,
                                                               const unsigned char* __restrict__ vmask,
                                                               const unsigned char* __restrict__ tcount,
                                                               const unsigned* __restrict__ voffs, const unsigned* __restrict__ toffs,
                                                               float* __restrict__ vertices, float* __restrict__ colors,
                                                               int* __restrict__ triangles, long long max_vertices,
                                                               long long max_triangles) {
    const long long plane = (long long)g.nx * g.ny;
    compact_walk_counted(TsdfVertexCount{vmask}, voffs, g.N, [&](long long p, long long slot, unsigned) {
        const unsigned mask = vmask[p];
        const int row = (int)(p / g.nx);
        const int i = (int)p - row * g.nx, k = row / g.ny, j = row - k * g.ny;
        const float fa = tsdf[p];
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            if (!((mask >> q) & 1u)) continue;
            const int c = tsdf_kind_corner(q);
            const long long other = p + (c & 1) + (c & 2 ? g.nx : 0) + (c & 4 ? plane : 0);
            if (other >= g.N) continue;  // never with this volume's own classification; a stale workspace must not read outside
            const float fb = tsdf[other];
            const float t = fa / (fa - fb);  // exactly one of the two is < 0: the difference is not zero
            if (slot < max_vertices) {
                float* o = vertices + 3 * slot;
                o[0] = ox + s * ((float)i + t * (float)(c & 1));
                o[1] = oy + s * ((float)j + t * (float)((c >> 1) & 1));
                o[2] = oz + s * ((float)k + t * (float)((c >> 2) & 1));
                if (colors) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float ca = color[ch * g.N + p], cb = color[ch * g.N + other];
                        colors[3 * slot + ch] = ca + t * (cb - ca);
                    }
                }
            }
            ++slot;
        }
    });
    compact_walk_counted(TsdfTriangleCount{tcount}, toffs, g.N, [&](long long p, long long slot, unsigned) {
        // a cell with triangles has all eight corners in the grid; a stale workspace must not make a lane read outside it
        if (g.row(p, 3) + 1 >= g.N) return;
        unsigned ins = 0u;
        unsigned long long masks = 0ull;  // byte c: the vertex mask of corner c
        long long base[4];                // the first vertex of the voxel at (0, dy, dz)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long q = g.row(p, r);
            ins |= (tsdf[q] < 0.f ? 1u : 0u) << (2 * r) | (tsdf[q + 1] < 0.f ? 1u : 0u) << (2 * r + 1);
            masks |= ((unsigned long long)vmask[q] | (unsigned long long)vmask[q + 1] << 8) << (16 * r);
            base[r] = tsdf_vertex_base(vmask, voffs, q);
        }
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const unsigned m = tsdf_tetra_mask(ins, t), n = tsdf_case_triangles(m);
            for (unsigned k = 0; k < n; ++k, ++slot) {
                const unsigned word = TSDF_TRI[t][m][k];
                if (slot >= max_triangles) continue;
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const unsigned code = (word >> (6 * e)) & 63u, c = code & 7u, kind = code >> 3, r = c >> 1;
                    const long long rb = r == 0 ? base[0] : r == 1 ? base[1] : r == 2 ? base[2] : base[3];
                    // the voxel at x + 1 starts where the vertices of the one at x end
                    const unsigned before = c & 1u ? (unsigned)__popc((unsigned)(masks >> (16 * r)) & 0x7fu) : 0u;
                    const unsigned mine = (unsigned)(masks >> (8 * c)) & 0xffu;
                    triangles[3 * slot + e] = (int)(rb + before + __popc(mine & ((1u << kind) - 1u)));
                }
            }
        }
    });
}

static size_t tsdf_bytes_per_map(long long N) { return align_up((size_t)N, CP_CHUNK); }

}  // namespace mvd

extern "C" int mvd_tsdf_integrate_f32(float* tsdf, float* weight, float* color, int nx, int ny, int nz, const float* const* depth,
                                      const float* const* weight_maps, const float* const* images, const float* matrices, int V, int H,
                                      int W, float trunc, float max_weight, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(tsdf && weight && depth && matrices, "tsdf_integrate: NULL argument");
    MVD_REQUIRE(V >= 1 && V <= MVD_MAX_VIEWS, "tsdf_integrate: %d views, supported 1..%d", V, MVD_MAX_VIEWS);
    MVD_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL, "tsdf_integrate: bad map size %d x %d", H, W);
    MVD_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "tsdf_integrate: bad volume %d x %d x %d", nx, ny, nz);
    const long long N = (long long)nx * ny * nz;
    MVD_REQUIRE(N <= 0x7fffffffLL, "tsdf_integrate: nx ny nz = %lld must be below 2^31", N);
    MVD_REQUIRE(trunc > 0.f, "tsdf_integrate: trunc must be positive");
    MVD_REQUIRE((((uintptr_t)tsdf | (uintptr_t)weight | (uintptr_t)color) & 15) == 0,
                "tsdf_integrate: tsdf, weight and color must be 16-byte aligned");
    ViewPtrs d{}, w{}, im{};
    const bool has_image = color && images;
    for (int v = 0; v < V; ++v) {
        MVD_REQUIRE(depth[v], "tsdf_integrate: depth[%d] is NULL", v);
        MVD_REQUIRE(!weight_maps || weight_maps[v], "tsdf_integrate: weight_maps[%d] is NULL", v);
        MVD_REQUIRE(!has_image || images[v], "tsdf_integrate: images[%d] is NULL", v);
        d.p[v] = depth[v];
        if (weight_maps) w.p[v] = weight_maps[v];
        if (has_image) im.p[v] = images[v];
    }
    const long long groups = (N + TI_VOX - 1) / TI_VOX;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((groups + TI_THREADS - 1) / TI_THREADS)), dim3(TI_THREADS), 0,
                       (hipStream_t)stream, tsdf, weight, color, nx, ny, N, d, w, im, matrices, V, H, W, trunc, max_weight,
                       weight_maps ? 1 : 0, has_image ? 1 : 0);
    return launch_status("tsdf_integrate");
}

extern "C" size_t mvd_tsdf_extract_workspace_bytes(int nx, int ny, int nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
    const long long N = (long long)nx * ny * nz;
    // the two chunk-sum arrays, the totals, the block sums of the two-level scan, the vertex masks, the triangle counts
    return 2 * mvd::compact_offsets_bytes(N) + 256 + mvd::compact_block_bytes(N) + 2 * mvd::tsdf_bytes_per_map(N);
}

extern "C" int mvd_tsdf_extract_f32(const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, float origin_x,
                                    float origin_y, float origin_z, float voxel, float min_weight, int classified, float* vertices,
                                    float* colors, int* triangles, long long max_vertices, long long max_triangles, long long* counts,
                                    void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(tsdf && weight && counts, "tsdf_extract: NULL argument");
    MVD_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "tsdf_extract: bad volume %d x %d x %d", nx, ny, nz);
    const long long N = (long long)nx * ny * nz;
    MVD_REQUIRE(N <= 0x7fffffffLL, "tsdf_extract: nx ny nz = %lld must be below 2^31", N);
    MVD_REQUIRE(!vertices == !triangles, "tsdf_extract: vertices and triangles go together");
    MVD_REQUIRE(!colors || (color && vertices), "tsdf_extract: colors needs color and vertices");
    MVD_REQUIRE(!vertices || (max_vertices >= 0 && max_triangles >= 0 && max_vertices <= 0x7fffffffLL && max_triangles <= 0x7fffffffLL),
                "tsdf_extract: max_vertices and max_triangles must be in 0 .. 2^31 - 1");
    MVD_REQUIRE(((uintptr_t)counts & 15) == 0, "tsdf_extract: counts must be 16-byte aligned");
    MVD_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= mvd_tsdf_extract_workspace_bytes(nx, ny, nz),
                "tsdf_extract: workspace too small or not 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    unsigned* voffs = reinterpret_cast<unsigned*>(ws);
    unsigned* toffs = reinterpret_cast<unsigned*>(ws + compact_offsets_bytes(N));
    long long* totals = reinterpret_cast<long long*>(ws + 2 * compact_offsets_bytes(N));
    unsigned* block = reinterpret_cast<unsigned*>(ws + 2 * compact_offsets_bytes(N) + 256);
    unsigned char* vmask = ws + 2 * compact_offsets_bytes(N) + 256 + compact_block_bytes(N);
    unsigned char* tcount = vmask + tsdf_bytes_per_map(N);
    const TsdfGrid g{nx, ny, nz, N};
    const unsigned nwg = compact_workgroups(N);
    if (!classified) {
        hipLaunchKernelGGL(tsdf_classify_kernel, dim3(nwg), dim3(CP_THREADS), 0, st, tsdf, weight, g, min_weight, vmask, tcount, voffs,
                           toffs);
        // a 512^3 volume has 524,288 chunks: the two-level scan (compact_scan_kernel over the block sums)
        compact_scan_blocks(voffs, N, block, totals, st);
        compact_scan_blocks(toffs, N, block, totals + 1, st);
    }
    if (hipMemcpyAsync(counts, totals, 2 * sizeof(long long), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return launch_status("tsdf_extract");
    if (vertices) {
        hipLaunchKernelGGL(tsdf_emit_kernel, dim3(nwg), dim3(CP_THREADS), 0, st, tsdf, color, g, origin_x, origin_y, origin_z, voxel,
                           vmask, tcount, voffs, toffs, vertices, colors, triangles, max_vertices, max_triangles);
    }
    return launch_status("tsdf_extract");
}
