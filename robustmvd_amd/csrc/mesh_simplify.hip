// Mesh simplification by vertex clustering with quadric placement (mesh_simplify.py is the definition).
//   mvd_mesh_cluster_ids           from the vertices' sorted cell keys: every vertex's cluster, the clusters' segments and keys (compact.h)
//   mvd_mesh_cluster_means_f64     the float64 mean of every cluster's rows of a per-vertex array (fixed_sums.h's segment order)
//   mvd_mesh_cluster_triples       per triangle the rotated cluster triple, the alive byte and the three corner keys
//   mvd_mesh_cluster_quadrics_f64  from the corners sorted by cluster: every cluster's ten quadric sums, float64 (the same order)
//   mvd_mesh_cluster_place_f32     one lane per cluster: the regularised 3 x 3 solve, or the mean, or the single vertex
//   mvd_mesh_cluster_mark_first    from the triples sorted lexicographically: the first triangle of every run of equal triples
// The kept triangles and the referenced clusters are then compacted by mvd_mesh_filter, and the rows moved by
// mvd_mesh_gather_rows_f32 (mesh_clean.hip).
// What bounds each kernel: every one is a straight pass with a trip count fixed by its arguments; none waits for another thread.
// No atomic anywhere; every float64 sum has the order of fixed_sums.h's segment walk, which the segment's length alone fixes, and the
// library is built without contraction: two runs, and tests/sum_order.py's numpy, give the same bits.
// Every index read from an argument (a permutation entry, a triangle's vertex, a cluster id, a segment bound) is checked against
// its array's size before it is used as an address.
#include "cloud_grid.h"
#include "compact.h"
#include "fixed_sums.h"

namespace mvd {

constexpr int MS_THREADS = 256;
static_assert(MS_THREADS == FS_THREADS && MS_THREADS == CP_THREADS, "the kernels are launched as fixed_sums.h and compact.h expect");

static inline unsigned ms_blocks(long long n) { return (unsigned)((n + MS_THREADS - 1) / MS_THREADS); }

// fixed_sums.h's segment walk as two launches, each half in the walk's own order, so that a long segment has a wave of its own.  In
// the walk a wave owns 64 consecutive segments and adds its long ones one after the other: with a few thousand clusters of hundreds of
// corners each, a few hundred waves carried the whole mesh (profiles/mesh_simplify.txt).  segment_short: one lane per segment of at
// most FS_LONG items, the items in order; launch FS_THREADS threads per 256 segments.  segment_long: one wave per segment of more,
// lane l the items l, l + 64, ... in order, then the wave sum; launch FS_THREADS threads per FS_WAVES segments, and every lane of a
// wave must call it.  seg as in fixed_segment_walk: ascending, clamped into 0 .. n.
template <int N, class Item, class Store>
__device__ __forceinline__ void segment_short(const int* __restrict__ seg, long long nseg, int n, const Item& item, const Store& store) {
    const long long c = (long long)blockIdx.x * FS_THREADS + threadIdx.x;
    if (c >= nseg) return;
    const int b = min(max(seg[c], 0), n), e = min(max(seg[c + 1], b), n);
    if (e - b > FS_LONG) return;
    FixedSums<N> s{};
    for (int p = b; p < e; ++p) item(s, p);
    store(s, e - b, c);
}

template <int N, class Item, class Store>
__device__ __forceinline__ void segment_long(const int* __restrict__ seg, long long nseg, int n, const Item& item, const Store& store) {
    const long long c = (long long)blockIdx.x * FS_WAVES + (threadIdx.x >> 6);  // wave-uniform
    if (c >= nseg) return;
    const int b = min(max(seg[c], 0), n), e = min(max(seg[c + 1], b), n);
    if (e - b <= FS_LONG) return;
    FixedSums<N> s{};
    fixed_lane_span(s, b, e, threadIdx.x & 63, item);
#pragma unroll
    for (int k = 0; k < N; ++k) s.v[k] = fixed_wave_sum(s.v[k]);
    if ((threadIdx.x & 63) == 0) store(s, e - b, c);
}

// ---- cluster ids -----------------------------------------------------------------------------------------------------------------------
// Position p of the sorted keys is the head of a cluster's segment when its key is a valid vertex's and differs from the key before
// it: cloud_eval.hip's VoxelHead, compacted as there.
struct ClusterHead {
    const long long* keys;
    __device__ bool operator()(long long p) const {
        const long long k = keys[p];
        return k != CE_INVALID_KEY && (p == 0 || keys[p - 1] != k);
    }
};

// compact_walk with the inclusive rank kept for every position, not only for the heads: the number of heads at or before p, less
// one, is p's cluster.  The last valid position closes the last segment.
__global__ void __launch_bounds__(CP_THREADS) cluster_ids_kernel(const long long* __restrict__ keys, const long long* __restrict__ perm,
                                                                 int n, const unsigned* __restrict__ offsets,
                                                                 const long long* __restrict__ total, int* __restrict__ vertex_cluster,
                                                                 int* __restrict__ seg, long long* __restrict__ cluster_key) {
    const int lane = threadIdx.x & 63;
    const long long chunk = compact_wave_chunk();
    if (chunk * CP_CHUNK >= n) return;  // the whole wave
    const ClusterHead head{keys};
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);  // the lanes at or below this one
    long long run = offsets[chunk];
#pragma unroll
    for (int k = 0; k < CP_SUB; ++k) {
        const long long p = chunk * CP_CHUNK + 64 * k + lane;
        const bool in = p < n;
        const long long key = in ? keys[p] : CE_INVALID_KEY;
        const bool h = in && head(p);
        const unsigned long long ballot = __ballot(h);
        const long long id = run + __popcll(ballot & upto) - 1;  // 0 .. n-1 for a valid key: a head is at or before it
        if (in) {
            const long long v = perm[p];
            if ((unsigned long long)v < (unsigned long long)n) vertex_cluster[v] = key != CE_INVALID_KEY && id >= 0 ? (int)id : -1;
        }
        if (h) {
            seg[id] = (int)p;
            cluster_key[id] = key;
        }
        if (in && key != CE_INVALID_KEY && (p + 1 == n || keys[p + 1] == CE_INVALID_KEY)) seg[min(total[0], (long long)n)] = (int)(p + 1);
        run += __popcll(ballot);
    }
}

// ---- means -----------------------------------------------------------------------------------------------------------------------------
// N columns c0 .. c0 + N - 1 of rows of k float32: one lane per cluster walks its vertices in sorted (= ascending vertex) order
// (LONG false), one wave a cluster of more than 64 (LONG true).
template <int N, bool LONG>
__global__ void __launch_bounds__(FS_THREADS) cluster_means_kernel(const float* __restrict__ rows, int M, int k, int c0,
                                                                   const long long* __restrict__ perm, const int* __restrict__ seg, int K,
                                                                   double* __restrict__ out) {
    const auto add = [&](FixedSums<N>& s, long long pos) {
        const long long v = perm[pos];
        if ((unsigned long long)v >= (unsigned long long)M) return;  // not a permutation of 0 .. M-1: skipped, never dereferenced
#pragma unroll
        for (int j = 0; j < N; ++j) s.v[j] += (double)rows[v * k + c0 + j];
    };
    const auto store = [&](const FixedSums<N>& s, int len, long long c) {
        const double nd = (double)len;
#pragma unroll
        for (int j = 0; j < N; ++j) out[c * k + c0 + j] = s.v[j] / nd;
    };
    if constexpr (LONG) segment_long<N>(seg, K, M, add, store); else segment_short<N>(seg, K, M, add, store);
}

// ---- triples ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MS_THREADS) cluster_triples_kernel(const int* __restrict__ tri, int T, int M,
                                                                     const int* __restrict__ vertex_cluster, int K, int* __restrict__ triples,
                                                                     unsigned char* __restrict__ alive, int* __restrict__ corner_key) {
    const long long t = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    if (t >= T) return;
    int c[3];
    bool valid = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int i = tri[3 * t + j];
        c[j] = (unsigned)i < (unsigned)M ? vertex_cluster[i] : -1;
        valid = valid && (unsigned)c[j] < (unsigned)K;
    }
    const bool live = valid && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
    const int first = c[0] < c[1] ? (c[0] < c[2] ? 0 : 2) : (c[1] < c[2] ? 1 : 2);  // the smallest of three different ones
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int s = first + j >= 3 ? first + j - 3 : first + j;
        triples[3 * t + j] = live ? (s == 0 ? c[0] : s == 1 ? c[1] : c[2]) : -1;
        corner_key[3 * t + j] = valid ? c[j] : K;  // a dropped triangle's corners sort last
    }
    alive[t] = live ? 1 : 0;
}

// ---- quadrics --------------------------------------------------------------------------------------------------------------------------
// seg[k] = the first sorted position whose key is >= k, k = 0 .. K: a cluster without a corner gets an empty segment, and whatever
// the keys hold every bound lies in 0 .. n.
__global__ void __launch_bounds__(MS_THREADS) corner_segments_kernel(const int* __restrict__ key, int n, int K, int* __restrict__ seg) {
    const long long k = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    if (k > K) return;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (key[mid] < (int)k) lo = mid + 1; else hi = mid;
    }
    seg[k] = lo;
}

__device__ __forceinline__ double cell_centre(long long idx, double c, double o) { return ((double)idx + 0.5) * c + o; }

// Sorted position p holds corner perm[p] = 3 t + j of cluster key[p].  One lane per cluster walks its corners in order (LONG false),
// one wave a cluster of more than 64 (LONG true): per corner the triangle's three indices and nine coordinates are read once, the cross product,
// the offset d and the ten products are formed in float64, about 45 float64 operations for 12 scattered 4-byte loads.
template <bool LONG>
__global__ void __launch_bounds__(FS_THREADS) cluster_quadrics_kernel(const float* __restrict__ vtx, int M, const int* __restrict__ tri, int T,
                                                                      const int* __restrict__ key, const long long* __restrict__ perm,
                                                                      const int* __restrict__ seg, const long long* __restrict__ cluster_key,
                                                                      int K, double ox, double oy, double oz, double c,
                                                                      double* __restrict__ quadric) {
    const int n = 3 * T;
    const auto add = [&](FixedSums<10>& s, long long pos) {
        const long long corner = perm[pos];
        const int cl = key[pos];
        if ((unsigned long long)corner >= (unsigned long long)n || (unsigned)cl >= (unsigned)K) return;
        const long long t = corner / 3;
        const int i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
        if ((unsigned)i0 >= (unsigned)M || (unsigned)i1 >= (unsigned)M || (unsigned)i2 >= (unsigned)M) return;
        const double ax = vtx[3 * (long long)i0], ay = vtx[3 * (long long)i0 + 1], az = vtx[3 * (long long)i0 + 2];
        const double e1x = (double)vtx[3 * (long long)i1] - ax, e1y = (double)vtx[3 * (long long)i1 + 1] - ay,
                     e1z = (double)vtx[3 * (long long)i1 + 2] - az;
        const double e2x = (double)vtx[3 * (long long)i2] - ax, e2y = (double)vtx[3 * (long long)i2 + 1] - ay,
                     e2z = (double)vtx[3 * (long long)i2 + 2] - az;
        const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const long long ck = cluster_key[cl];
        const double qx = ax - cell_centre(ck >> (2 * CE_BITS), c, ox), qy = ay - cell_centre((ck >> CE_BITS) & CE_LIMIT, c, oy),
                     qz = az - cell_centre(ck & CE_LIMIT, c, oz);
        const double d = -((nx * qx + ny * qy) + nz * qz);
        s.v[0] += nx * nx;
        s.v[1] += nx * ny;
        s.v[2] += nx * nz;
        s.v[3] += ny * ny;
        s.v[4] += ny * nz;
        s.v[5] += nz * nz;
        s.v[6] += nx * d;
        s.v[7] += ny * d;
        s.v[8] += nz * d;
        s.v[9] += d * d;
    };
    const auto store = [&](const FixedSums<10>& s, int, long long cl) {
#pragma unroll
        for (int j = 0; j < 10; ++j) quadric[10 * cl + j] = s.v[j];
    };
    if constexpr (LONG) segment_long<10>(seg, K, n, add, store); else segment_short<10>(seg, K, n, add, store);
}

// ---- placement -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ms_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for inf and NaN

__global__ void __launch_bounds__(MS_THREADS) cluster_place_kernel(const double* __restrict__ quadric, const double* __restrict__ mean,
                                                                   const int* __restrict__ seg, const long long* __restrict__ cluster_key,
                                                                   const long long* __restrict__ perm, const float* __restrict__ vtx, int K,
                                                                   int M, double ox, double oy, double oz, double c, double reg,
                                                                   float* __restrict__ out, unsigned char* __restrict__ placed) {
    const long long k = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    if (k >= K) return;
    const double m0 = mean[3 * k], m1 = mean[3 * k + 1], m2 = mean[3 * k + 2];
    float v0 = (float)m0, v1 = (float)m1, v2 = (float)m2;
    unsigned char how = 0;
    const int b = seg[k], e = seg[k + 1];
    const long long only = e - b == 1 && (unsigned)b < (unsigned)M ? perm[b] : -1;
    if ((unsigned long long)only < (unsigned long long)M) {
        v0 = vtx[3 * only];
        v1 = vtx[3 * only + 1];
        v2 = vtx[3 * only + 2];
        how = 2;
    } else if (quadric) {
        const double* q = quadric + 10 * k;
        const double a00 = q[0], a01 = q[1], a02 = q[2], a11 = q[3], a12 = q[4], a22 = q[5];
        const long long ck = cluster_key[k];
        const double c0 = cell_centre(ck >> (2 * CE_BITS), c, ox), c1 = cell_centre((ck >> CE_BITS) & CE_LIMIT, c, oy),
                     c2 = cell_centre(ck & CE_LIMIT, c, oz);
        const double lam = reg * ((a00 + a11) + a22);
        const double d00 = a00 + lam, d11 = a11 + lam, d22 = a22 + lam;
        const double r0 = -q[6] + lam * (m0 - c0), r1 = -q[7] + lam * (m1 - c1), r2 = -q[8] + lam * (m2 - c2);
        const double C00 = d11 * d22 - a12 * a12, C01 = a02 * a12 - a01 * d22, C02 = a01 * a12 - a02 * d11;
        const double C11 = d00 * d22 - a02 * a02, C12 = a01 * a02 - d00 * a12, C22 = d00 * d11 - a01 * a01;
        const double det = (d00 * C00 + a01 * C01) + a02 * C02;
        const double x0 = ((C00 * r0 + C01 * r1) + C02 * r2) / det, x1 = ((C01 * r0 + C11 * r1) + C12 * r2) / det,
                     x2 = ((C02 * r0 + C12 * r1) + C22 * r2) / det;
        const double half = 0.5 * c;
        if (lam > 0.0 && ms_finite(det) && det > 0.0 && ms_finite(x0) && ms_finite(x1) && ms_finite(x2) && fabs(x0) <= half &&
            fabs(x1) <= half && fabs(x2) <= half) {
            v0 = (float)(c0 + x0);
            v1 = (float)(c1 + x1);
            v2 = (float)(c2 + x2);
            how = 1;
        }
    }
    out[3 * k] = v0;
    out[3 * k + 1] = v1;
    out[3 * k + 2] = v2;
    placed[k] = how;
}

// ---- duplicates ------------------------------------------------------------------------------------------------------------------------
// Sorted position p holds triangle perm[p]; the alive triples ascend lexicographically, equal ones in ascending triangle index (the
// sorts are stable).  A triangle is kept when it is alive and the position before it holds another triple or a dead triangle.
__global__ void __launch_bounds__(MS_THREADS) cluster_mark_first_kernel(const int* __restrict__ triples, const unsigned char* __restrict__ alive,
                                                                        const long long* __restrict__ perm, int T,
                                                                        unsigned char* __restrict__ keep) {
    const long long p = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    if (p >= T) return;
    const long long t = perm[p];
    if ((unsigned long long)t >= (unsigned long long)T) return;
    bool k = alive[t] != 0;
    if (k && p > 0) {
        const long long u = perm[p - 1];
        if ((unsigned long long)u < (unsigned long long)T && alive[u] != 0 && triples[3 * u] == triples[3 * t] &&
            triples[3 * u + 1] == triples[3 * t + 1] && triples[3 * u + 2] == triples[3 * t + 2])
            k = false;
    }
    keep[t] = k ? 1 : 0;
}

}  // namespace mvd

extern "C" size_t mvd_mesh_cluster_ids_workspace_bytes(long long M) {
    if (M <= 0) return 0;
    return mvd::compact_offsets_bytes(M) + mvd::compact_block_bytes(M);
}

extern "C" int mvd_mesh_cluster_ids(const long long* keys, const long long* perm, long long M, int* vertex_cluster, int* cluster_start,
                                    long long* cluster_key, long long* num_clusters, void* workspace, size_t workspace_bytes,
                                    mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_cluster_ids", "vertices", M);
    MVD_REQUIRE(num_clusters && ((uintptr_t)num_clusters & 7) == 0, "mesh_cluster_ids: num_clusters must be given and 8-byte aligned");
    MVD_REQUIRE(cluster_start && ((uintptr_t)cluster_start & 3) == 0, "mesh_cluster_ids: cluster_start must be given and 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    // no valid vertex: nobody closes a segment, and cluster_start is the one entry 0
    if (hipMemsetAsync(cluster_start, 0, sizeof(int), st) != hipSuccess) return launch_status("mesh_cluster_ids");
    if (M == 0) {
        if (hipMemsetAsync(num_clusters, 0, sizeof(long long), st) != hipSuccess) return launch_status("mesh_cluster_ids");
        return MVD_OK;
    }
    MVD_REQUIRE(keys && perm && vertex_cluster && cluster_key, "mesh_cluster_ids: NULL argument");
    MVD_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= mvd_mesh_cluster_ids_workspace_bytes(M),
                "mesh_cluster_ids: workspace too small or not 256-byte aligned");
    unsigned* chunk = static_cast<unsigned*>(workspace);
    unsigned* block = reinterpret_cast<unsigned*>(static_cast<unsigned char*>(workspace) + compact_offsets_bytes(M));
    const unsigned nwg = compact_workgroups(M);
    hipLaunchKernelGGL(compact_count_kernel<ClusterHead>, dim3(nwg), dim3(CP_THREADS), 0, st, ClusterHead{keys}, M, chunk);
    compact_scan_blocks(chunk, M, block, num_clusters, st);
    hipLaunchKernelGGL(cluster_ids_kernel, dim3(nwg), dim3(CP_THREADS), 0, st, keys, perm, (int)M, chunk, num_clusters, vertex_cluster,
                       cluster_start, cluster_key);
    return launch_status("mesh_cluster_ids");
}

namespace mvd {
static inline unsigned ms_wave_blocks(long long n) { return (unsigned)((n + FS_WAVES - 1) / FS_WAVES); }  // one wave per item

template <int N>
static void launch_cluster_means(hipStream_t st, const float* rows, int M, int k, int c0, const long long* perm, const int* seg, int K,
                                 double* means) {
    hipLaunchKernelGGL((cluster_means_kernel<N, false>), dim3(ms_blocks(K)), dim3(FS_THREADS), 0, st, rows, M, k, c0, perm, seg, K, means);
    hipLaunchKernelGGL((cluster_means_kernel<N, true>), dim3(ms_wave_blocks(K)), dim3(FS_THREADS), 0, st, rows, M, k, c0, perm, seg, K, means);
}
}  // namespace mvd

extern "C" int mvd_mesh_cluster_means_f64(const float* rows, const long long* perm, const int* cluster_start, long long K, long long M,
                                          int k, double* means, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_cluster_means", "vertices", M);
    MVD_REQUIRE(K >= 0 && K <= M, "mesh_cluster_means: %lld clusters of %lld vertices", K, M);
    MVD_REQUIRE(k >= 1 && k <= 65536, "mesh_cluster_means: %d columns, supported 1 .. 65536", k);
    MVD_REQUIRE(M * k <= 0x7fffffffLL, "mesh_cluster_means: M k = %lld values, supported up to 2^31 - 1", M * k);
    if (K == 0) return MVD_OK;
    MVD_REQUIRE(rows && perm && cluster_start && means, "mesh_cluster_means: NULL argument");
    MVD_REQUIRE(((uintptr_t)means & 7) == 0, "mesh_cluster_means: means must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    for (int c0 = 0; c0 < k;) {  // up to four columns per pass; a column's order does not depend on its pass
        const int left = k - c0, take = left >= 4 ? 4 : left;
        switch (take) {
            case 4: launch_cluster_means<4>(st, rows, (int)M, k, c0, perm, cluster_start, (int)K, means); break;
            case 3: launch_cluster_means<3>(st, rows, (int)M, k, c0, perm, cluster_start, (int)K, means); break;
            case 2: launch_cluster_means<2>(st, rows, (int)M, k, c0, perm, cluster_start, (int)K, means); break;
            default: launch_cluster_means<1>(st, rows, (int)M, k, c0, perm, cluster_start, (int)K, means); break;
        }
        c0 += take;
    }
    return launch_status("mesh_cluster_means");
}

extern "C" int mvd_mesh_cluster_triples(const int* triangles, long long T, long long M, const int* vertex_cluster, long long K, int* triples,
                                        unsigned char* alive, int* corner_key, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_cluster_triples", "triangles", T);
    MVD_REQUIRE_COUNT("mesh_cluster_triples", "vertices", M);
    MVD_REQUIRE(K >= 0 && K <= M, "mesh_cluster_triples: %lld clusters of %lld vertices", K, M);
    MVD_REQUIRE(3 * T <= 0x7fffffffLL, "mesh_cluster_triples: %lld triangles, 3 T must be below 2^31", T);
    if (T == 0) return MVD_OK;
    MVD_REQUIRE(triangles && vertex_cluster && triples && alive && corner_key && M > 0, "mesh_cluster_triples: NULL argument");
    hipLaunchKernelGGL(cluster_triples_kernel, dim3(ms_blocks(T)), dim3(MS_THREADS), 0, (hipStream_t)stream, triangles, (int)T, (int)M,
                       vertex_cluster, (int)K, triples, alive, corner_key);
    return launch_status("mesh_cluster_triples");
}

extern "C" size_t mvd_mesh_cluster_quadrics_workspace_bytes(long long K) {
    if (K <= 0) return 0;
    return mvd::align_up((size_t)(K + 1) * sizeof(int), 256);
}

extern "C" int mvd_mesh_cluster_quadrics_f64(const float* vertices, long long M, const int* triangles, long long T, const int* sorted_cluster,
                                             const long long* perm, const long long* cluster_key, long long K, double origin_x,
                                             double origin_y, double origin_z, double cell, double* quadrics, void* workspace,
                                             size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_cluster_quadrics", "triangles", T);
    MVD_REQUIRE_COUNT("mesh_cluster_quadrics", "vertices", M);
    MVD_REQUIRE(K >= 0 && K <= M, "mesh_cluster_quadrics: %lld clusters of %lld vertices", K, M);
    MVD_REQUIRE(3 * T <= 0x7fffffffLL, "mesh_cluster_quadrics: %lld triangles, 3 T must be below 2^31", T);
    MVD_REQUIRE(isfinite(origin_x) && isfinite(origin_y) && isfinite(origin_z), "mesh_cluster_quadrics: the origin is not finite");
    MVD_REQUIRE(isfinite(cell) && cell > 0.0, "mesh_cluster_quadrics: cell must be finite and > 0, got %g", cell);
    if (K == 0) return MVD_OK;
    MVD_REQUIRE(vertices && cluster_key && quadrics, "mesh_cluster_quadrics: NULL argument");
    MVD_REQUIRE(T == 0 || (triangles && sorted_cluster && perm), "mesh_cluster_quadrics: NULL argument");
    MVD_REQUIRE(((uintptr_t)quadrics & 7) == 0, "mesh_cluster_quadrics: quadrics must be 8-byte aligned");
    MVD_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0 && workspace_bytes >= mvd_mesh_cluster_quadrics_workspace_bytes(K),
                "mesh_cluster_quadrics: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    int* seg = static_cast<int*>(workspace);
    hipLaunchKernelGGL(corner_segments_kernel, dim3(ms_blocks(K + 1)), dim3(MS_THREADS), 0, st, sorted_cluster, (int)(3 * T), (int)K, seg);
    hipLaunchKernelGGL(cluster_quadrics_kernel<false>, dim3(ms_blocks(K)), dim3(FS_THREADS), 0, st, vertices, (int)M, triangles, (int)T,
                       sorted_cluster, perm, seg, cluster_key, (int)K, origin_x, origin_y, origin_z, cell, quadrics);
    hipLaunchKernelGGL(cluster_quadrics_kernel<true>, dim3(ms_wave_blocks(K)), dim3(FS_THREADS), 0, st, vertices, (int)M, triangles, (int)T,
                       sorted_cluster, perm, seg, cluster_key, (int)K, origin_x, origin_y, origin_z, cell, quadrics);
    return launch_status("mesh_cluster_quadrics");
}

extern "C" int mvd_mesh_cluster_place_f32(const double* quadrics, const double* means, const int* cluster_start,
                                          const long long* cluster_key, const long long* perm, const float* vertices, long long K,
                                          long long M, double origin_x, double origin_y, double origin_z, double cell,
                                          double regularisation, float* out_vertices, unsigned char* placed, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_cluster_place", "vertices", M);
    MVD_REQUIRE(K >= 0 && K <= M, "mesh_cluster_place: %lld clusters of %lld vertices", K, M);
    MVD_REQUIRE(isfinite(origin_x) && isfinite(origin_y) && isfinite(origin_z), "mesh_cluster_place: the origin is not finite");
    MVD_REQUIRE(isfinite(cell) && cell > 0.0, "mesh_cluster_place: cell must be finite and > 0, got %g", cell);
    MVD_REQUIRE(!quadrics || (isfinite(regularisation) && regularisation > 0.0),
                "mesh_cluster_place: regularisation must be finite and > 0, got %g", regularisation);
    if (K == 0) return MVD_OK;
    MVD_REQUIRE(means && cluster_start && cluster_key && perm && vertices && out_vertices && placed, "mesh_cluster_place: NULL argument");
    MVD_REQUIRE((((uintptr_t)means | (uintptr_t)quadrics) & 7) == 0, "mesh_cluster_place: means and quadrics must be 8-byte aligned");
    hipLaunchKernelGGL(cluster_place_kernel, dim3(ms_blocks(K)), dim3(MS_THREADS), 0, (hipStream_t)stream, quadrics, means, cluster_start,
                       cluster_key, perm, vertices, (int)K, (int)M, origin_x, origin_y, origin_z, cell, regularisation, out_vertices, placed);
    return launch_status("mesh_cluster_place");
}

extern "C" int mvd_mesh_cluster_mark_first(const int* triples, const unsigned char* alive, const long long* perm, long long T,
                                           unsigned char* keep, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_cluster_mark_first", "triangles", T);
    if (T == 0) return MVD_OK;
    MVD_REQUIRE(triples && alive && perm && keep, "mesh_cluster_mark_first: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    // a perm that is no permutation leaves the triangles it does not name dropped
    if (hipMemsetAsync(keep, 0, (size_t)T, st) != hipSuccess) return launch_status("mesh_cluster_mark_first");
    hipLaunchKernelGGL(cluster_mark_first_kernel, dim3(ms_blocks(T)), dim3(MS_THREADS), 0, st, triples, alive, perm, (int)T, keep);
    return launch_status("mesh_cluster_mark_first");
}
