// Point-cloud evaluation: the truncated nearest neighbour between two clouds on a sorted uniform grid, the scores of its distances and
// the voxel thinning of a cloud.  The reference has NO counterpart (it ends at the per-view depth map), so there is no file:line to
// cite: the definition is the comment of these entries in include/mvd.h, restated in float64 numpy by robustmvd_amd/cloud_eval.py.
//   mvd_cloud_cell_keys_f32    point -> the 63-bit key of its grid cell / voxel (ix << 42 | iy << 21 | iz), invalid points last
//   mvd_cloud_grid_build_f32   the points gathered into key order as 16-byte records (x, y, z, original index)
//   mvd_cloud_nearest_f32      per query the nearest target within max_dist: a wave stages the cells around its queries through LDS
//   mvd_cloud_scores_f32       float64 sum of the distances, the count of valid points and the counts under T thresholds
//   mvd_voxel_reduce_f32       one point per occupied voxel: the float64 mean of its points and colours, and their number (the
//                              voxels are numbered by the compaction of compact.h)
// No atomics anywhere and fixed summation orders: two calls give the same bits.  The sort between the keys and their consumers is the
// caller's (a stable sort of the keys and the permutation it returns).
#include <math.h>
#include <stdint.h>

#include "cloud_grid.h"  // CE_*, cell_index, cell_key, lower_bound: shared with mesh_eval.hip
#include "compact.h"
#include "fixed_sums.h"

namespace mvd {

// ---- keys and records --------------------------------------------------------------------------------------------------------------
// The indices are clamped into the key's range: the callers that need exact membership (the target grid, the voxels) have checked
// the extent on the host, and for a query cloud the keys only decide the order in which the queries are visited.
__global__ void __launch_bounds__(256) cell_keys_kernel(const float* __restrict__ pts, int n, double ox, double oy, double oz, double inv,
                                                        long long* __restrict__ keys) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = pts[3 * (long long)i], y = pts[3 * (long long)i + 1], z = pts[3 * (long long)i + 2];
    long long key = CE_INVALID_KEY;
    if (finite3(x, y, z)) {
        const double hi = (double)(CE_LIMIT - 1);
        key = cell_key(cell_index(x, ox, inv, 0.0, hi), cell_index(y, oy, inv, 0.0, hi), cell_index(z, oz, inv, 0.0, hi));
    }
    keys[i] = key;
}

__global__ void __launch_bounds__(256) grid_build_kernel(const float* __restrict__ pts, const long long* __restrict__ perm, int n,
                                                         float4* __restrict__ rec) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long p = perm[i];
    float4 r = make_float4(NAN, NAN, NAN, __int_as_float(0));  // a permutation entry out of range: a record that matches nothing
    if ((unsigned long long)p < (unsigned long long)n) r = make_float4(pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], __int_as_float((int)p));
    rec[i] = r;
}

// ---- nearest neighbour -------------------------------------------------------------------------------------------------------------
// One wave (= one workgroup) per 64 consecutive query records.  The queries come sorted by the same cell keys as the targets, so a
// wave's queries sit in a few neighbouring cells.  The wave works through them group by group: the first query not yet served leads,
// and its group is every unserved query of the same (x, y) column whose z index is within 3 above the leader's.  With z in the
// key's low bits the cells (x', y', z_lead - 1 .. z_lead + 4) of one of the nine neighbouring columns are ONE run of the sorted keys,
// found by two binary searches; lanes 0..8 search the nine runs at once.  The runs are treated as one list of records, staged
// through LDS 256 at a time (four 16-byte loads in flight per lane), and EVERY lane scans every staged record with broadcast
// ds_read_b128s: a record outside a lane's own 27 cells is still a target, so scanning it cannot make the minimum wrong, and no lane
// diverges.  Nothing is sized by a cell's population: a cell of a million points is 3,900 stages.
//
// Why the 27 cells are enough.  Let q, p have a computed distance < max_dist.  The computed distance is within a few float32
// roundings of the true one, so per axis |q - p| < max_dist (1 + 2^-21).  The entry requires a cell edge c >= max_dist (1 + 2^-10)
// (inv = 1 / c), so |q - p| * inv < (1 + 2^-21) / (1 + 2^-10) < 1 - 2^-11.  The index is the floor of t(v) = fl((v - o) * inv), two
// double roundings: |t(v) - (v - o) * inv| <= 2^-52 |t(v)| < 2^-30 for |t| < 2^22.  So |t(q) - t(p)| < 1 - 2^-11 + 2^-29 < 1 and the
// floors differ by at most one on every axis.  A target's indices are inside [0, CE_LIMIT) (the caller's check); a query's are
// clamped to [-2, CE_LIMIT + 2], which moves only queries at least two cells outside the targets' range, and those have no target
// within max_dist.
//
// The best candidate is the minimum of (bits of d^2) << 32 | original index as an unsigned 64-bit number: d^2 >= +0, so its bits
// order like its value, equal d^2 are decided by the smaller index, and a NaN (an invalid target) is above the starting value.
constexpr int NN_STAGE = 256;

__global__ void __launch_bounds__(64) cloud_nearest_kernel(const float4* __restrict__ qrec, int n, const float4* __restrict__ trec,
                                                           const long long* __restrict__ tkeys, int m, double ox, double oy, double oz,
                                                           double inv, float max_dist, float* __restrict__ dist,
                                                           int* __restrict__ index) {
    __shared__ float4 s_rec[NN_STAGE];
    __shared__ int s_lo[9];
    __shared__ int s_pre[10];  // s_pre[r] = the records of the runs before r
    const int lane = threadIdx.x;
    const long long i = (long long)blockIdx.x * 64 + lane;
    const bool have = i < n;
    const float4 me = have ? qrec[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool valid = have && finite3(me.x, me.y, me.z);
    const double chi = (double)(CE_LIMIT + 2);
    const int cx = valid ? cell_index(me.x, ox, inv, -2.0, chi) : 0;
    const int cy = valid ? cell_index(me.y, oy, inv, -2.0, chi) : 0;
    const int cz = valid ? cell_index(me.z, oz, inv, -2.0, chi) : 0;

    unsigned long long best = (0x7f800000ull << 32) | 0xffffffffull;  // d^2 = +inf, no index
    unsigned long long todo = __ballot(valid);
    while (todo != 0ull) {  // wave-uniform: the barriers below are reached by all 64 lanes
        const int lead = __ffsll((long long)todo) - 1;
        const int gx = __shfl(cx, lead), gy = __shfl(cy, lead), gz = __shfl(cz, lead);
        const bool in_group = ((todo >> lane) & 1ull) && cx == gx && cy == gy && (unsigned)(cz - gz) < 4u;
        todo &= ~__ballot(in_group);  // the leader is in its own group: the loop ends
        const int zlo = max(gz - 1, 0), zhi = min(gz + 4, CE_LIMIT - 1);
        int lo = 0, cnt = 0;
        if (lane < 9) {
            const int x = gx + lane / 3 - 1, y = gy + lane % 3 - 1;
            if (x >= 0 && x < CE_LIMIT && y >= 0 && y < CE_LIMIT && zlo <= zhi) {
                lo = lower_bound(tkeys, m, cell_key(x, y, zlo));
                cnt = max(lower_bound(tkeys, m, cell_key(x, y, zhi) + 1) - lo, 0);  // 0: keys that do not ascend stay in bounds
            }
        }
        // inclusive prefix of the nine counts over lanes 0..8
        int pre = cnt;
#pragma unroll
        for (int s = 1; s < 16; s <<= 1) {
            const int up = __shfl_up(pre, s);
            if (lane >= s) pre += up;
        }
        if (lane < 9) {
            s_lo[lane] = lo;
            s_pre[lane + 1] = pre;
        }
        if (lane == 0) s_pre[0] = 0;
        __syncthreads();
        const int total = s_pre[9];
        for (int base = 0; base < total; base += NN_STAGE) {
            const int c = min(NN_STAGE, total - base);
#pragma unroll
            for (int k = 0; k < NN_STAGE / 64; ++k) {
                const int slot = lane + 64 * k, f = base + slot;
                if (slot < c) {
                    int r = 0;
#pragma unroll
                    for (int r2 = 1; r2 < 9; ++r2)
                        if (f >= s_pre[r2]) r = r2;
                    s_rec[slot] = trec[s_lo[r] + (f - s_pre[r])];  // inside [lo_r, hi_r), a sub-range of [0, m)
                }
            }
            __syncthreads();
#pragma unroll 4
            for (int j = 0; j < c; ++j) {
                const float4 p = s_rec[j];
                const float dx = me.x - p.x, dy = me.y - p.y, dz = me.z - p.z;
                const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
                const unsigned long long cand = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(p.w);
                best = cand < best ? cand : best;
            }
            __syncthreads();  // the stage is read before the next one, or the next group's tables, overwrite it
        }
        __syncthreads();  // total == 0: the tables are still read before the next group writes them
    }
    if (!have) return;
    const float d = sqrtf(__uint_as_float((unsigned)(best >> 32)));
    const bool found = valid && d < max_dist;  // false for the starting value and for a NaN
    const int orig = __float_as_int(me.w);
    if ((unsigned)orig < (unsigned)n) {
        dist[orig] = found ? d : max_dist;
        index[orig] = found ? (int)(unsigned)(best & 0xffffffffull) : -1;
    }
}

// ---- scores ------------------------------------------------------------------------------------------------------------------------
// A two-level sum of fixed_sums.h: a workgroup takes 2048 consecutive distances, thread i the distances i, i + 256, ..., and stores
// one record (the float64 sum, the valid points, the T counts); fixed_final_kernel adds the workgroups' records.
constexpr int SC_PER_THREAD = 8;
constexpr int SC_PER_WG = FS_THREADS * SC_PER_THREAD;
constexpr int SC_VALID = 1, SC_UNDER = 2;  // the words after the sum: the valid points, then those under threshold t
using ScoreRecord = FixedRecord<2 + MVD_CLOUD_MAX_THRESHOLDS, 1ull>;  // a double and nine int64, 80 bytes

__global__ void __launch_bounds__(FS_THREADS) scores_partial_kernel(const float* __restrict__ dist, const int* __restrict__ index,
                                                                    const float* __restrict__ pts, int n,
                                                                    const float* __restrict__ thresholds, int T,
                                                                    unsigned char* __restrict__ partials) {
    float tau[MVD_CLOUD_MAX_THRESHOLDS];
#pragma unroll
    for (int t = 0; t < MVD_CLOUD_MAX_THRESHOLDS; ++t) tau[t] = t < T ? thresholds[t] : -1.f;  // no distance is under -1
    ScoreRecord a{};
    const long long base = (long long)blockIdx.x * SC_PER_WG + threadIdx.x;
#pragma unroll
    for (int k = 0; k < SC_PER_THREAD; ++k) {
        const long long i = base + (long long)k * FS_THREADS;
        if (i >= n) break;
        // a query with a neighbour is a valid point; the others are looked up where the points are given
        bool ok = true;
        if (pts && index[i] < 0) ok = finite3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
        if (!ok) continue;
        const float d = dist[i];
        a.addf(0, (double)d);
        a.addi(SC_VALID, 1);
#pragma unroll
        for (int t = 0; t < MVD_CLOUD_MAX_THRESHOLDS; ++t) a.addi(SC_UNDER + t, d < tau[t] ? 1 : 0);
    }
    fixed_reduce_store(a, partials + (size_t)blockIdx.x * ScoreRecord::block_bytes);
}

// ---- voxel reduce ------------------------------------------------------------------------------------------------------------------
// Position i of the sorted keys is the head of a voxel's segment when its key is a valid point's and differs from the key before it.
// The heads are compacted by compact.h, as the masked pixels of depth_fusion.hip are (ballot counts per 256-key chunk, one
// workgroup's exclusive scan, rank in the ballot), which numbers the voxels in key order and leaves each voxel's first position in
// seg[voxel]; seg[number of voxels] is the number of valid points.  Then the segment walk of fixed_sums.h adds every voxel's points in
// sorted (= original, the sort is stable) order in float64: a lane per voxel, the whole wave for a voxel of more than 64 points, so a
// voxel that holds the whole cloud costs n / 64 steps.

struct VoxelHead {
    const long long* keys;
    __device__ bool operator()(long long p) const {
        const long long k = keys[p];
        return k != CE_INVALID_KEY && (p == 0 || keys[p - 1] != k);
    }
};

__global__ void __launch_bounds__(CP_THREADS) voxel_heads_kernel(const long long* __restrict__ keys, int n,
                                                                 const unsigned* __restrict__ offsets,
                                                                 const long long* __restrict__ total, int* __restrict__ seg) {
    compact_walk(VoxelHead{keys}, offsets, n, [&](long long p, long long slot) { seg[slot] = (int)p; });
    // the last valid point closes the last segment: not a part of the compaction, and no launch of its own
    const long long base = compact_wave_chunk() * CP_CHUNK + (threadIdx.x & 63);
#pragma unroll
    for (int k = 0; k < CP_SUB; ++k) {
        const long long p = base + 64 * k;
        if (p < n && keys[p] != CE_INVALID_KEY && (p + 1 == n || keys[p + 1] == CE_INVALID_KEY)) seg[total[0]] = (int)(p + 1);
    }
}

template <bool COLOR>
__global__ void __launch_bounds__(FS_THREADS) voxel_mean_kernel(const int* __restrict__ seg, const long long* __restrict__ total,
                                                                const long long* __restrict__ perm, const float* __restrict__ pts,
                                                                const float* __restrict__ col, int n, float* __restrict__ xyz,
                                                                float* __restrict__ rgb, int* __restrict__ counts) {
    constexpr int N = COLOR ? 6 : 3;
    const auto add = [&](FixedSums<N>& s, long long pos) {
        const long long p = perm[pos];
        if ((unsigned long long)p >= (unsigned long long)n) return;  // not a permutation of 0..n-1: skipped, never dereferenced
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s.v[k] += (double)pts[3 * p + k];
            if constexpr (COLOR) s.v[3 + k] += (double)col[3 * p + k];
        }
    };
    const auto span = [&](FixedSums<N>& s, long long b, long long e, int lane) { fixed_lane_span(s, b, e, lane, add); };
    const auto store = [&](const FixedSums<N>& s, int len, long long vox) {
        const double nd = (double)len;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            xyz[3 * vox + k] = (float)(s.v[k] / nd);
            if constexpr (COLOR) rgb[3 * vox + k] = (float)(s.v[3 + k] / nd);
        }
        counts[vox] = len;
    };
    // seg ends at the number of valid points <= n
    fixed_segment_walk<N>(seg, min(total[0], (long long)n), n, add, span, store);
}

}  // namespace mvd

extern "C" int mvd_cloud_cell_keys_f32(const float* points, long long n, double origin_x, double origin_y, double origin_z, double inv,
                                       long long* keys, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_cell_keys", "points", n);
    if (n == 0) return MVD_OK;
    MVD_REQUIRE(points && keys, "cloud_cell_keys: NULL argument");
    MVD_REQUIRE(isfinite(origin_x) && isfinite(origin_y) && isfinite(origin_z), "cloud_cell_keys: the origin is not finite");
    MVD_REQUIRE(isfinite(inv) && inv > 0.0, "cloud_cell_keys: inv must be finite and > 0, got %g", inv);
    hipLaunchKernelGGL(cell_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, (int)n, origin_x,
                       origin_y, origin_z, inv, keys);
    return launch_status("cloud_cell_keys");
}

extern "C" int mvd_cloud_grid_build_f32(const float* points, const long long* perm, long long n, float* records, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_grid_build", "points", n);
    if (n == 0) return MVD_OK;
    MVD_REQUIRE(points && perm && records, "cloud_grid_build: NULL argument");
    MVD_REQUIRE(((uintptr_t)records & 15) == 0, "cloud_grid_build: records must be 16-byte aligned");
    hipLaunchKernelGGL(grid_build_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, perm, (int)n,
                       reinterpret_cast<float4*>(records));
    return launch_status("cloud_grid_build");
}

extern "C" int mvd_cloud_nearest_f32(const float* query_records, long long n, const float* target_records, const long long* target_keys,
                                     long long m, double origin_x, double origin_y, double origin_z, double inv, float max_dist,
                                     float* dist, int* index, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_nearest", "points", n);
    MVD_REQUIRE_COUNT("cloud_nearest", "points", m);
    MVD_REQUIRE(max_dist > 0.f && finite_f32(max_dist), "cloud_nearest: max_dist must be finite and > 0, got %g", (double)max_dist);
    MVD_REQUIRE(isfinite(origin_x) && isfinite(origin_y) && isfinite(origin_z), "cloud_nearest: the origin is not finite");
    MVD_REQUIRE(isfinite(inv) && inv > 0.0, "cloud_nearest: inv must be finite and > 0, got %g", inv);
    MVD_REQUIRE(inv * ((double)max_dist * (1.0 + 1.0 / 1024.0)) <= 1.0 + 1e-12,
                "cloud_nearest: the cell edge %g is below max_dist (1 + 2^-10) = %g", 1.0 / inv, (double)max_dist * (1.0 + 1.0 / 1024.0));
    if (n == 0) return MVD_OK;
    MVD_REQUIRE(query_records && dist && index, "cloud_nearest: NULL argument");
    MVD_REQUIRE(m == 0 || (target_records && target_keys), "cloud_nearest: NULL target");
    MVD_REQUIRE((((uintptr_t)query_records | (uintptr_t)target_records) & 15) == 0, "cloud_nearest: records must be 16-byte aligned");
    hipLaunchKernelGGL(cloud_nearest_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(query_records), (int)n, reinterpret_cast<const float4*>(target_records), target_keys,
                       (int)m, origin_x, origin_y, origin_z, inv, max_dist, dist, index);
    return launch_status("cloud_nearest");
}

extern "C" size_t mvd_cloud_scores_workspace_bytes(long long n) {
    if (n <= 0) return 0;
    return mvd::align_up(mvd::fixed_partials_bytes<mvd::ScoreRecord>(n, mvd::SC_PER_WG), 256);
}

extern "C" int mvd_cloud_scores_f32(const float* dist, const int* index, const float* points, long long n, const float* thresholds, int T,
                                    void* result, void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_scores", "points", n);
    MVD_REQUIRE(T >= 1 && T <= MVD_CLOUD_MAX_THRESHOLDS, "cloud_scores: %d thresholds, supported 1..%d", T, MVD_CLOUD_MAX_THRESHOLDS);
    MVD_REQUIRE(thresholds && result, "cloud_scores: NULL argument");
    MVD_REQUIRE(((uintptr_t)result & 7) == 0, "cloud_scores: result must be 8-byte aligned");
    MVD_REQUIRE(n == 0 || (dist && index), "cloud_scores: NULL argument");
    MVD_REQUIRE(n == 0 || (workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= mvd_cloud_scores_workspace_bytes(n)),
                "cloud_scores: workspace too small or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nwg = (int)fixed_workgroups(n, SC_PER_WG);
    unsigned char* partials = static_cast<unsigned char*>(workspace);
    if (nwg > 0)
        hipLaunchKernelGGL(scores_partial_kernel, dim3((unsigned)nwg), dim3(FS_THREADS), 0, st, dist, index, points, (int)n, thresholds, T,
                           partials);
    fixed_final_launch<ScoreRecord>(partials, nwg, result, st);
    return launch_status("cloud_scores");
}

extern "C" size_t mvd_voxel_reduce_workspace_bytes(long long n) {
    if (n <= 0) return 0;
    return mvd::compact_offsets_bytes(n) + mvd::align_up((size_t)(n + 1) * sizeof(int), 256);
}

extern "C" int mvd_voxel_reduce_f32(const long long* keys, const long long* perm, const float* points, const float* colors, long long n,
                                    float* xyz, float* rgb, int* counts, long long* num_voxels, void* workspace, size_t workspace_bytes,
                                    mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("voxel_reduce", "points", n);
    MVD_REQUIRE(num_voxels && ((uintptr_t)num_voxels & 7) == 0, "voxel_reduce: num_voxels must be given and 8-byte aligned");
    MVD_REQUIRE(!colors == !rgb, "voxel_reduce: colors and rgb go together");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(num_voxels, 0, sizeof(long long), st) != hipSuccess) return launch_status("voxel_reduce");
        return MVD_OK;
    }
    MVD_REQUIRE(keys && perm && points && xyz && counts, "voxel_reduce: NULL argument");
    MVD_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0 && workspace_bytes >= mvd_voxel_reduce_workspace_bytes(n),
                "voxel_reduce: workspace too small or misaligned");
    const unsigned nwg = compact_workgroups(n);
    unsigned* chunk_counts = static_cast<unsigned*>(workspace);
    int* seg = reinterpret_cast<int*>(static_cast<unsigned char*>(workspace) + compact_offsets_bytes(n));
    hipLaunchKernelGGL(compact_count_kernel<VoxelHead>, dim3(nwg), dim3(CP_THREADS), 0, st, VoxelHead{keys}, n, chunk_counts);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(CP_THREADS), 0, st, chunk_counts, compact_chunks(n), num_voxels);
    hipLaunchKernelGGL(voxel_heads_kernel, dim3(nwg), dim3(CP_THREADS), 0, st, keys, (int)n, chunk_counts, num_voxels, seg);
    // one lane per voxel, at most n voxels: the waves past the count leave at once
    const unsigned mwg = (unsigned)((n + FS_THREADS - 1) / FS_THREADS);
    if (colors)
        hipLaunchKernelGGL(voxel_mean_kernel<true>, dim3(mwg), dim3(FS_THREADS), 0, st, seg, num_voxels, perm, points, colors, (int)n, xyz,
                           rgb, counts);
    else
        hipLaunchKernelGGL(voxel_mean_kernel<false>, dim3(mwg), dim3(FS_THREADS), 0, st, seg, num_voxels, perm, points, colors, (int)n, xyz,
                           rgb, counts);
    return launch_status("voxel_reduce");
}
