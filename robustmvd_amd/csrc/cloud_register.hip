// Point-cloud registration (ICP): the per-iteration device work around mvd_cloud_nearest_f32.  The reference has NO counterpart, so
// there is no file:line to cite: the definition is robustmvd_amd/cloud_register.py (transform_numpy, pair_sums_numpy) and the comment
// of these entries in include/mvd.h.
//   mvd_cloud_transform_f32          points (and normals) through T: x -> M x + t
//   mvd_cloud_transform_records_f32  mvd_cloud_grid_build_f32 fused with the move: sorted position i = T(points[perm[i]]), perm[i]
//   mvd_cloud_pair_sums_f32          per source point: q = T(S_i) again (the same operations, the same bits as the records), the
//                                    gather of P[index[i]] (and its normal), and the float64 sums the closed-form solvers need
// Every per-point value is a fixed sequence of IEEE double operations (no contraction: the pragma below, and the library's
// -ffp-contract=off), so numpy forms the same bits; the sums are added in an order fixed by n alone.  No atomics: two calls give
// the same bits.
#include <math.h>
#include <stdint.h>

#include "fixed_sums.h"

#pragma STDC FP_CONTRACT OFF

namespace mvd {

struct RgTransform {
    double m[12];  // the rows of [M | t]
};

// q_a = float32(((M[a,0] x + M[a,1] y) + M[a,2] z) + t[a]) in float64, rounded once.  A row with a non-finite coordinate, before or
// after, is (NaN, NaN, NaN) with the bits 0x7fc00000: an invalid point stays one, and no NaN's sign or payload is left to the hardware.
__device__ __forceinline__ bool rg_move(const RgTransform& T, float x, float y, float z, float& qx, float& qy, float& qz) {
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    qx = (float)(((T.m[0] * dx + T.m[1] * dy) + T.m[2] * dz) + T.m[3]);
    qy = (float)(((T.m[4] * dx + T.m[5] * dy) + T.m[6] * dz) + T.m[7]);
    qz = (float)(((T.m[8] * dx + T.m[9] * dy) + T.m[10] * dz) + T.m[11]);
    const bool ok = finite3(x, y, z) && finite3(qx, qy, qz);
    if (!ok) qx = qy = qz = __uint_as_float(0x7fc00000u);
    return ok;
}

__global__ void __launch_bounds__(256) transform_kernel(const float* __restrict__ pts, const float* __restrict__ nrm, int n, RgTransform T,
                                                        float* __restrict__ out_pts, float* __restrict__ out_nrm) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float qx, qy, qz;
    rg_move(T, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], qx, qy, qz);
    out_pts[3 * i] = qx;
    out_pts[3 * i + 1] = qy;
    out_pts[3 * i + 2] = qz;
    if (!nrm) return;
    // a normal goes through M alone and is normalised in float64; an invalid or vanishing one is (0, 0, 0)
    const float nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2];
    const double vx = (double)nx, vy = (double)ny, vz = (double)nz;
    const double wx = (T.m[0] * vx + T.m[1] * vy) + T.m[2] * vz;
    const double wy = (T.m[4] * vx + T.m[5] * vy) + T.m[6] * vz;
    const double wz = (T.m[8] * vx + T.m[9] * vy) + T.m[10] * vz;
    const double len = sqrt((wx * wx + wy * wy) + wz * wz);
    const bool ok = finite3(nx, ny, nz) && len > 0.0 && isfinite(len);
    out_nrm[3 * i] = ok ? (float)(wx / len) : 0.f;
    out_nrm[3 * i + 1] = ok ? (float)(wy / len) : 0.f;
    out_nrm[3 * i + 2] = ok ? (float)(wz / len) : 0.f;
}

__global__ void __launch_bounds__(256) transform_records_kernel(const float* __restrict__ pts, const long long* __restrict__ perm, int n,
                                                                RgTransform T, float4* __restrict__ rec) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long p = perm[i];
    float4 r = make_float4(NAN, NAN, NAN, __int_as_float(0));  // a permutation entry out of range: a record that matches nothing
    if ((unsigned long long)p < (unsigned long long)n) {
        rg_move(T, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], r.x, r.y, r.z);
        r.w = __int_as_float((int)p);
    }
    rec[i] = r;
}

// ---- pair sums ---------------------------------------------------------------------------------------------------------------------
// A two-level sum of fixed_sums.h.  A workgroup takes 2048 consecutive source points, a lane eight of them in two batches of four:
// the four indices and source points are loaded first, then the four gathers of P[j] (and the normal) are issued together, and only
// then are the terms formed, so that a lane has four dependent gathers in flight instead of one.  A workgroup's record is a count and
// 18 or 28 doubles in a 256-byte block; fixed_final_kernel adds the workgroups' records.
constexpr int RG_BATCH = 4;
constexpr int RG_PER_THREAD = 8;
constexpr int RG_PER_WG = FS_THREADS * RG_PER_THREAD;
constexpr int RG_WORDS = 32;  // the result block: an int64 count, the doubles, zeros
constexpr int RG_POINT = 18, RG_PLANE = 28;
static_assert(RG_PER_WG == MVD_CLOUD_PAIR_SUMS_PER_WORKGROUP, "include/mvd.h states the points per workgroup");
static_assert(RG_PER_THREAD % RG_BATCH == 0, "pair sums geometry");

template <bool PLANE>
using PairRecord = FixedRecord<1 + (PLANE ? RG_PLANE : RG_POINT), ((1ull << (PLANE ? RG_PLANE : RG_POINT)) - 1ull) << 1, RG_WORDS>;

// The terms of one pair; the operation order is the docstring's of cloud_register.pair_sums_numpy.
template <bool PLANE>
__device__ __forceinline__ void rg_add(PairRecord<PLANE>& acc, float qx, float qy, float qz, float px, float py, float pz, float nx,
                                       float ny, float nz, double cx, double cy, double cz) {
    const double a[3] = {(double)qx - cx, (double)qy - cy, (double)qz - cz};
    const double b[3] = {(double)px - cx, (double)py - cy, (double)pz - cz};
    const double d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
    acc.addi(0, 1);
    const auto add = [&](int k, double term) { acc.addf(1 + k, term); };  // sum k of the definition
    if constexpr (!PLANE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            add(k, a[k]);
            add(3 + k, b[k]);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) add(6 + 3 * r + c, a[r] * b[c]);
        add(15, (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
        add(16, (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
        add(17, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    } else {
        const double u[3] = {(double)nx, (double)ny, (double)nz};
        const double r = (d[0] * u[0] + d[1] * u[1]) + d[2] * u[2];
        const double J[6] = {a[1] * u[2] - a[2] * u[1], a[2] * u[0] - a[0] * u[2], a[0] * u[1] - a[1] * u[0], u[0], u[1], u[2]};
        int slot = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) add(slot++, J[i] * J[j]);
#pragma unroll
        for (int k = 0; k < 6; ++k) add(21 + k, J[k] * r);
        add(27, r * r);
    }
}

template <bool PLANE>
__global__ void __launch_bounds__(FS_THREADS) pair_sums_partial_kernel(const float* __restrict__ src, int n, RgTransform T,
                                                                       const int* __restrict__ index, const float* __restrict__ tgt,
                                                                       const float* __restrict__ tnrm, int m, double cx, double cy,
                                                                       double cz, unsigned char* __restrict__ partials) {
    PairRecord<PLANE> acc{};
    const long long base = (long long)blockIdx.x * RG_PER_WG + threadIdx.x;
    for (int b0 = 0; b0 < RG_PER_THREAD; b0 += RG_BATCH) {
        int j[RG_BATCH];
        float s[RG_BATCH][3], p[RG_BATCH][3], u[RG_BATCH][3];
#pragma unroll
        for (int k = 0; k < RG_BATCH; ++k) {
            const long long i = base + (long long)(b0 + k) * FS_THREADS;
            j[k] = -1;
            s[k][0] = s[k][1] = s[k][2] = 0.f;
            if (i < n) {
                j[k] = index[i];
                s[k][0] = src[3 * i];
                s[k][1] = src[3 * i + 1];
                s[k][2] = src[3 * i + 2];
            }
        }
#pragma unroll
        for (int k = 0; k < RG_BATCH; ++k) {
            const bool has = (unsigned)j[k] < (unsigned)m;  // -1, and an index that is no target's, pair with nothing
            const long long t = has ? j[k] : 0;
            p[k][0] = p[k][1] = p[k][2] = u[k][0] = u[k][1] = u[k][2] = 0.f;
            if (has) {
                p[k][0] = tgt[3 * t];
                p[k][1] = tgt[3 * t + 1];
                p[k][2] = tgt[3 * t + 2];
                if (PLANE) {
                    u[k][0] = tnrm[3 * t];
                    u[k][1] = tnrm[3 * t + 1];
                    u[k][2] = tnrm[3 * t + 2];
                }
            }
            if (!has) j[k] = -1;
        }
#pragma unroll
        for (int k = 0; k < RG_BATCH; ++k) {
            float qx, qy, qz;
            bool pair = rg_move(T, s[k][0], s[k][1], s[k][2], qx, qy, qz) && j[k] >= 0 && finite3(p[k][0], p[k][1], p[k][2]);
            if (PLANE) pair = pair && finite3(u[k][0], u[k][1], u[k][2]) && !(u[k][0] == 0.f && u[k][1] == 0.f && u[k][2] == 0.f);
            if (pair) rg_add<PLANE>(acc, qx, qy, qz, p[k][0], p[k][1], p[k][2], u[k][0], u[k][1], u[k][2], cx, cy, cz);
        }
    }
    fixed_reduce_store(acc, partials + (size_t)blockIdx.x * PairRecord<PLANE>::block_bytes);
}

static inline bool rg_load(const double* transform, RgTransform& T) {
    for (int k = 0; k < 12; ++k) {
        T.m[k] = transform[k];
        if (!isfinite(T.m[k])) return false;
    }
    return true;
}

}  // namespace mvd

extern "C" int mvd_cloud_transform_f32(const float* points, const float* normals, long long n, const double* transform, float* out_points,
                                       float* out_normals, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_transform", "points", n);
    RgTransform T;
    MVD_REQUIRE(transform && rg_load(transform, T), "cloud_transform: the transform must be 12 finite doubles");
    MVD_REQUIRE(!normals == !out_normals, "cloud_transform: normals and out_normals go together");
    if (n == 0) return MVD_OK;
    MVD_REQUIRE(points && out_points, "cloud_transform: NULL argument");
    hipLaunchKernelGGL(transform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, normals, (int)n, T,
                       out_points, out_normals);
    return launch_status("cloud_transform");
}

extern "C" int mvd_cloud_transform_records_f32(const float* points, const long long* perm, long long n, const double* transform,
                                               float* records, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_transform_records", "points", n);
    RgTransform T;
    MVD_REQUIRE(transform && rg_load(transform, T), "cloud_transform_records: the transform must be 12 finite doubles");
    if (n == 0) return MVD_OK;
    MVD_REQUIRE(points && perm && records, "cloud_transform_records: NULL argument");
    MVD_REQUIRE(((uintptr_t)records & 15) == 0, "cloud_transform_records: records must be 16-byte aligned");
    hipLaunchKernelGGL(transform_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, perm, (int)n,
                       T, reinterpret_cast<float4*>(records));
    return launch_status("cloud_transform_records");
}

extern "C" size_t mvd_cloud_pair_sums_workspace_bytes(long long n) {
    if (n <= 0) return 0;
    return mvd::fixed_partials_bytes<mvd::PairRecord<true>>(n, mvd::RG_PER_WG);
}

extern "C" int mvd_cloud_pair_sums_f32(const float* source, long long n, const double* transform, const int* index, const float* target,
                                       const float* target_normals, long long m, double pivot_x, double pivot_y, double pivot_z,
                                       void* result, void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_pair_sums", "points", n);
    MVD_REQUIRE_COUNT("cloud_pair_sums", "points", m);
    RgTransform T;
    MVD_REQUIRE(transform && rg_load(transform, T), "cloud_pair_sums: the transform must be 12 finite doubles");
    MVD_REQUIRE(isfinite(pivot_x) && isfinite(pivot_y) && isfinite(pivot_z), "cloud_pair_sums: the pivot is not finite");
    MVD_REQUIRE(result && ((uintptr_t)result & 7) == 0, "cloud_pair_sums: result must be given and 8-byte aligned");
    MVD_REQUIRE(n == 0 || (source && index), "cloud_pair_sums: NULL argument");
    MVD_REQUIRE(m == 0 || target, "cloud_pair_sums: NULL target");
    MVD_REQUIRE(n == 0 || (workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= mvd_cloud_pair_sums_workspace_bytes(n)),
                "cloud_pair_sums: workspace too small or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nwg = (int)fixed_workgroups(n, RG_PER_WG);
    unsigned char* partials = static_cast<unsigned char*>(workspace);
    if (target_normals) {
        if (nwg > 0)
            hipLaunchKernelGGL(pair_sums_partial_kernel<true>, dim3((unsigned)nwg), dim3(FS_THREADS), 0, st, source, (int)n, T, index, target,
                               target_normals, (int)m, pivot_x, pivot_y, pivot_z, partials);
        fixed_final_launch<PairRecord<true>>(partials, nwg, result, st);
    } else {
        if (nwg > 0)
            hipLaunchKernelGGL(pair_sums_partial_kernel<false>, dim3((unsigned)nwg), dim3(FS_THREADS), 0, st, source, (int)n, T, index, target,
                               target_normals, (int)m, pivot_x, pivot_y, pivot_z, partials);
        fixed_final_launch<PairRecord<false>>(partials, nwg, result, st);
    }
    return launch_status("cloud_pair_sums");
}
