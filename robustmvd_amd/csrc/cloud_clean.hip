// Point-cloud clean-up: the neighbourhood queries on the sorted grid of cloud_grid.h, the PCA normals and the outlier verdicts.  The
// reference has NO counterpart (it ends at the per-view depth map), so there is no file:line to cite: the definition is the comment of
// these entries in include/mvd.h, restated in numpy by robustmvd_amd/cloud_clean.py.
//   mvd_cloud_radius_moments_f32   per query the count of the targets with d2 < r2, the float64 sum of their distances and the nine
//                                  float64 moments of their offsets from the query
//   mvd_cloud_knn_f32              per query the up-to-k targets with d2 < r2 that are smallest in (bits of d2, original index)
//   mvd_cloud_list_moments_f32     the same count, sum and moments over each query's k-NN list, a gather
//   mvd_cloud_normals_f64          the eigenvector of the smallest eigenvalue of each point's covariance (cyclic Jacobi in float64,
//                                  a lane per point), the surface variation and the orientation
//   mvd_cloud_keep_density / mvd_cloud_knn_mean_sums_f32 / mvd_cloud_keep_threshold   the verdicts of the two outlier rules
//   mvd_cloud_select               the kept indices and the remap of a keep mask through compact.h
// No atomics anywhere and fixed summation orders: two calls give the same bits.
#include <math.h>
#include <stdint.h>

#include "cloud_grid.h"
#include "compact.h"
#include "fixed_sums.h"

namespace mvd {

// ---- the walk over a wave's neighbourhoods -----------------------------------------------------------------------------------------
// The staging loop of cloud_nearest_kernel (cloud_eval.hip, where its shape is explained): one wave per 64 consecutive query records;
// the first query not yet served leads a group of the queries of its (x, y) column within 3 cells above it; lanes 0..8 find the nine
// runs of sorted keys that cover the cells (x', y', z_lead - 1 .. z_lead + 4); the runs are staged through LDS 256 records at a time
// and EVERY lane calls visit(record) for every staged record.  A query is in exactly one group and a group's runs are disjoint, so a
// lane meets every target of its 27 cells exactly once.  The nine runs are visited in ascending (x', y'), that is in ascending key
// order, and each run in sorted order: a lane meets its neighbours in ascending position of the target grid's sorted order, which is
// the order the sums of mvd_cloud_radius_moments_f32 are defined in.
//
// Why the 27 cells are enough for d2 < r2.  d2 = fl(fl(dx dx + dy dy) + dz dz) of the float32 differences is at least
// dx dx (1 - 2^-24)^3 for each axis (every rounding is monotone and the other terms are non-negative), and r2 = fl(r r) <= r^2 (1 + 2^-24).
// So d2 < r2 gives |dx| < r (1 + 2^-22), and dx = fl(q - p) is within 2^-24 relative of q - p: per axis |q - p| < r (1 + 2^-21).  With a
// cell edge c >= r (1 + 2^-10) the argument of cloud_eval.hip goes through unchanged: |q - p| * inv < 1 - 2^-11, the two double
// roundings of the index move it by less than 2^-29, and the floors differ by at most one on every axis.  Conversely a staged record
// outside a lane's 27 cells fails d2 < r2, so visiting it changes nothing.
constexpr int CC_STAGE = 256;

struct WaveQuery {
    float4 me;   // x, y, z and the original index's bits
    bool have;   // the lane has a record
    bool valid;  // and its point is finite
};

template <class Visit>
__device__ __forceinline__ WaveQuery neighbour_walk(const float4* __restrict__ qrec, int n, const float4* __restrict__ trec,
                                                    const long long* __restrict__ tkeys, int m, double ox, double oy, double oz,
                                                    double inv, const Visit& visit) {
    __shared__ float4 s_rec[CC_STAGE];
    __shared__ int s_lo[9];
    __shared__ int s_pre[10];  // s_pre[r] = the records of the runs before r
    const int lane = threadIdx.x;
    const long long i = (long long)blockIdx.x * 64 + lane;
    WaveQuery w;
    w.have = i < n;
    w.me = w.have ? qrec[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    w.valid = w.have && finite3(w.me.x, w.me.y, w.me.z);
    const double chi = (double)(CE_LIMIT + 2);
    const int cx = w.valid ? cell_index(w.me.x, ox, inv, -2.0, chi) : 0;
    const int cy = w.valid ? cell_index(w.me.y, oy, inv, -2.0, chi) : 0;
    const int cz = w.valid ? cell_index(w.me.z, oz, inv, -2.0, chi) : 0;

    unsigned long long todo = __ballot(w.valid);
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
        int pre = cnt;  // inclusive prefix of the nine counts over lanes 0..8
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
        for (int base = 0; base < total; base += CC_STAGE) {
            const int c = min(CC_STAGE, total - base);
#pragma unroll
            for (int k = 0; k < CC_STAGE / 64; ++k) {
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
            if (in_group) {  // the lanes of other groups have other cells: these records are not theirs to count
#pragma unroll 2
                for (int j = 0; j < c; ++j) visit(s_rec[j]);
            }
            __syncthreads();  // the stage is read before the next one, or the next group's tables, overwrite it
        }
        __syncthreads();  // total == 0: the tables are still read before the next group writes them
    }
    return w;
}

// d2 = (dx dx + dy dy) + dz dz in float32 without contraction (the library is built with -ffp-contract=off): float32 numpy's bits
__device__ __forceinline__ float pair_d2(const float4& q, const float4& p) {
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// count, the sum of the distances and the nine moments of the offsets v = double(p) - double(q): s[0] the distances, s[1..3] = sum v,
// s[4..9] = sum v_a v_b for a <= b, row-major
struct Moments {
    int count;
    double s[10];
    __device__ __forceinline__ void add(float qx, float qy, float qz, float px, float py, float pz, float dist) {
        const double vx = (double)px - (double)qx, vy = (double)py - (double)qy, vz = (double)pz - (double)qz;
        count += 1;
        s[0] += (double)dist;
        s[1] += vx;
        s[2] += vy;
        s[3] += vz;
        s[4] += vx * vx;
        s[5] += vx * vy;
        s[6] += vx * vz;
        s[7] += vy * vy;
        s[8] += vy * vz;
        s[9] += vz * vz;
    }
    __device__ __forceinline__ void store(long long row, int* __restrict__ count_out, double* __restrict__ sum_dist,
                                          double* __restrict__ moments) const {
        count_out[row] = count;
        sum_dist[row] = s[0];
#pragma unroll
        for (int k = 0; k < 9; ++k) moments[9 * row + k] = s[1 + k];
    }
};

__global__ void __launch_bounds__(64) radius_moments_kernel(const float4* __restrict__ qrec, int n, const float4* __restrict__ trec,
                                                            const long long* __restrict__ tkeys, int m, double ox, double oy, double oz,
                                                            double inv, float r2, int exclude_self, int* __restrict__ count,
                                                            double* __restrict__ sum_dist, double* __restrict__ moments) {
    Moments a{};
    float4 me = make_float4(0.f, 0.f, 0.f, 0.f);  // set before the first visit: the walk reads the record first
    int self = -1;
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i < n) {
        me = qrec[i];
        self = exclude_self ? __float_as_int(me.w) : -1;
    }
    const WaveQuery w = neighbour_walk(qrec, n, trec, tkeys, m, ox, oy, oz, inv, [&](const float4& p) {
        const float d2 = pair_d2(me, p);
        if (d2 < r2 && __float_as_int(p.w) != self) a.add(me.x, me.y, me.z, p.x, p.y, p.z, sqrtf(d2));  // a NaN is not < r2
    });
    if (!w.have) return;
    const int orig = __float_as_int(w.me.w);
    if ((unsigned)orig < (unsigned)n) a.store(orig, count, sum_dist, moments);
}

// ---- k nearest -----------------------------------------------------------------------------------------------------------------------
// cloud_nearest_kernel's 64-bit candidate, (bits of d2) << 32 | original index, kept as an ascending list of CAP in registers.  A
// candidate below the list's last entry is inserted by one pass of min / max over the list (fully unrolled: the list never leaves the
// registers); most staged records fail the test and cost one comparison.
constexpr unsigned long long KNN_NONE = 0xffffffffffffffffull;

template <int CAP>
__global__ void __launch_bounds__(64) knn_kernel(const float4* __restrict__ qrec, int n, const float4* __restrict__ trec,
                                                 const long long* __restrict__ tkeys, int m, double ox, double oy, double oz, double inv,
                                                 float max_dist, float r2, int k, int exclude_self, int* __restrict__ index,
                                                 float* __restrict__ dist, int* __restrict__ count) {
    unsigned long long list[CAP];
#pragma unroll
    for (int s = 0; s < CAP; ++s) list[s] = KNN_NONE;
    float4 me = make_float4(0.f, 0.f, 0.f, 0.f);
    int self = -1;
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i < n) {
        me = qrec[i];
        self = exclude_self ? __float_as_int(me.w) : -1;
    }
    const WaveQuery w = neighbour_walk(qrec, n, trec, tkeys, m, ox, oy, oz, inv, [&](const float4& p) {
        const float d2 = pair_d2(me, p);
        unsigned long long c = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(p.w);
        if (d2 < r2 && __float_as_int(p.w) != self && c < list[CAP - 1]) {
#pragma unroll
            for (int s = 0; s < CAP; ++s) {
                const unsigned long long lo = c < list[s] ? c : list[s];
                c = c < list[s] ? list[s] : c;
                list[s] = lo;
            }
        }
    });
    if (!w.have) return;
    const int orig = __float_as_int(w.me.w);
    if ((unsigned)orig >= (unsigned)n) return;
    int found = 0;
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
        if (s < k) {
            const bool ok = list[s] != KNN_NONE;
            found += ok ? 1 : 0;
            index[(long long)orig * k + s] = ok ? (int)(unsigned)(list[s] & 0xffffffffull) : -1;
            dist[(long long)orig * k + s] = ok ? sqrtf(__uint_as_float((unsigned)(list[s] >> 32))) : max_dist;
        }
    }
    count[orig] = found;
}

__global__ void __launch_bounds__(256) list_moments_kernel(const float* __restrict__ qpts, int n, const float* __restrict__ tpts, int m,
                                                           const int* __restrict__ index, const float* __restrict__ dist, int k,
                                                           int* __restrict__ count, double* __restrict__ sum_dist,
                                                           double* __restrict__ moments) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float qx = qpts[3 * i], qy = qpts[3 * i + 1], qz = qpts[3 * i + 2];
    Moments a{};
    for (int s = 0; s < k; ++s) {
        const int j = index[i * k + s];
        if ((unsigned)j >= (unsigned)m) break;  // -1 ends the list; an index out of range is never dereferenced
        a.add(qx, qy, qz, tpts[3 * (long long)j], tpts[3 * (long long)j + 1], tpts[3 * (long long)j + 2], dist[i * k + s]);
    }
    a.store(i, count, sum_dist, moments);
}

// ---- normals ---------------------------------------------------------------------------------------------------------------------------
// One lane per point.  C = sum v v^T / N - m m^T with N = count + 1 (the point itself adds zeros).  Cyclic Jacobi, a fixed number of
// sweeps over (0,1), (0,2), (1,2): each rotation annihilates one off-diagonal entry with t = sign(theta) / (|theta| + sqrt(theta^2 + 1)),
// theta = (a_qq - a_pp) / (2 a_pq) (Rutishauser's form: |t| <= 1, no cancellation); an entry that is already zero rotates by nothing.
// For a 3 x 3 matrix the off-diagonal norm falls quadratically after the first sweep or two: eight sweeps leave it at rounding level for
// every matrix, and the eigenvector of a gap g relative to the largest eigenvalue is within a few 2^-53 / g of the true one.
constexpr int JACOBI_SWEEPS = 8;
constexpr int ORIENT_NONE = 0, ORIENT_VIEWPOINT = 1, ORIENT_VIEWPOINTS = 2, ORIENT_LIKE = 3;

__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3], int p, int q) {
    const double apq = a[p][q];
    if (apq == 0.0) return;
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    const double t = isfinite(theta) ? copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0)) : 0.0;  // theta^2 = inf: t = 0
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const int r = 3 - p - q;  // the third index
    const double arp = a[r][p], arq = a[r][q];
    a[p][p] -= t * apq;
    a[q][q] += t * apq;
    a[p][q] = a[q][p] = 0.0;
    a[r][p] = a[p][r] = c * arp - s * arq;
    a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vp = v[k][p], vq = v[k][q];
        v[k][p] = c * vp - s * vq;
        v[k][q] = s * vp + c * vq;
    }
}

__global__ void __launch_bounds__(256) normals_kernel(const float* __restrict__ pts, int n, const int* __restrict__ count,
                                                      const double* __restrict__ moments, int min_neighbours, int orient, double wx,
                                                      double wy, double wz, const float* __restrict__ toward, float* __restrict__ normal,
                                                      float* __restrict__ curvature) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float qx = pts[3 * i], qy = pts[3 * i + 1], qz = pts[3 * i + 2];
    const int cnt = count[i];
    float out[3] = {0.f, 0.f, 0.f}, curv = NAN;
    if (finite3(qx, qy, qz) && cnt >= min_neighbours) {
        const double N = (double)cnt + 1.0;
        const double* M = moments + 9 * i;
        const double mx = M[0] / N, my = M[1] / N, mz = M[2] / N;
        double a[3][3], v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        a[0][0] = M[3] / N - mx * mx;
        a[0][1] = a[1][0] = M[4] / N - mx * my;
        a[0][2] = a[2][0] = M[5] / N - mx * mz;
        a[1][1] = M[6] / N - my * my;
        a[1][2] = a[2][1] = M[7] / N - my * mz;
        a[2][2] = M[8] / N - mz * mz;
        for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
            jacobi_rotate(a, v, 0, 1);
            jacobi_rotate(a, v, 0, 2);
            jacobi_rotate(a, v, 1, 2);
        }
        // the smallest eigenvalue's column (the first among equals), and the other two in order
        const double e0 = a[0][0], e1 = a[1][1], e2 = a[2][2];
        const int k0 = (e0 <= e1 && e0 <= e2) ? 0 : (e1 <= e2 ? 1 : 2);
        const double l0 = k0 == 0 ? e0 : (k0 == 1 ? e1 : e2);
        const double oa = k0 == 0 ? e1 : e0, ob = k0 == 2 ? e1 : e2;
        const double l1 = fmin(oa, ob), l2 = fmax(oa, ob);
        if (l1 > 1e-9 * l2) {  // false for a NaN too
            double nx = k0 == 0 ? v[0][0] : (k0 == 1 ? v[0][1] : v[0][2]);
            double ny = k0 == 0 ? v[1][0] : (k0 == 1 ? v[1][1] : v[1][2]);
            double nz = k0 == 0 ? v[2][0] : (k0 == 1 ? v[2][1] : v[2][2]);
            const double len = sqrt((nx * nx + ny * ny) + nz * nz);
            nx /= len, ny /= len, nz /= len;
            double dot = 0.0;
            if (orient == ORIENT_VIEWPOINT || orient == ORIENT_VIEWPOINTS) {
                if (orient == ORIENT_VIEWPOINTS) wx = (double)toward[3 * i], wy = (double)toward[3 * i + 1], wz = (double)toward[3 * i + 2];
                dot = (nx * (wx - (double)qx) + ny * (wy - (double)qy)) + nz * (wz - (double)qz);
            } else if (orient == ORIENT_LIKE) {
                dot = (nx * (double)toward[3 * i] + ny * (double)toward[3 * i + 1]) + nz * (double)toward[3 * i + 2];
            }
            bool flip = dot < 0.0;
            if (!(dot < 0.0) && !(dot > 0.0)) {  // no orientation, a dot of 0 or a NaN: the component of largest magnitude is positive
                const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
                const double big = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
                flip = big < 0.0;
            }
            if (flip) nx = -nx, ny = -ny, nz = -nz;
            out[0] = (float)nx, out[1] = (float)ny, out[2] = (float)nz;
            const double sum = (l0 + l1) + l2;
            curv = sum == 0.0 ? 0.f : (float)(l0 / sum);
        }
    }
    normal[3 * i] = out[0], normal[3 * i + 1] = out[1], normal[3 * i + 2] = out[2];
    curvature[i] = curv;
}

// ---- verdicts ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) keep_density_kernel(const float* __restrict__ pts, const int* __restrict__ count, int n,
                                                           int min_neighbours, unsigned char* __restrict__ keep) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keep[i] = finite3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]) && count[i] >= min_neighbours ? 1 : 0;
}

// mean_i = (sum of double(dist) over the list, in list order) / k for a point with a FULL list, and the two-level sums of fixed_sums.h over
// those points: the float64 sum of the means, of their squares, and their number.
constexpr int KM_PER_THREAD = 8;
constexpr int KM_PER_WG = FS_THREADS * KM_PER_THREAD;
using MeanRecord = FixedRecord<3, 3ull, 4>;  // two doubles, an int64 and a word of padding: 32 bytes

__global__ void __launch_bounds__(FS_THREADS) knn_mean_partial_kernel(const float* __restrict__ dist, const int* __restrict__ count, int n,
                                                                      int k, double* __restrict__ mean,
                                                                      unsigned char* __restrict__ partials) {
    MeanRecord a{};
    const long long base = (long long)blockIdx.x * KM_PER_WG + threadIdx.x;
#pragma unroll
    for (int t = 0; t < KM_PER_THREAD; ++t) {
        const long long i = base + (long long)t * FS_THREADS;
        if (i >= n) break;
        double mu = NAN;
        if (count[i] == k) {
            double s = 0.0;
            for (int j = 0; j < k; ++j) s += (double)dist[i * k + j];
            mu = s / (double)k;
            a.addf(0, mu);
            a.addf(1, mu * mu);
            a.addi(2, 1);
        }
        mean[i] = mu;
    }
    fixed_reduce_store(a, partials + (size_t)blockIdx.x * MeanRecord::block_bytes);
}

__global__ void __launch_bounds__(256) keep_threshold_kernel(const double* __restrict__ mean, int n, double threshold,
                                                             unsigned char* __restrict__ keep) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keep[i] = mean[i] <= threshold ? 1 : 0;  // a NaN (no full list) is dropped
}

// ---- selection -------------------------------------------------------------------------------------------------------------------------
struct KeepByte {
    const unsigned char* keep;
    __device__ bool operator()(long long p) const { return keep[p] != 0; }
};

__global__ void __launch_bounds__(CP_THREADS) select_kernel(const unsigned char* __restrict__ keep, int n,
                                                            const unsigned* __restrict__ offsets, int* __restrict__ kept,
                                                            int* __restrict__ remap) {
    const long long base = compact_wave_chunk() * CP_CHUNK + (threadIdx.x & 63);
#pragma unroll
    for (int k = 0; k < CP_SUB; ++k) {
        const long long p = base + 64 * k;
        if (p < n && keep[p] == 0) remap[p] = -1;
    }
    compact_walk(KeepByte{keep}, offsets, n, [&](long long p, long long slot) {
        kept[slot] = (int)p;
        remap[p] = (int)slot;
    });
}

static int check_grid_args(const char* what, long long n, long long m, double ox, double oy, double oz, double inv, float radius) {
    MVD_REQUIRE(n >= 0 && n <= 0x7fffffffLL && m >= 0 && m <= 0x7fffffffLL, "%s: %lld queries and %lld targets, supported 0 .. 2^31 - 1",
                what, n, m);
    MVD_REQUIRE(radius > 0.f && finite_f32(radius) && finite_f32(radius * radius), "%s: the radius must be finite and > 0, got %g", what,
                (double)radius);
    MVD_REQUIRE(isfinite(ox) && isfinite(oy) && isfinite(oz), "%s: the origin is not finite", what);
    MVD_REQUIRE(isfinite(inv) && inv > 0.0, "%s: inv must be finite and > 0, got %g", what, inv);
    MVD_REQUIRE(inv * ((double)radius * (1.0 + 1.0 / 1024.0)) <= 1.0 + 1e-12, "%s: the cell edge %g is below radius (1 + 2^-10) = %g", what,
                1.0 / inv, (double)radius * (1.0 + 1.0 / 1024.0));
    return MVD_OK;
}

}  // namespace mvd

extern "C" int mvd_cloud_radius_moments_f32(const float* query_records, long long n, const float* target_records,
                                            const long long* target_keys, long long m, double origin_x, double origin_y, double origin_z,
                                            double inv, float radius, int exclude_self, int* count, double* sum_dist, double* moments,
                                            mvd_stream_t stream) {
    using namespace mvd;
    if (int rc = check_grid_args("cloud_radius_moments", n, m, origin_x, origin_y, origin_z, inv, radius)) return rc;
    if (n == 0) return MVD_OK;
    MVD_REQUIRE(query_records && count && sum_dist && moments, "cloud_radius_moments: NULL argument");
    MVD_REQUIRE(m == 0 || (target_records && target_keys), "cloud_radius_moments: NULL target");
    MVD_REQUIRE((((uintptr_t)query_records | (uintptr_t)target_records) & 15) == 0, "cloud_radius_moments: records must be 16-byte aligned");
    MVD_REQUIRE((((uintptr_t)sum_dist | (uintptr_t)moments) & 7) == 0, "cloud_radius_moments: the sums must be 8-byte aligned");
    hipLaunchKernelGGL(radius_moments_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(query_records), (int)n, reinterpret_cast<const float4*>(target_records), target_keys,
                       (int)m, origin_x, origin_y, origin_z, inv, radius * radius, exclude_self ? 1 : 0, count, sum_dist, moments);
    return launch_status("cloud_radius_moments");
}

extern "C" int mvd_cloud_knn_f32(const float* query_records, long long n, const float* target_records, const long long* target_keys,
                                 long long m, double origin_x, double origin_y, double origin_z, double inv, float max_dist, int k,
                                 int exclude_self, int* index, float* dist, int* count, mvd_stream_t stream) {
    using namespace mvd;
    if (int rc = check_grid_args("cloud_knn", n, m, origin_x, origin_y, origin_z, inv, max_dist)) return rc;
    MVD_REQUIRE(k >= 1 && k <= MVD_CLOUD_KNN_MAX, "cloud_knn: k = %d, supported 1..%d", k, MVD_CLOUD_KNN_MAX);
    MVD_REQUIRE(n * k <= 0x7fffffffLL, "cloud_knn: %lld list entries, supported below 2^31", n * k);
    if (n == 0) return MVD_OK;
    MVD_REQUIRE(query_records && index && dist && count, "cloud_knn: NULL argument");
    MVD_REQUIRE(m == 0 || (target_records && target_keys), "cloud_knn: NULL target");
    MVD_REQUIRE((((uintptr_t)query_records | (uintptr_t)target_records) & 15) == 0, "cloud_knn: records must be 16-byte aligned");
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    const float4* q = reinterpret_cast<const float4*>(query_records);
    const float4* t = reinterpret_cast<const float4*>(target_records);
    const float r2 = max_dist * max_dist;
    const int self = exclude_self ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    // the list capacity is a template argument (the list lives in registers): a k between two capacities is served by the next one
    if (k <= 4)
        hipLaunchKernelGGL(knn_kernel<4>, grid, block, 0, st, q, (int)n, t, target_keys, (int)m, origin_x, origin_y, origin_z, inv, max_dist,
                           r2, k, self, index, dist, count);
    else if (k <= 8)
        hipLaunchKernelGGL(knn_kernel<8>, grid, block, 0, st, q, (int)n, t, target_keys, (int)m, origin_x, origin_y, origin_z, inv, max_dist,
                           r2, k, self, index, dist, count);
    else
        hipLaunchKernelGGL(knn_kernel<16>, grid, block, 0, st, q, (int)n, t, target_keys, (int)m, origin_x, origin_y, origin_z, inv, max_dist,
                           r2, k, self, index, dist, count);
    return launch_status("cloud_knn");
}

extern "C" int mvd_cloud_list_moments_f32(const float* queries, long long n, const float* targets, long long m, const int* index,
                                          const float* dist, int k, int* count, double* sum_dist, double* moments, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_list_moments", "points", n);
    MVD_REQUIRE_COUNT("cloud_list_moments", "points", m);
    MVD_REQUIRE(k >= 1 && k <= MVD_CLOUD_KNN_MAX, "cloud_list_moments: k = %d, supported 1..%d", k, MVD_CLOUD_KNN_MAX);
    MVD_REQUIRE(n * k <= 0x7fffffffLL, "cloud_list_moments: %lld list entries, supported below 2^31", n * k);
    if (n == 0) return MVD_OK;
    MVD_REQUIRE(queries && index && dist && count && sum_dist && moments, "cloud_list_moments: NULL argument");
    MVD_REQUIRE(m == 0 || targets, "cloud_list_moments: NULL target");
    MVD_REQUIRE((((uintptr_t)sum_dist | (uintptr_t)moments) & 7) == 0, "cloud_list_moments: the sums must be 8-byte aligned");
    hipLaunchKernelGGL(list_moments_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, queries, (int)n, targets,
                       (int)m, index, dist, k, count, sum_dist, moments);
    return launch_status("cloud_list_moments");
}

extern "C" int mvd_cloud_normals_f64(const float* points, long long n, const int* count, const double* moments, int min_neighbours,
                                     int orient, double toward_x, double toward_y, double toward_z, const float* toward, float* normal,
                                     float* curvature, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_normals", "points", n);
    MVD_REQUIRE(min_neighbours >= 2, "cloud_normals: min_neighbours = %d, at least 2", min_neighbours);
    MVD_REQUIRE(orient >= ORIENT_NONE && orient <= ORIENT_LIKE, "cloud_normals: orient = %d, supported 0..3", orient);
    MVD_REQUIRE(orient != ORIENT_VIEWPOINT || (isfinite(toward_x) && isfinite(toward_y) && isfinite(toward_z)),
                "cloud_normals: the viewpoint is not finite");
    if (n == 0) return MVD_OK;
    MVD_REQUIRE(points && count && moments && normal && curvature, "cloud_normals: NULL argument");
    MVD_REQUIRE(((uintptr_t)moments & 7) == 0, "cloud_normals: moments must be 8-byte aligned");
    MVD_REQUIRE((orient == ORIENT_VIEWPOINTS || orient == ORIENT_LIKE) == (toward != nullptr),
                "cloud_normals: the per-point array goes with orient 2 and 3");
    hipLaunchKernelGGL(normals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, (int)n, count, moments,
                       min_neighbours, orient, toward_x, toward_y, toward_z, toward, normal, curvature);
    return launch_status("cloud_normals");
}

extern "C" int mvd_cloud_keep_density(const float* points, const int* count, long long n, int min_neighbours, unsigned char* keep,
                                      mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_keep_density", "points", n);
    MVD_REQUIRE(min_neighbours >= 0, "cloud_keep_density: min_neighbours = %d, at least 0", min_neighbours);
    if (n == 0) return MVD_OK;
    MVD_REQUIRE(points && count && keep, "cloud_keep_density: NULL argument");
    hipLaunchKernelGGL(keep_density_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, count, (int)n,
                       min_neighbours, keep);
    return launch_status("cloud_keep_density");
}

extern "C" size_t mvd_cloud_knn_mean_sums_workspace_bytes(long long n) {
    if (n <= 0) return 0;
    return mvd::align_up(mvd::fixed_partials_bytes<mvd::MeanRecord>(n, mvd::KM_PER_WG), 256);
}

extern "C" int mvd_cloud_knn_mean_sums_f32(const float* dist, const int* count, long long n, int k, double* mean, void* result,
                                           void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_knn_mean_sums", "points", n);
    MVD_REQUIRE(k >= 1 && k <= MVD_CLOUD_KNN_MAX, "cloud_knn_mean_sums: k = %d, supported 1..%d", k, MVD_CLOUD_KNN_MAX);
    MVD_REQUIRE(n * k <= 0x7fffffffLL, "cloud_knn_mean_sums: %lld list entries, supported below 2^31", n * k);
    MVD_REQUIRE(result && ((uintptr_t)result & 7) == 0, "cloud_knn_mean_sums: result must be given and 8-byte aligned");
    MVD_REQUIRE(n == 0 || (dist && count && mean && ((uintptr_t)mean & 7) == 0), "cloud_knn_mean_sums: NULL or misaligned argument");
    MVD_REQUIRE(n == 0 || (workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= mvd_cloud_knn_mean_sums_workspace_bytes(n)),
                "cloud_knn_mean_sums: workspace too small or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nwg = (int)fixed_workgroups(n, KM_PER_WG);
    unsigned char* partials = static_cast<unsigned char*>(workspace);
    if (nwg > 0)
        hipLaunchKernelGGL(knn_mean_partial_kernel, dim3((unsigned)nwg), dim3(FS_THREADS), 0, st, dist, count, (int)n, k, mean, partials);
    fixed_final_launch<MeanRecord>(partials, nwg, result, st);
    return launch_status("cloud_knn_mean_sums");
}

extern "C" int mvd_cloud_keep_threshold(const double* mean, long long n, double threshold, unsigned char* keep, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_keep_threshold", "points", n);
    MVD_REQUIRE(!isnan(threshold), "cloud_keep_threshold: the threshold is NaN");
    if (n == 0) return MVD_OK;
    MVD_REQUIRE(mean && keep && ((uintptr_t)mean & 7) == 0, "cloud_keep_threshold: NULL or misaligned argument");
    hipLaunchKernelGGL(keep_threshold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mean, (int)n, threshold,
                       keep);
    return launch_status("cloud_keep_threshold");
}

extern "C" size_t mvd_cloud_select_workspace_bytes(long long n) {
    if (n <= 0) return 0;
    return mvd::compact_offsets_bytes(n);
}

extern "C" int mvd_cloud_select(const unsigned char* keep, long long n, int* kept, int* remap, long long* total, void* workspace,
                                size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("cloud_select", "points", n);
    MVD_REQUIRE(total && ((uintptr_t)total & 7) == 0, "cloud_select: total must be given and 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(total, 0, sizeof(long long), st) != hipSuccess) return launch_status("cloud_select");
        return MVD_OK;
    }
    MVD_REQUIRE(keep && kept && remap, "cloud_select: NULL argument");
    MVD_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0 && workspace_bytes >= mvd_cloud_select_workspace_bytes(n),
                "cloud_select: workspace too small or misaligned");
    const unsigned nwg = compact_workgroups(n);
    unsigned* chunk_counts = static_cast<unsigned*>(workspace);
    hipLaunchKernelGGL(compact_count_kernel<KeepByte>, dim3(nwg), dim3(CP_THREADS), 0, st, KeepByte{keep}, n, chunk_counts);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(CP_THREADS), 0, st, chunk_counts, compact_chunks(n), total);
    hipLaunchKernelGGL(select_kernel, dim3(nwg), dim3(CP_THREADS), 0, st, keep, (int)n, chunk_counts, kept, remap);
    return launch_status("cloud_select");
}
