// Mesh evaluation: the truncated distance from points to a triangle mesh on a sorted uniform grid over the triangles' boxes, and the
// deterministic covering samples of a mesh's surface.  The reference has NO counterpart (it ends at the per-view depth map), so there
// is no file:line to cite: the definition is the comment of these entries in include/mvd.h, restated in float64 numpy by
// robustmvd_amd/mesh_eval.py.
//   mvd_mesh_cell_counts_f32     triangle -> the number of grid cells its axis-aligned box covers (0: an invalid triangle)
//   mvd_mesh_pairs_f32           one (cell key, triangle) pair per cell of every box, in triangle order, x-major inside a box
//   mvd_mesh_records_f32         the sorted pairs' triangles gathered as 48-byte records (the three vertices, the triangle's index)
//   mvd_mesh_nearest_f32         per query the nearest triangle within max_dist: a wave stages the cells around its queries through LDS
//   mvd_mesh_sample_counts_f32   triangle -> k^2, the number of its samples at a spacing
//   mvd_mesh_sample_f32          the samples: the centroids of the k^2 congruent sub-triangles, with interpolated vertex attributes
// The grid's cells and keys are cloud_grid.h's, the ones of cloud_eval.hip.  No atomics anywhere: two calls give the same bits.  The
// prefix sums of the counts and the stable sort of the pair keys are the caller's (plumbing between two kernels).
#include <math.h>
#include <stdint.h>

#include "cloud_grid.h"

namespace mvd {

constexpr long long ME_COUNT_CAP = 1ll << 31;  // a triangle's count saturates here: the caller refuses such a total anyway
constexpr long long ME_K_CAP = 1ll << 26;      // k k is an exact double below this

struct MeshTri {
    float ax, ay, az, bx, by, bz, cx, cy, cz;
    bool ok;  // every index in [0, M) and every coordinate finite
};

__device__ __forceinline__ MeshTri load_triangle(const float* __restrict__ v, long long M, const int* __restrict__ tri, long long t) {
    MeshTri r{};
    const int i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    r.ok = (unsigned long long)i0 < (unsigned long long)M && i0 >= 0 && (unsigned long long)i1 < (unsigned long long)M && i1 >= 0 &&
           (unsigned long long)i2 < (unsigned long long)M && i2 >= 0;
    if (!r.ok) return r;
    r.ax = v[3 * (long long)i0], r.ay = v[3 * (long long)i0 + 1], r.az = v[3 * (long long)i0 + 2];
    r.bx = v[3 * (long long)i1], r.by = v[3 * (long long)i1 + 1], r.bz = v[3 * (long long)i1 + 2];
    r.cx = v[3 * (long long)i2], r.cy = v[3 * (long long)i2 + 1], r.cz = v[3 * (long long)i2 + 2];
    r.ok = finite3(r.ax, r.ay, r.az) && finite3(r.bx, r.by, r.bz) && finite3(r.cx, r.cy, r.cz);
    return r;
}

// the first position whose end is > p: ends are the inclusive prefix sums of non-negative counts, so this is the item that owns
// position p (items of count 0 own nothing and are passed over)
__device__ __forceinline__ long long owner_of(const long long* __restrict__ ends, long long T, long long p) {
    long long lo = 0, hi = T;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (ends[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- the triangle grid -------------------------------------------------------------------------------------------------------------
// A triangle's box in cells: per axis cell_index of the smallest and of the largest of its three coordinates, no dilation.  The
// indices are clamped into the key's range (the caller has checked the extent on the host).
struct CellBox {
    int x0, y0, z0, nx, ny, nz;
    __device__ long long volume() const { return (long long)nx * ny * nz; }  // <= (2^21)^3 < 2^63
};

__device__ __forceinline__ CellBox cell_box(const MeshTri& t, double ox, double oy, double oz, double inv) {
    const double hi = (double)(CE_LIMIT - 1);
    CellBox b;
    b.x0 = cell_index(fminf(t.ax, fminf(t.bx, t.cx)), ox, inv, 0.0, hi);
    b.y0 = cell_index(fminf(t.ay, fminf(t.by, t.cy)), oy, inv, 0.0, hi);
    b.z0 = cell_index(fminf(t.az, fminf(t.bz, t.cz)), oz, inv, 0.0, hi);
    b.nx = cell_index(fmaxf(t.ax, fmaxf(t.bx, t.cx)), ox, inv, 0.0, hi) - b.x0 + 1;
    b.ny = cell_index(fmaxf(t.ay, fmaxf(t.by, t.cy)), oy, inv, 0.0, hi) - b.y0 + 1;
    b.nz = cell_index(fmaxf(t.az, fmaxf(t.bz, t.cz)), oz, inv, 0.0, hi) - b.z0 + 1;
    return b;
}

__global__ void __launch_bounds__(256) mesh_cell_counts_kernel(const float* __restrict__ v, long long M, const int* __restrict__ tri,
                                                               int T, double ox, double oy, double oz, double inv,
                                                               long long* __restrict__ counts) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const MeshTri m = load_triangle(v, M, tri, t);
    counts[t] = m.ok ? min(cell_box(m, ox, oy, oz, inv).volume(), ME_COUNT_CAP) : 0ll;
}

// One lane per pair, so that one huge triangle does not serialise a lane: the triangle from the offsets, the cell from the rank
// inside the box (x-major, then y, then z).
__global__ void __launch_bounds__(256) mesh_pairs_kernel(const float* __restrict__ v, long long M, const int* __restrict__ tri, int T,
                                                         const long long* __restrict__ ends, int P, double ox, double oy, double oz,
                                                         double inv, long long* __restrict__ keys, int* __restrict__ pair_tri) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const long long t = owner_of(ends, T, p);
    long long key = CE_INVALID_KEY;
    int owner = -1;
    if (t < T) {
        const MeshTri m = load_triangle(v, M, tri, t);
        const long long rank = p - (t > 0 ? ends[t - 1] : 0ll);
        if (m.ok) {
            const CellBox b = cell_box(m, ox, oy, oz, inv);
            if (rank >= 0 && rank < b.volume()) {  // ends that are not the counts' prefix sums: a pair that matches nothing
                const int dz = (int)(rank % b.nz), dy = (int)((rank / b.nz) % b.ny), dx = (int)(rank / ((long long)b.nz * b.ny));
                key = cell_key(b.x0 + dx, b.y0 + dy, b.z0 + dz);
                owner = (int)t;
            }
        }
    }
    keys[p] = key;
    pair_tri[p] = owner;
}

// 48 bytes per sorted pair: (Ax Ay Az Bx) (By Bz Cx Cy) (Cz index 0 0).  A pair out of range: NaNs, a record that matches nothing.
constexpr int ME_REC4 = 3;  // float4s per record

__global__ void __launch_bounds__(256) mesh_records_kernel(const float* __restrict__ v, long long M, const int* __restrict__ tri, int T,
                                                           const int* __restrict__ pair_tri, const long long* __restrict__ perm, int P,
                                                           float4* __restrict__ rec) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const long long p = perm[i];
    float4 r0 = make_float4(NAN, NAN, NAN, NAN), r1 = r0, r2 = make_float4(NAN, __int_as_float(0), 0.f, 0.f);
    if ((unsigned long long)p < (unsigned long long)P) {
        const int t = pair_tri[p];
        if ((unsigned)t < (unsigned)T) {
            const MeshTri m = load_triangle(v, M, tri, t);
            if (m.ok) {
                r0 = make_float4(m.ax, m.ay, m.az, m.bx);
                r1 = make_float4(m.by, m.bz, m.cx, m.cy);
                r2 = make_float4(m.cz, __int_as_float(t), 0.f, 0.f);
            }
        }
    }
    rec[ME_REC4 * i] = r0;
    rec[ME_REC4 * i + 1] = r1;
    rec[ME_REC4 * i + 2] = r2;
}

// ---- point-to-triangle distance ----------------------------------------------------------------------------------------------------
// The definition's chain (include/mvd.h) with everything relative to the query: a = A - q, b = B - q, c = C - q, the edges from the
// vertices.  The squared distance is the smallest of the three segment distances and, where the query projects inside, of the plane
// distance: no region case analysis, and no division that a degenerate triangle can poison (ee == 0 gives t = 0, nn == 0 no plane).
// The sums are FMAs and the two divisions reciprocals (1 ulp), which the tests' band (four times the gap between the float32 and
// the float64 numpy chain) allows: an error in t moves the segment distance in second order only, being at its minimum.
__device__ __forceinline__ float dot3(float ux, float uy, float uz, float vx, float vy, float vz) {
    return fmaf(ux, vx, fmaf(uy, vy, uz * vz));
}

__device__ __forceinline__ float segment_d2(float px, float py, float pz, float ex, float ey, float ez) {
    const float ee = dot3(ex, ey, ez, ex, ey, ez);
    const float pe = dot3(px, py, pz, ex, ey, ez);
    float t = fminf(fmaxf(-pe * __builtin_amdgcn_rcpf(ee), 0.f), 1.f);  // fmaxf drops a NaN
    t = ee > 0.f ? t : 0.f;
    const float rx = fmaf(t, ex, px), ry = fmaf(t, ey, py), rz = fmaf(t, ez, pz);
    return dot3(rx, ry, rz, rx, ry, rz);
}

// n . (p x e)
__device__ __forceinline__ float side(float nx, float ny, float nz, float px, float py, float pz, float ex, float ey, float ez) {
    const float cx = fmaf(py, ez, -(pz * ey)), cy = fmaf(pz, ex, -(px * ez)), cz = fmaf(px, ey, -(py * ex));
    return dot3(nx, ny, nz, cx, cy, cz);
}

__device__ __forceinline__ float triangle_d2(float qx, float qy, float qz, const float4 r0, const float4 r1, const float4 r2) {
    const float ax = r0.x - qx, ay = r0.y - qy, az = r0.z - qz;
    const float bx = r0.w - qx, by = r1.x - qy, bz = r1.y - qz;
    const float cx = r1.z - qx, cy = r1.w - qy, cz = r2.x - qz;
    const float e0x = r0.w - r0.x, e0y = r1.x - r0.y, e0z = r1.y - r0.z;
    const float e1x = r1.z - r0.w, e1y = r1.w - r1.x, e1z = r2.x - r1.y;
    const float e2x = r0.x - r1.z, e2y = r0.y - r1.w, e2z = r0.z - r2.x;
    float d2 = fminf(segment_d2(ax, ay, az, e0x, e0y, e0z), fminf(segment_d2(bx, by, bz, e1x, e1y, e1z), segment_d2(cx, cy, cz, e2x, e2y, e2z)));
    const float nx = fmaf(e0y, e1z, -(e0z * e1y)), ny = fmaf(e0z, e1x, -(e0x * e1z)), nz = fmaf(e0x, e1y, -(e0y * e1x));
    const float nn = dot3(nx, ny, nz, nx, ny, nz);
    const bool inside = nn > 0.f && side(nx, ny, nz, ax, ay, az, e0x, e0y, e0z) >= 0.f && side(nx, ny, nz, bx, by, bz, e1x, e1y, e1z) >= 0.f &&
                        side(nx, ny, nz, cx, cy, cz, e2x, e2y, e2z) >= 0.f;
    const float na = dot3(nx, ny, nz, ax, ay, az);
    const float plane = na * na * __builtin_amdgcn_rcpf(nn);
    return inside ? fminf(d2, plane) : d2;
}

// ---- nearest triangle --------------------------------------------------------------------------------------------------------------
// cloud_nearest_kernel's structure (cloud_eval.hip) with triangle records in place of points.  One wave (= one workgroup) per 64
// consecutive query records, which come sorted by the cell keys of the same grid.  The first query not yet served leads; its group is
// every unserved query of the same (x, y) column whose z index is within 3 above the leader's.  With z in the key's low bits the cells
// (x', y', z_lead - 1 .. z_lead + 4) of one of the nine neighbouring columns are ONE run of the sorted pair keys, found by two binary
// searches; lanes 0..8 search the nine runs at once.  The runs are treated as one list of records, staged through LDS 128 records
// (6 KB) at a time, six 16-byte loads in flight per lane, and EVERY lane scans every staged record with three broadcast
// ds_read_b128s (all lanes on one address: no bank conflict).  A record outside a lane's own 27 cells is still a triangle of the
// mesh, and a triangle that sits in several scanned cells is simply seen several times: neither can make the minimum wrong.
// Nothing is sized by a cell's population.
//
// Why the 27 cells are enough.  Let the computed distance of q to a triangle be < max_dist, and let p be the triangle's point
// nearest to q.  |q - p| is within max_dist 2^-11 of the computed distance (a few float32 roundings of differences of that size;
// a needle whose normal has lost its digits is outside this claim, and a query that far off on such a triangle sits at the
// truncation's edge either way), so per axis |q_a - p_a| < max_dist (1 + 2^-11).  The entry requires a cell edge
// c >= max_dist (1 + 2^-10), so |q_a - p_a| * inv < (1 + 2^-11) / (1 + 2^-10) < 1 - 2^-12.  The index is the floor of
// t(v) = fl((v - o) * inv), which is non-decreasing in the real v and within 2^-30 of (v - o) * inv for |t| < 2^22 (the argument above
// cloud_nearest_kernel).  So the floors of t(q_a) and t(p_a) differ by at most one on every axis: p's cell is one of the 27.  And p
// lies in the triangle's box, min_a <= p_a <= max_a, so by monotonicity floor t(min_a) <= floor t(p_a) <= floor t(max_a): p's
// cell is one of the box's cells, each of which lists the triangle.  A query's indices are clamped to [-2, CE_LIMIT + 2], which
// moves only queries at least two cells outside the grid.
//
// The best candidate is the minimum of (bits of d^2) << 32 | triangle as an unsigned 64-bit number, as in cloud_nearest_kernel.
constexpr int MN_STAGE = 128;

__global__ void __launch_bounds__(64) mesh_nearest_kernel(const float4* __restrict__ qrec, int n, const float4* __restrict__ trec,
                                                          const long long* __restrict__ tkeys, int m, double ox, double oy, double oz,
                                                          double inv, float max_dist, float* __restrict__ dist,
                                                          int* __restrict__ index) {
    __shared__ float4 s_rec[MN_STAGE * ME_REC4];
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
        for (int base = 0; base < total; base += MN_STAGE) {
            const int c = min(MN_STAGE, total - base);
#pragma unroll
            for (int k = 0; k < MN_STAGE * ME_REC4 / 64; ++k) {
                const int slot = lane + 64 * k, rec = slot / ME_REC4, f = base + rec;
                if (rec < c) {
                    int r = 0;
#pragma unroll
                    for (int r2 = 1; r2 < 9; ++r2)
                        if (f >= s_pre[r2]) r = r2;
                    // record s_lo[r] + (f - s_pre[r]) is inside [lo_r, hi_r), a sub-range of [0, m)
                    s_rec[slot] = trec[(long long)ME_REC4 * (s_lo[r] + (f - s_pre[r])) + (slot - ME_REC4 * rec)];
                }
            }
            __syncthreads();
#pragma unroll 2
            for (int j = 0; j < c; ++j) {
                const float4 r0 = s_rec[ME_REC4 * j], r1 = s_rec[ME_REC4 * j + 1], r2 = s_rec[ME_REC4 * j + 2];
                const float d2 = triangle_d2(me.x, me.y, me.z, r0, r1, r2);
                const unsigned long long cand = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(r2.y);
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

// ---- surface samples ---------------------------------------------------------------------------------------------------------------
// The smallest integer k >= 1 with k k >= r, capped at ME_K_CAP: from (long)sqrt(r) with integer correction steps, so that it does
// not depend on how sqrt rounds.  k k is exact in double below the cap.
__device__ __forceinline__ long long ceil_sqrt(double r) {
    if (!(r < (double)ME_K_CAP * (double)ME_K_CAP)) return ME_K_CAP;  // also a NaN
    long long k = (long long)sqrt(r);
    if (k < 1) k = 1;
    while ((double)k * (double)k < r) ++k;
    while (k > 1 && (double)(k - 1) * (double)(k - 1) >= r) --k;
    return k;
}

__device__ __forceinline__ double edge2(float ux, float uy, float uz, float vx, float vy, float vz) {
    const double dx = (double)ux - (double)vx, dy = (double)uy - (double)vy, dz = (double)uz - (double)vz;
    return (dx * dx + dy * dy) + dz * dz;
}

// k = max(1, ceil(longest edge / spacing)) from r = L2 * inv_s2
__device__ __forceinline__ long long sample_k(const MeshTri& m, double inv_s2) {
    const double l2 = fmax(edge2(m.bx, m.by, m.bz, m.ax, m.ay, m.az),
                           fmax(edge2(m.cx, m.cy, m.cz, m.bx, m.by, m.bz), edge2(m.ax, m.ay, m.az, m.cx, m.cy, m.cz)));
    return ceil_sqrt(l2 * inv_s2);
}

__global__ void __launch_bounds__(256) mesh_sample_counts_kernel(const float* __restrict__ v, long long M, const int* __restrict__ tri,
                                                                 int T, double inv_s2, long long* __restrict__ counts) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const MeshTri m = load_triangle(v, M, tri, t);
    long long c = 0;
    if (m.ok) {
        const long long k = sample_k(m, inv_s2);
        c = min(k * k, ME_COUNT_CAP);
    }
    counts[t] = c;
}

// One lane per sample.  Rows i = 0..k-1 hold 2 (k - i) - 1 samples, so the rows from i on hold (k - i)^2: with m = k^2 - rank, the
// row's w = k - i is the smallest integer with w w >= m (the same integer square root), and the position in the row is w w - m.
template <bool ATTR>
__global__ void __launch_bounds__(256) mesh_sample_kernel(const float* __restrict__ v, long long M, const int* __restrict__ tri, int T,
                                                          const float* __restrict__ attr, int C, const long long* __restrict__ ends,
                                                          int S, double inv_s2, float* __restrict__ points,
                                                          int* __restrict__ sample_tri, float* __restrict__ out_attr) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const long long t = owner_of(ends, T, s);
    float px = NAN, py = NAN, pz = NAN;
    int owner = -1;
    double wa = 0.0, wb = 0.0, wc = 0.0;
    int i0 = 0, i1 = 0, i2 = 0;
    if (t < T) {
        const MeshTri m = load_triangle(v, M, tri, t);
        const long long rank = s - (t > 0 ? ends[t - 1] : 0ll);
        if (m.ok) {
            const long long k = sample_k(m, inv_s2);
            if (rank >= 0 && rank < k * k) {  // ends that are not the counts' prefix sums: a sample that belongs to nothing
                const long long left = k * k - rank;  // 1 .. k^2 < 2^31
                const long long w = ceil_sqrt((double)left);
                const long long i = k - w, pos = w * w - left, j = pos >> 1;
                const long long down = pos & 1;
                const double k3 = (double)(3 * k);
                wb = (double)(3 * i + 1 + down) / k3;
                wc = (double)(3 * j + 1 + down) / k3;
                wa = (double)(3 * (k - i - j) - 2 - 2 * down) / k3;
                px = (float)((wa * (double)m.ax + wb * (double)m.bx) + wc * (double)m.cx);
                py = (float)((wa * (double)m.ay + wb * (double)m.by) + wc * (double)m.cy);
                pz = (float)((wa * (double)m.az + wb * (double)m.bz) + wc * (double)m.cz);
                owner = (int)t;
                i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];  // in [0, M): m.ok
            }
        }
    }
    points[3 * s] = px, points[3 * s + 1] = py, points[3 * s + 2] = pz;
    sample_tri[s] = owner;
    if constexpr (ATTR) {
        for (int ch = 0; ch < C; ++ch) {
            float val = NAN;
            if (owner >= 0)
                val = (float)((wa * (double)attr[(long long)i0 * C + ch] + wb * (double)attr[(long long)i1 * C + ch]) +
                              wc * (double)attr[(long long)i2 * C + ch]);
            out_attr[s * C + ch] = val;
        }
    }
}

}  // namespace mvd

#define MESH_EVAL_REQUIRE_MESH(what)                                                                  \
    MVD_REQUIRE_COUNT(what, "vertices", M);                                                           \
    MVD_REQUIRE_COUNT(what, "triangles", T);                                                          \
    MVD_REQUIRE(T == 0 || triangles, what ": NULL triangles");                                        \
    MVD_REQUIRE(M == 0 || vertices, what ": NULL vertices")

#define MESH_EVAL_REQUIRE_GRID(what)                                                                                         \
    MVD_REQUIRE(isfinite(origin_x) && isfinite(origin_y) && isfinite(origin_z), what ": the origin is not finite");          \
    MVD_REQUIRE(isfinite(inv) && inv > 0.0, what ": inv must be finite and > 0, got %g", inv)

extern "C" int mvd_mesh_cell_counts_f32(const float* vertices, long long M, const int* triangles, long long T, double origin_x,
                                        double origin_y, double origin_z, double inv, long long* counts, mvd_stream_t stream) {
    using namespace mvd;
    MESH_EVAL_REQUIRE_MESH("mesh_cell_counts");
    MESH_EVAL_REQUIRE_GRID("mesh_cell_counts");
    if (T == 0) return MVD_OK;
    MVD_REQUIRE(counts, "mesh_cell_counts: NULL counts");
    hipLaunchKernelGGL(mesh_cell_counts_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices, M, triangles,
                       (int)T, origin_x, origin_y, origin_z, inv, counts);
    return launch_status("mesh_cell_counts");
}

extern "C" int mvd_mesh_pairs_f32(const float* vertices, long long M, const int* triangles, long long T, const long long* ends,
                                  long long P, double origin_x, double origin_y, double origin_z, double inv, long long* keys,
                                  int* pair_triangle, mvd_stream_t stream) {
    using namespace mvd;
    MESH_EVAL_REQUIRE_MESH("mesh_pairs");
    MESH_EVAL_REQUIRE_GRID("mesh_pairs");
    MVD_REQUIRE_COUNT("mesh_pairs", "pairs", P);
    if (P == 0) return MVD_OK;
    MVD_REQUIRE(T > 0 && ends && keys && pair_triangle, "mesh_pairs: %lld pairs need triangles, ends, keys and pair_triangle", P);
    hipLaunchKernelGGL(mesh_pairs_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices, M, triangles,
                       (int)T, ends, (int)P, origin_x, origin_y, origin_z, inv, keys, pair_triangle);
    return launch_status("mesh_pairs");
}

extern "C" int mvd_mesh_records_f32(const float* vertices, long long M, const int* triangles, long long T, const int* pair_triangle,
                                    const long long* perm, long long P, float* records, mvd_stream_t stream) {
    using namespace mvd;
    MESH_EVAL_REQUIRE_MESH("mesh_records");
    MVD_REQUIRE_COUNT("mesh_records", "pairs", P);
    if (P == 0) return MVD_OK;
    MVD_REQUIRE(T > 0 && pair_triangle && perm && records, "mesh_records: NULL argument");
    MVD_REQUIRE(((uintptr_t)records & 15) == 0, "mesh_records: records must be 16-byte aligned");
    hipLaunchKernelGGL(mesh_records_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices, M, triangles,
                       (int)T, pair_triangle, perm, (int)P, reinterpret_cast<float4*>(records));
    return launch_status("mesh_records");
}

extern "C" int mvd_mesh_nearest_f32(const float* query_records, long long n, const float* triangle_records, const long long* pair_keys,
                                    long long P, double origin_x, double origin_y, double origin_z, double inv, float max_dist,
                                    float* dist, int* index, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_nearest", "points", n);
    MVD_REQUIRE_COUNT("mesh_nearest", "pairs", P);
    MVD_REQUIRE(max_dist > 0.f && finite_f32(max_dist), "mesh_nearest: max_dist must be finite and > 0, got %g", (double)max_dist);
    MESH_EVAL_REQUIRE_GRID("mesh_nearest");
    MVD_REQUIRE(inv * ((double)max_dist * (1.0 + 1.0 / 1024.0)) <= 1.0 + 1e-12,
                "mesh_nearest: the cell edge %g is below max_dist (1 + 2^-10) = %g", 1.0 / inv, (double)max_dist * (1.0 + 1.0 / 1024.0));
    if (n == 0) return MVD_OK;
    MVD_REQUIRE(query_records && dist && index, "mesh_nearest: NULL argument");
    MVD_REQUIRE(P == 0 || (triangle_records && pair_keys), "mesh_nearest: NULL grid");
    MVD_REQUIRE((((uintptr_t)query_records | (uintptr_t)triangle_records) & 15) == 0, "mesh_nearest: records must be 16-byte aligned");
    hipLaunchKernelGGL(mesh_nearest_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(query_records), (int)n, reinterpret_cast<const float4*>(triangle_records), pair_keys,
                       (int)P, origin_x, origin_y, origin_z, inv, max_dist, dist, index);
    return launch_status("mesh_nearest");
}

extern "C" int mvd_mesh_sample_counts_f32(const float* vertices, long long M, const int* triangles, long long T, double inv_s2,
                                          long long* counts, mvd_stream_t stream) {
    using namespace mvd;
    MESH_EVAL_REQUIRE_MESH("mesh_sample_counts");
    MVD_REQUIRE(isfinite(inv_s2) && inv_s2 > 0.0, "mesh_sample_counts: inv_s2 must be finite and > 0, got %g", inv_s2);
    if (T == 0) return MVD_OK;
    MVD_REQUIRE(counts, "mesh_sample_counts: NULL counts");
    hipLaunchKernelGGL(mesh_sample_counts_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices, M,
                       triangles, (int)T, inv_s2, counts);
    return launch_status("mesh_sample_counts");
}

extern "C" int mvd_mesh_sample_f32(const float* vertices, long long M, const int* triangles, long long T, const float* attributes,
                                   int channels, const long long* ends, long long S, double inv_s2, float* points,
                                   int* sample_triangle, float* out_attributes, mvd_stream_t stream) {
    using namespace mvd;
    MESH_EVAL_REQUIRE_MESH("mesh_sample");
    MVD_REQUIRE_COUNT("mesh_sample", "samples", S);
    MVD_REQUIRE(isfinite(inv_s2) && inv_s2 > 0.0, "mesh_sample: inv_s2 must be finite and > 0, got %g", inv_s2);
    MVD_REQUIRE(!attributes == !out_attributes, "mesh_sample: attributes and out_attributes go together");
    MVD_REQUIRE(!attributes || (channels >= 1 && channels <= 65536), "mesh_sample: %d channels, supported 1..65536", channels);
    if (S == 0) return MVD_OK;
    MVD_REQUIRE(T > 0 && ends && points && sample_triangle, "mesh_sample: %lld samples need triangles, ends, points and sample_triangle", S);
    const dim3 grid((unsigned)((S + 255) / 256));
    if (attributes)
        hipLaunchKernelGGL(mesh_sample_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, vertices, M, triangles, (int)T, attributes,
                           channels, ends, (int)S, inv_s2, points, sample_triangle, out_attributes);
    else
        hipLaunchKernelGGL(mesh_sample_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, vertices, M, triangles, (int)T, attributes,
                           channels, ends, (int)S, inv_s2, points, sample_triangle, out_attributes);
    return launch_status("mesh_sample");
}
