// Float64 (and int64) sums whose order is fixed by the number of items alone: the one copy behind mvd_cloud_scores_f32 and
// mvd_voxel_reduce_f32 (cloud_eval.hip), mvd_cloud_pair_sums_f32 (cloud_register.hip) and mvd_mesh_component_sums_f64
// (mesh_clean.hip).  No atomics; the library is built without contraction, so two runs, and tests/sum_order.py's numpy, give the
// same bits.  Header-only, static / templated as compact.h is (the build has no relocatable device code).
//   wave sum     v += shfl_xor(v, s) for s = 32 .. 1: every lane ends with the same bits (a + b = b + a)
//   record       FixedRecord: K 8-byte words per thread, each a double or an int64.  fixed_reduce_store: the wave sum of every word,
//                lane 0 of each wave to LDS, then thread k adds word k over the waves in wave order and stores it
//   two levels   a kernel of the user's gives every workgroup of FS_THREADS threads fixed_workgroups(n, per_wg) consecutive items and
//                stores one record per workgroup (fixed_reduce_store); fixed_final_kernel, one workgroup, adds them: thread t the
//                records t, t + FS_THREADS, ... in that order, then fixed_reduce_store
//   segments     fixed_segment_walk: one lane per segment of an ascending table.  At most 64 items: the lane adds them in order.
//                More: the whole wave, lane l the items l, l + 64, ..., then the wave sum
// Not here: depth_eval.hip's block_sum.  It is an LDS halving tree over all 256 lanes, which adds lanes t and t + 128 first: another
// order across the waves than wave 0 + 1 + 2 + 3, and the bits it gives are pinned by test_hip_eval.py.
#pragma once
#include "mvd_common.h"

namespace mvd {

constexpr int FS_THREADS = 256;  // every kernel that calls fixed_reduce_store or fixed_segment_walk is launched with this many
constexpr int FS_WAVES = FS_THREADS / 64;
constexpr int FS_LONG = 64;  // segments above this length are added by the wave

__device__ __forceinline__ double fixed_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}
__device__ __forceinline__ long long fixed_wave_sum(long long v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// K words summed per thread, stored as a block of WORDS >= K words (the rest zeros).  Bit k of DOUBLES: word k is a double, kept as
// its bits; the others are int64.  Zero-initialise it (`Rec a{}`): +0.0 and 0.
template <int K, unsigned long long DOUBLES, int WORDS = K>
struct FixedRecord {
    static_assert(K >= 1 && K <= 64 && WORDS >= K && WORDS <= FS_THREADS, "one thread per word of the block");
    static constexpr int words = K, block_words = WORDS;
    static constexpr size_t block_bytes = (size_t)WORDS * 8;
    long long w[K];

    __device__ __forceinline__ void addf(int k, double v) { w[k] = __double_as_longlong(__longlong_as_double(w[k]) + v); }
    __device__ __forceinline__ void addi(int k, long long v) { w[k] += v; }
    // a + b for two values of word k, as its type says
    static __device__ __forceinline__ long long sum(int k, long long a, long long b) {
        return (DOUBLES >> k) & 1ull ? __double_as_longlong(__longlong_as_double(a) + __longlong_as_double(b)) : a + b;
    }
    static __device__ __forceinline__ long long wave_sum(int k, long long a) {
        return (DOUBLES >> k) & 1ull ? __double_as_longlong(fixed_wave_sum(__longlong_as_double(a))) : fixed_wave_sum(a);
    }
};

// The workgroup's sum of every thread's record into out[0 .. WORDS).  Every thread of the workgroup must call it (the barrier).
template <int K, unsigned long long DOUBLES, int WORDS>
__device__ __forceinline__ void fixed_reduce_store(FixedRecord<K, DOUBLES, WORDS> a, void* __restrict__ out) {
    using Rec = FixedRecord<K, DOUBLES, WORDS>;
    __shared__ long long s_w[FS_WAVES][K];
#pragma unroll
    for (int k = 0; k < K; ++k) a.w[k] = Rec::wave_sum(k, a.w[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_w[threadIdx.x >> 6][k] = a.w[k];
    }
    __syncthreads();
    const int word = threadIdx.x;  // one word of the block per thread, each summed over the waves in wave order
    if (word < K) {
        long long v = s_w[0][word];
        for (int wave = 1; wave < FS_WAVES; ++wave) v = Rec::sum(word, v, s_w[wave][word]);
        static_cast<long long*>(out)[word] = v;
    } else if (word < WORDS) {
        static_cast<long long*>(out)[word] = 0;
    }
}

// ---- two levels ------------------------------------------------------------------------------------------------------------------------
static inline long long fixed_workgroups(long long n, int per_wg) { return (n + per_wg - 1) / per_wg; }
template <class Rec>
static inline size_t fixed_partials_bytes(long long n, int per_wg) { return (size_t)fixed_workgroups(n, per_wg) * Rec::block_bytes; }

template <class Rec>
__global__ void __launch_bounds__(FS_THREADS) fixed_final_kernel(const long long* __restrict__ partials, int nwg, void* __restrict__ result) {
    Rec a{};
    for (int g = threadIdx.x; g < nwg; g += FS_THREADS) {
        const long long* p = partials + (size_t)g * Rec::block_words;
#pragma unroll
        for (int k = 0; k < Rec::words; ++k) a.w[k] = Rec::sum(k, a.w[k], p[k]);
    }
    fixed_reduce_store(a, result);
}

// the second level over the nwg records that the user's kernel left in `partials`; nwg == 0: a block of zeros
template <class Rec>
static inline void fixed_final_launch(const void* partials, int nwg, void* result, hipStream_t st) {
    hipLaunchKernelGGL(fixed_final_kernel<Rec>, dim3(1), dim3(FS_THREADS), 0, st, static_cast<const long long*>(partials), nwg, result);
}

// ---- segments --------------------------------------------------------------------------------------------------------------------------
template <int N>
struct FixedSums {
    double v[N];
};

// lane's share of the span [b, e): the items b + lane, b + lane + 64, ... in that order
template <int N, class Item>
__device__ __forceinline__ void fixed_lane_span(FixedSums<N>& s, long long b, long long e, int lane, const Item& item) {
    for (long long p = b + lane; p < e; p += 64) item(s, p);
}

// Segment c = positions [seg[c], seg[c + 1]) for c < nseg, the table ascending and ending at most at n; the clamps keep a corrupted
// table inside 0 .. n.  item(s, p) adds position p's item to s; span(s, b, e, lane) adds the calling lane's share of a long
// segment [b, e) (fixed_lane_span, or an order of the user's own); store(s, len, c) gets every finished segment once, from one lane.
// Launch FS_THREADS threads for every 256 segments; a wave whose segments start at or past nseg does nothing.  Every lane of the wave
// must call it (the ballot and the shuffles).
template <int N, class Item, class Span, class Store>
__device__ __forceinline__ void fixed_segment_walk(const int* __restrict__ seg, long long nseg, int n, const Item& item, const Span& span,
                                                   const Store& store) {
    const int lane = threadIdx.x & 63;
    const long long wave_base = ((long long)blockIdx.x * FS_WAVES + (threadIdx.x >> 6)) * 64;
    if (wave_base >= nseg) return;  // the whole wave
    const long long c = wave_base + lane;
    const bool have = c < nseg;
    const int b = have ? min(max(seg[c], 0), n) : 0, e = have ? min(max(seg[c + 1], b), n) : 0;
    if (have && e - b <= FS_LONG) {
        FixedSums<N> s{};
        for (int p = b; p < e; ++p) item(s, p);
        store(s, e - b, c);
    }
    unsigned long long longs = __ballot(have && e - b > FS_LONG);
    while (longs != 0ull) {  // wave-uniform
        const int owner = __ffsll((long long)longs) - 1;
        longs &= longs - 1ull;
        const int lb = __shfl(b, owner), le = __shfl(e, owner);
        FixedSums<N> s{};
        span(s, lb, le, lane);
#pragma unroll
        for (int k = 0; k < N; ++k) s.v[k] = fixed_wave_sum(s.v[k]);
        if (lane == 0) store(s, le - lb, wave_base + owner);
    }
}

}  // namespace mvd
