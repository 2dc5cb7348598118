// Deterministic, order-preserving stream compaction: the one copy behind mvd_compact_points_f32 (depth_fusion.hip: the masked pixels)
// and mvd_voxel_reduce_f32 (cloud_eval.hip: the segment heads of the sorted keys).  No atomic decides a position.
// A chunk is 256 consecutive elements, the four ballots of one wave, which keeps the one-workgroup scan at 14 counts per lane at
// 768 x 1152.  count: chunk -> the popcounts of its ballots; scan: one workgroup turns the counts into exclusive offsets in place
// and writes the total; walk (inside the user's own kernel): slot = offset of the chunk + the popcounts of the chunk's earlier
// ballots + the rank of the lane in its ballot.
// A predicate is a functor `bool operator()(long long p) const`, called only for p < n.  The count and the kernel that walks launch
// compact_workgroups(n) workgroups of CP_THREADS, the scan one.
#pragma once
#include "mvd_common.h"

namespace mvd {

constexpr int CP_THREADS = 256;
constexpr int CP_WAVES = CP_THREADS / 64;
constexpr int CP_SUB = 4;              // ballots per chunk
constexpr int CP_CHUNK = 64 * CP_SUB;  // elements per chunk

static inline long long compact_chunks(long long n) { return (n + CP_CHUNK - 1) / CP_CHUNK; }
static inline unsigned compact_workgroups(long long n) { return (unsigned)((compact_chunks(n) + CP_WAVES - 1) / CP_WAVES); }
// bytes of the per-chunk counts / offsets at the head of a workspace; what follows them starts 256-byte aligned
static inline size_t compact_offsets_bytes(long long n) { return align_up((size_t)compact_chunks(n) * sizeof(unsigned), 256); }

// the chunk of the calling wave; lane l tests its elements chunk * CP_CHUNK + l + 64 k, k = 0..3
__device__ __forceinline__ long long compact_wave_chunk() { return (long long)blockIdx.x * CP_WAVES + (threadIdx.x >> 6); }

template <class Pred>
__global__ void __launch_bounds__(CP_THREADS) compact_count_kernel(Pred pred, long long n, unsigned* __restrict__ counts) {
    const long long chunk = compact_wave_chunk();
    const long long base = chunk * CP_CHUNK + (threadIdx.x & 63);
    unsigned c = 0u;
#pragma unroll
    for (int k = 0; k < CP_SUB; ++k) {
        const long long p = base + 64 * k;
        const bool set = p < n && pred(p);
        c += (unsigned)__popcll(__ballot(set));
    }
    if ((threadIdx.x & 63) == 0 && chunk * CP_CHUNK < n) counts[chunk] = c;
}

// static: one copy per translation unit that launches it (the build has no relocatable device code)
static __global__ void __launch_bounds__(CP_THREADS) compact_scan_kernel(unsigned* __restrict__ counts, long long nchunks,
                                                                         long long* __restrict__ total) {
    __shared__ unsigned part[CP_THREADS];
    const int t = threadIdx.x;
    const long long per = (nchunks + CP_THREADS - 1) / CP_THREADS;
    // lane t owns counts [b, e): where 256 * per exceeds nchunks the last lanes' ranges are cut short or empty
    const long long b = min((long long)t * per, nchunks), e = min(b + per, nchunks);
    unsigned acc = 0u;
    for (long long i = b; i < e; ++i) acc += counts[i];
    part[t] = acc;
    __syncthreads();
    for (int s = 1; s < CP_THREADS; s <<= 1) {  // inclusive scan of the 256 segment sums
        const unsigned add = t >= s ? part[t - s] : 0u;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    unsigned run = part[t] - acc;  // exclusive
    for (long long i = b; i < e; ++i) {
        const unsigned c = counts[i];
        counts[i] = run;
        run += c;
    }
    if (t == CP_THREADS - 1) total[0] = (long long)part[t];
}

// The walk of the calling wave's chunk: every selected element p gets emit(p, slot), slot its position among all selected elements.
// The chunk's offset and the four predicates are asked for before the first ballot, so that their loads are in flight together.  A wave whose chunk
// starts at or past n does nothing.  Every lane of the wave must call it (the ballots).
template <class Pred, class Emit>
__device__ __forceinline__ void compact_walk(const Pred& pred, const unsigned* __restrict__ offsets, long long n, const Emit& emit) {
    const int lane = threadIdx.x & 63;
    const long long chunk = compact_wave_chunk();
    if (chunk * CP_CHUNK >= n) return;  // the whole wave
    const long long base = chunk * CP_CHUNK + lane;
    long long run = offsets[chunk];  // asked for first: a predicate whose loads depend on one another does not delay it
    bool set[CP_SUB];
#pragma unroll
    for (int k = 0; k < CP_SUB; ++k) set[k] = base + 64 * k < n && pred(base + 64 * k);
#pragma unroll
    for (int k = 0; k < CP_SUB; ++k) {
        const unsigned long long ballot = __ballot(set[k]);
        if (set[k]) emit(base + 64 * k, run + __popcll(ballot & ((1ull << lane) - 1ull)));
        run += __popcll(ballot);
    }
}

// ---- the counted form (tsdf.hip: a voxel's mesh vertices and a cell's triangles) ---------------------------------------------------
// Every element selects `count` consecutive slots, 0 <= count <= CP_MAX_COUNT, instead of 0 or 1; the chunk, the scan and the walk keep
// their shape.  A count is a functor `unsigned operator()(long long p) const`, called only for p < n.  The chunk sums go through the
// same compact_scan_kernel: a total is exact while it is below 2^32.
constexpr unsigned CP_MAX_COUNT = 12;

// the sum of c over the 64 lanes of the wave, in every lane
__device__ __forceinline__ unsigned compact_wave_sum(unsigned c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    return c;
}

// the sum of c over the lanes below the calling one
__device__ __forceinline__ unsigned compact_wave_exclusive(unsigned c) {
    const int lane = threadIdx.x & 63;
    unsigned inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    return inc - c;
}

// The count step for a kernel that classifies its elements itself: c[k] is the count of element chunk * CP_CHUNK + lane + 64 k (0 past
// n), and lane 0 stores the chunk's sum.  Every lane of the wave must call it.
__device__ __forceinline__ void compact_store_chunk_sum(const unsigned (&c)[CP_SUB], long long n, unsigned* __restrict__ counts) {
    const long long chunk = compact_wave_chunk();
    const unsigned sum = compact_wave_sum(c[0] + c[1] + c[2] + c[3]);
    if ((threadIdx.x & 63) == 0 && chunk * CP_CHUNK < n) counts[chunk] = sum;
}

// The scan for many chunks.  compact_scan_kernel gives every lane of its one workgroup nchunks / 256 counts in two serial loops: 14
// at 768 x 1152, 2048 for a 512^3 volume.  compact_scan_blocks is the same scan in two levels: one workgroup sums each block of
// CP_BLOCK chunks, compact_scan_kernel scans the block sums (32 per lane at 2^31 elements), one workgroup scans each block on top of
// its offset.  Integer sums: the offsets and the total are compact_scan_kernel's.  block: compact_block_bytes(n) of workspace.
constexpr int CP_BLOCK = 4 * CP_THREADS;  // chunks per block, four per lane

static inline long long compact_blocks(long long n) { return (compact_chunks(n) + CP_BLOCK - 1) / CP_BLOCK; }
static inline size_t compact_block_bytes(long long n) { return align_up((size_t)compact_blocks(n) * sizeof(unsigned), 256); }

// APPLY false: block[b] = the sum of block b's counts.  APPLY true: block[b] holds the block's offset, and the counts become offsets.
template <bool APPLY>
__global__ void __launch_bounds__(CP_THREADS) compact_block_kernel(unsigned* __restrict__ counts, long long nchunks,
                                                                   unsigned* __restrict__ block) {
    __shared__ unsigned part[CP_THREADS];
    const int t = threadIdx.x;
    const long long first = (long long)blockIdx.x * CP_BLOCK + 4 * t;
    unsigned c[4], acc = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c[k] = first + k < nchunks ? counts[first + k] : 0u;
        acc += c[k];
    }
    part[t] = acc;
    __syncthreads();
    for (int s = 1; s < CP_THREADS; s <<= 1) {  // inclusive scan of the 256 lane sums
        const unsigned add = t >= s ? part[t - s] : 0u;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    if (!APPLY) {
        if (t == CP_THREADS - 1) block[blockIdx.x] = part[t];
        return;
    }
    unsigned run = block[blockIdx.x] + part[t] - acc;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (first + k < nchunks) counts[first + k] = run;
        run += c[k];
    }
}

static inline void compact_scan_blocks(unsigned* counts, long long n, unsigned* block, long long* total, hipStream_t st) {
    const long long nchunks = compact_chunks(n);
    const unsigned nblocks = (unsigned)compact_blocks(n);
    hipLaunchKernelGGL(compact_block_kernel<false>, dim3(nblocks), dim3(CP_THREADS), 0, st, counts, nchunks, block);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(CP_THREADS), 0, st, block, (long long)nblocks, total);
    hipLaunchKernelGGL(compact_block_kernel<true>, dim3(nblocks), dim3(CP_THREADS), 0, st, counts, nchunks, block);
}

// The walk: every element p with count c > 0 gets emit(p, slot, c), slot the first of its c slots.  Every lane of the wave must call it.
template <class Count, class Emit>
__device__ __forceinline__ void compact_walk_counted(const Count& count, const unsigned* __restrict__ offsets, long long n,
                                                     const Emit& emit) {
    const int lane = threadIdx.x & 63;
    const long long chunk = compact_wave_chunk();
    if (chunk * CP_CHUNK >= n) return;  // the whole wave
    const long long base = chunk * CP_CHUNK + lane;
    long long run = offsets[chunk];
    unsigned c[CP_SUB];
#pragma unroll
    for (int k = 0; k < CP_SUB; ++k) c[k] = base + 64 * k < n ? count(base + 64 * k) : 0u;
#pragma unroll
    for (int k = 0; k < CP_SUB; ++k) {
        const unsigned below = compact_wave_exclusive(c[k]);
        if (c[k]) emit(base + 64 * k, run + below, c[k]);
        run += __shfl(below + c[k], 63);
    }
}

}  // namespace mvd
