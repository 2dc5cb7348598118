// Mesh clean-up (mesh_clean.py is the definition): connected components of a triangle list, the component table, the filter that
// drops components and the vertices they leave behind, and area-weighted vertex normals.
//   mvd_mesh_hook_round          one round of min-label hooking with pointer jumping: a launch over the triangles, one over the vertices
//   mvd_mesh_component_rank      the roots ranked in ascending vertex order (compact.h), every vertex's component or -1
//   mvd_mesh_component_table     every triangle's component, every component's number of vertices
//   mvd_mesh_component_sums_f64  from the triangles sorted by component: every component's number of triangles and its area, float64
//   mvd_mesh_filter              the kept triangles and vertices compacted in their order (compact.h), re-indexed, with the remaps
//   mvd_mesh_gather_rows_f32     the rows of a per-vertex array moved through the remap, bit for bit
//   mvd_mesh_vertex_normals_f32  from the corners sorted by vertex: one lane walks one vertex's run
// What bounds each kernel: every one is a straight pass with a trip count fixed by its arguments.  None waits for another thread: no
// spin loop, no compare-and-swap retry, no lock, no grid synchronisation.  The rounds of the labelling are driven by the host, which
// reads one word per round and stops at a hard cap.  The only atomics are 32-bit integer atomicMin / atomicAdd on global memory, whose
// results do not depend on the order of arrival; no float atomic anywhere, every float64 sum has a fixed order: two runs give the same bits.
//
// Labelling.  label[v] starts at v.  A round is
//   hook      per triangle (a,b,c): m = min(label[label[a]], label[label[b]], label[label[c]]); atomicMin m into label[label[x]] and
//             into label[x] for x = a, b, c   (the parent hook and the vertex hook of FastSV, with the triangle as a 3-clique)
//   shortcut  per vertex: label[v] = label[label[v]]
// Why every value a thread can read is a vertex of the same component, and why labels only decrease.  Invariant: label[y] is a vertex
// of y's component and label[y] <= y.  It holds at the start.  The hook stores m, a label of a label of a vertex of the triangle, so
// by the invariant a vertex of that component, into label[x] for x a vertex of the triangle or its label, so again of that component;
// it stores with atomicMin, so the word only decreases and stays <= x.  The shortcut is the only writer of label[v] in its launch and
// stores label[label[v]] <= label[v] (the invariant at label[v]), of the same component.  A load that races with a store returns
// the word before or after it (aligned 32-bit words), and a load served by a cache that has not seen the store returns an earlier
// value of the word: each of them was stored under the invariant, so it is a vertex of the component, in 0 .. M-1, and at least the
// present value.  A stale value can therefore only make a thread hook with a larger m than the best one, never a wrong one, and the
// launch boundary makes every store visible to the next launch.
// Fixed point.  A round in which no atomicMin lowered a word and no shortcut changed one read a state that nobody wrote, so all its
// loads were exact: label[label[x]] is equal over each triangle, and label[v] = label[label[v]].  Then label is constant over a component,
// the constant L is a vertex of it with label[L] = L, and label[v] <= v makes L its lowest vertex.  That state is unique: whatever
// order the hooks land in, the result is the same bits.
#include "compact.h"
#include "fixed_sums.h"

namespace mvd {

constexpr int MC_THREADS = 256;

__device__ __forceinline__ int label_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// lowers *p to m -> whether the word was above m.  The load first: a word at or below m already (most of them, in the last rounds)
// costs no atomic; the loaded value is at least the present one, so no lowering is missed.
__device__ __forceinline__ bool label_lower(int* p, int m) { return label_load(p) > m && atomicMin(p, m) > m; }

__global__ void __launch_bounds__(MC_THREADS) mesh_init_kernel(int* __restrict__ label, unsigned char* __restrict__ referenced, int M) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= M) return;
    label[v] = (int)v;
    referenced[v] = 0;
}

__global__ void __launch_bounds__(MC_THREADS) mesh_hook_kernel(const int* __restrict__ tri, int T, int M, int* label,
                                                               unsigned char* __restrict__ referenced, int mark, int* __restrict__ changed) {
    const long long t = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (t >= T) return;
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    if ((unsigned)a >= (unsigned)M || (unsigned)b >= (unsigned)M || (unsigned)c >= (unsigned)M) return;  // the caller refuses these
    if (mark) referenced[a] = referenced[b] = referenced[c] = 1;  // plain byte stores; every lane stores the same 1
    const int fa = label_load(label + a), fb = label_load(label + b), fc = label_load(label + c);  // in 0 .. M-1: the invariant
    if ((unsigned)fa >= (unsigned)M || (unsigned)fb >= (unsigned)M || (unsigned)fc >= (unsigned)M) return;  // a label array nobody started
    const int m = min(min(label_load(label + fa), label_load(label + fb)), label_load(label + fc));
    bool ch = label_lower(label + fa, m);
    ch |= label_lower(label + fb, m);
    ch |= label_lower(label + fc, m);
    ch |= label_lower(label + a, m);
    ch |= label_lower(label + b, m);
    ch |= label_lower(label + c, m);
    if (ch) changed[0] = 1;  // a plain vector store of 1, the same from every lane
}

__global__ void __launch_bounds__(MC_THREADS) mesh_shortcut_kernel(int* label, int M, int* __restrict__ changed) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= M) return;
    const int p = label_load(label + v);
    if ((unsigned)p >= (unsigned)M) return;  // a label array nobody started
    const int g = label_load(label + p);
    if (g < p) {
        label[v] = g;  // this lane is the only writer of label[v] in this launch
        changed[0] = 1;
    }
}

// ---- ranking ---------------------------------------------------------------------------------------------------------------------------
struct MeshRoot {
    const int* label;
    const unsigned char* referenced;
    __device__ bool operator()(long long v) const { return referenced[v] != 0 && label[v] == (int)v; }
};

__global__ void __launch_bounds__(CP_THREADS) mesh_rank_roots_kernel(const int* __restrict__ label, const unsigned char* __restrict__ referenced,
                                                                     int M, const unsigned* __restrict__ offsets, int* __restrict__ rank) {
    compact_walk(MeshRoot{label, referenced}, offsets, M, [&](long long v, long long slot) { rank[v] = (int)slot; });
}

__global__ void __launch_bounds__(MC_THREADS) mesh_vertex_component_kernel(const int* __restrict__ label,
                                                                           const unsigned char* __restrict__ referenced, int M,
                                                                           const int* __restrict__ rank, int* __restrict__ vcomp) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= M) return;
    int c = -1;
    if (referenced[v]) {
        const int r = label[v];
        if ((unsigned)r < (unsigned)M && referenced[r] && label[r] == r) c = rank[r];  // a converged labelling: always
    }
    vcomp[v] = c;
}

// ---- table -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MC_THREADS) mesh_triangle_component_kernel(const int* __restrict__ tri, int T, int M,
                                                                             const int* __restrict__ vcomp, int* __restrict__ tcomp) {
    const long long t = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (t >= T) return;
    const int a = tri[3 * t];
    tcomp[t] = (unsigned)a < (unsigned)M ? vcomp[a] : -1;
}

// counts[c] += the vertices of component c.  A wave takes VC_PER chunks of 64 consecutive vertices.  In a chunk the lanes of equal
// component count once, through a ballot (at most 64 passes per chunk, one per distinct component; neighbouring vertices of a mesh
// mostly share theirs: one or two), and the wave carries the running component's count from chunk to chunk in a wave-uniform pair,
// adding it with one integer atomic when the component changes and at the end: one large component costs one atomic per 1024
// vertices on its address instead of one per 64 (the table of the 4.8 M-triangle mesh: 0.46 -> 0.27 ms, of the strip 0.41 -> 0.07 ms).
constexpr int VC_PER = 16;

__global__ void __launch_bounds__(MC_THREADS) mesh_vertex_count_kernel(const int* __restrict__ vcomp, int M, int C, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const long long base = ((long long)blockIdx.x * (MC_THREADS / 64) + (threadIdx.x >> 6)) * 64 * VC_PER;
    int cur = -1, cur_n = 0;  // wave-uniform
    for (int k = 0; k < VC_PER; ++k) {
        const long long v = base + 64 * k + lane;
        const int c = v < M ? vcomp[v] : -1;
        const bool have = (unsigned)c < (unsigned)C;
        unsigned long long todo = __ballot(have);
        while (todo != 0ull) {  // wave-uniform; every pass clears at least the leader's bit
            const int lc = __shfl(c, __ffsll((long long)todo) - 1);
            const unsigned long long same = __ballot(have && c == lc) & todo;
            if (lc != cur) {
                if (cur_n > 0 && lane == 0) atomicAdd(counts + cur, cur_n);
                cur = lc;
                cur_n = 0;
            }
            cur_n += __popcll(same);
            todo &= ~same;
        }
    }
    if (cur_n > 0 && lane == 0) atomicAdd(counts + cur, cur_n);
}

// ---- areas -----------------------------------------------------------------------------------------------------------------------------
// The cross product of a triangle's two edge vectors from vertex 0, float64 from the float32 coordinates:
// e1 = p1 - p0, e2 = p2 - p0, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), one rounding per operation.
struct Cross {
    double x, y, z;
};

__device__ __forceinline__ Cross triangle_cross(const float* __restrict__ vtx, int a, int b, int c) {
    const double ax = vtx[3 * (long long)a], ay = vtx[3 * (long long)a + 1], az = vtx[3 * (long long)a + 2];
    const double e1x = (double)vtx[3 * (long long)b] - ax, e1y = (double)vtx[3 * (long long)b + 1] - ay, e1z = (double)vtx[3 * (long long)b + 2] - az;
    const double e2x = (double)vtx[3 * (long long)c] - ax, e2y = (double)vtx[3 * (long long)c + 1] - ay, e2z = (double)vtx[3 * (long long)c + 2] - az;
    return Cross{e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x};
}

__device__ __forceinline__ double cross_length(const Cross& n) { return sqrt((n.x * n.x + n.y * n.y) + n.z * n.z); }
__device__ __forceinline__ bool finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for inf and NaN

// Sorted position p holds triangle perm[p] of component key[p].  One workgroup takes MA_BLOCK consecutive positions: it stores each
// one's area and, for a block that lies inside one component, the block's sum (thread i adds positions i, i + 256, ... in order, then
// fixed_sums.h's sum over the workgroup).  seg[c] = the first position of component c, seg[C] = the number of positions
// with a component; the keys ascend and every component has a triangle, so every entry is written.
constexpr int MA_PER = 8;
constexpr int MA_BLOCK = MC_THREADS * MA_PER;  // 2048
static_assert(MC_THREADS == FS_THREADS, "the area and sum kernels are launched as fixed_sums.h expects");

__global__ void __launch_bounds__(MC_THREADS) mesh_area_kernel(const float* __restrict__ vtx, const int* __restrict__ tri, int T, int M,
                                                               const int* __restrict__ key, const long long* __restrict__ perm, int C,
                                                               double* __restrict__ area, double* __restrict__ block_sum, int* __restrict__ seg) {
    const long long base = (long long)blockIdx.x * MA_BLOCK;
    FixedRecord<1, 1ull> acc{};  // one double
#pragma unroll
    for (int k = 0; k < MA_PER; ++k) {
        const long long p = base + k * MC_THREADS + threadIdx.x;
        if (p >= T) continue;
        const long long t = perm[p];
        double a = 0.0;
        if ((unsigned long long)t < (unsigned long long)T) {
            const int i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
            if ((unsigned)i0 < (unsigned)M && (unsigned)i1 < (unsigned)M && (unsigned)i2 < (unsigned)M) {
                a = 0.5 * cross_length(triangle_cross(vtx, i0, i1, i2));
                if (!finite_f64(a)) a = 0.0;
            }
        }
        area[p] = a;
        acc.addf(0, a);
        const int c = key[p], before = p > 0 ? key[p - 1] : -1;
        if ((unsigned)c < (unsigned)C && c != before) seg[c] = (int)p;
        if (p + 1 == T) seg[C] = T;
    }
    fixed_reduce_store(acc, block_sum + blockIdx.x);
}

// fixed_sums.h's segment walk over `area`, one segment per component.  A segment of more than 64 positions that holds whole blocks is
// added through their stored sums: lane l adds items l, l + 64, ... of the segment's head up to the first block boundary, of its whole
// blocks' sums and of its tail, each from zero, and then head + blocks + tail.  The order is fixed by b and e alone.
__device__ __forceinline__ double area_span(const double* __restrict__ a, long long b, long long e, int lane) {
    double s = 0.0;
    for (long long p = b + lane; p < e; p += 64) s += a[p];
    return s;
}

__global__ void __launch_bounds__(MC_THREADS) mesh_component_sum_kernel(const int* __restrict__ seg, int C, int T,
                                                                        const double* __restrict__ area, const double* __restrict__ block_sum,
                                                                        int* __restrict__ num_triangles, double* __restrict__ out) {
    const auto add = [&](FixedSums<1>& s, long long p) { s.v[0] += area[p]; };
    const auto span = [&](FixedSums<1>& s, long long b, long long e, int lane) {
        const long long first = (b + MA_BLOCK - 1) / MA_BLOCK, last = e / MA_BLOCK;  // whole blocks [first, last)
        if (first >= last) {
            s.v[0] = area_span(area, b, e, lane);
        } else {
            s.v[0] = area_span(area, b, first * MA_BLOCK, lane);
            s.v[0] += area_span(block_sum, first, last, lane);
            s.v[0] += area_span(area, last * MA_BLOCK, e, lane);
        }
    };
    fixed_segment_walk<1>(seg, C, T, add, span, [&](const FixedSums<1>& s, int len, long long c) {
        num_triangles[c] = len;
        out[c] = s.v[0];
    });
}

// ---- filter ----------------------------------------------------------------------------------------------------------------------------
struct KeptTriangle {
    const int* tcomp;
    const unsigned char* keep;  // NULL: every component stays
    int C;
    __device__ bool operator()(long long t) const {
        if (!keep) return true;
        const int c = tcomp[t];
        return (unsigned)c < (unsigned)C && keep[c] != 0;
    }
};

struct KeptVertex {
    const unsigned char* used;  // NULL: every vertex stays
    __device__ bool operator()(long long v) const { return !used || used[v] != 0; }
};

__global__ void __launch_bounds__(MC_THREADS) mesh_mark_used_kernel(const int* __restrict__ tri, int T, int M, KeptTriangle kept,
                                                                    unsigned char* __restrict__ used) {
    const long long t = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (t >= T || !kept(t)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = tri[3 * t + k];
        if ((unsigned)i < (unsigned)M) used[i] = 1;  // plain byte stores; every lane stores the same 1
    }
}

__global__ void __launch_bounds__(MC_THREADS) mesh_store_counts_kernel(const long long* __restrict__ totals, long long* __restrict__ counts) {
    if (threadIdx.x < 2 && blockIdx.x == 0) counts[threadIdx.x] = totals[threadIdx.x];
}

__global__ void __launch_bounds__(CP_THREADS) mesh_vertex_remap_kernel(KeptVertex kept, int M, const unsigned* __restrict__ offsets,
                                                                       int* __restrict__ remap) {
    const long long base = compact_wave_chunk() * CP_CHUNK + (threadIdx.x & 63);
#pragma unroll
    for (int k = 0; k < CP_SUB; ++k) {
        const long long v = base + 64 * k;
        if (v < M && !kept(v)) remap[v] = -1;
    }
    compact_walk(kept, offsets, M, [&](long long v, long long slot) { remap[v] = (int)slot; });
}

__global__ void __launch_bounds__(CP_THREADS) mesh_triangle_write_kernel(KeptTriangle kept, const int* __restrict__ tri, int T, int M,
                                                                         const unsigned* __restrict__ offsets, const int* __restrict__ remap,
                                                                         long long max_triangles, int* __restrict__ out_tri,
                                                                         int* __restrict__ kept_index) {
    compact_walk(kept, offsets, T, [&](long long t, long long slot) {
        if (slot >= max_triangles) return;
        kept_index[slot] = (int)t;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = tri[3 * t + k];
            out_tri[3 * slot + k] = (unsigned)i < (unsigned)M ? remap[i] : -1;
        }
    });
}

__global__ void __launch_bounds__(MC_THREADS) mesh_gather_rows_kernel(const float* __restrict__ src, const int* __restrict__ remap, int M,
                                                                      int k, long long max_rows, float* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;  // one lane per float
    if (i >= (long long)M * k) return;
    const long long v = i / k;
    const int r = remap[v];
    if (r >= 0 && r < max_rows) dst[(long long)r * k + (i - v * k)] = src[i];
}

// ---- vertex normals ------------------------------------------------------------------------------------------------------------------
// Sorted position p holds corner perm[p] = 3 t + k of vertex key[p].  One lane per vertex: a binary search for the start of its run
// (at most 32 steps), then the run in order, 6 to 8 corners on these meshes.
__global__ void __launch_bounds__(MC_THREADS) mesh_vertex_normals_kernel(const float* __restrict__ vtx, int M, const int* __restrict__ tri,
                                                                         int T, const int* __restrict__ key,
                                                                         const long long* __restrict__ perm, float* __restrict__ normals) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= M) return;
    const long long n = 3ll * T;
    long long lo = 0, hi = n;  // the first position with key >= v
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (key[mid] < (int)v) lo = mid + 1; else hi = mid;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (long long p = lo; p < n && key[p] == (int)v; ++p) {
        const long long t = perm[p] / 3;
        if ((unsigned long long)perm[p] >= (unsigned long long)n) continue;
        const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        if ((unsigned)a >= (unsigned)M || (unsigned)b >= (unsigned)M || (unsigned)c >= (unsigned)M) continue;
        const Cross x = triangle_cross(vtx, a, b, c);
        sx += x.x;
        sy += x.y;
        sz += x.z;
    }
    const double len = cross_length(Cross{sx, sy, sz});
    const bool good = len > 0.0 && finite_f64(len);
    normals[3 * v] = good ? (float)(sx / len) : 0.f;
    normals[3 * v + 1] = good ? (float)(sy / len) : 0.f;
    normals[3 * v + 2] = good ? (float)(sz / len) : 0.f;
}

static inline unsigned mc_blocks(long long n) { return (unsigned)((n + MC_THREADS - 1) / MC_THREADS); }

}  // namespace mvd

extern "C" int mvd_mesh_hook_round(const int* triangles, long long T, long long M, int flags, int* label, unsigned char* referenced,
                                   int* changed, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_hook_round", "triangles", T);
    MVD_REQUIRE_COUNT("mesh_hook_round", "vertices", M);
    MVD_REQUIRE(changed && ((uintptr_t)changed & 3) == 0, "mesh_hook_round: changed must be given and 4-byte aligned");
    MVD_REQUIRE(M == 0 || (label && referenced), "mesh_hook_round: NULL argument");
    MVD_REQUIRE(((uintptr_t)label & 3) == 0, "mesh_hook_round: label must be 4-byte aligned");
    MVD_REQUIRE(T == 0 || (triangles && M > 0), "mesh_hook_round: triangles without vertices");
    MVD_REQUIRE((flags & ~(MVD_MESH_ROUND_FIRST | MVD_MESH_ROUND_NO_HOOK | MVD_MESH_ROUND_NO_SHORTCUT)) == 0, "mesh_hook_round: flags %d", flags);
    hipStream_t st = (hipStream_t)stream;
    const bool first = flags & MVD_MESH_ROUND_FIRST, hook = !(flags & MVD_MESH_ROUND_NO_HOOK), jump = !(flags & MVD_MESH_ROUND_NO_SHORTCUT);
    if (hook && hipMemsetAsync(changed, 0, sizeof(int), st) != hipSuccess) return launch_status("mesh_hook_round");
    if (M == 0) return MVD_OK;
    if (first) hipLaunchKernelGGL(mesh_init_kernel, dim3(mc_blocks(M)), dim3(MC_THREADS), 0, st, label, referenced, (int)M);
    if (T > 0 && hook)
        hipLaunchKernelGGL(mesh_hook_kernel, dim3(mc_blocks(T)), dim3(MC_THREADS), 0, st, triangles, (int)T, (int)M, label, referenced,
                           first ? 1 : 0, changed);
    if (T > 0 && jump) hipLaunchKernelGGL(mesh_shortcut_kernel, dim3(mc_blocks(M)), dim3(MC_THREADS), 0, st, label, (int)M, changed);
    return launch_status("mesh_hook_round");
}

extern "C" size_t mvd_mesh_component_rank_workspace_bytes(long long M) {
    if (M <= 0) return 0;
    return mvd::compact_offsets_bytes(M) + mvd::compact_block_bytes(M) + mvd::align_up((size_t)M * sizeof(int), 256);
}

extern "C" int mvd_mesh_component_rank(const int* label, const unsigned char* referenced, long long M, int* vertex_component,
                                       long long* num_components, void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_component_rank", "vertices", M);
    MVD_REQUIRE(num_components && ((uintptr_t)num_components & 7) == 0, "mesh_component_rank: num_components must be given and 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (M == 0) {
        if (hipMemsetAsync(num_components, 0, sizeof(long long), st) != hipSuccess) return launch_status("mesh_component_rank");
        return MVD_OK;
    }
    MVD_REQUIRE(label && referenced && vertex_component, "mesh_component_rank: NULL argument");
    MVD_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= mvd_mesh_component_rank_workspace_bytes(M),
                "mesh_component_rank: workspace too small or not 256-byte aligned");
    unsigned char* w = static_cast<unsigned char*>(workspace);
    unsigned* chunk = reinterpret_cast<unsigned*>(w);
    unsigned* block = reinterpret_cast<unsigned*>(w + compact_offsets_bytes(M));
    int* rank = reinterpret_cast<int*>(w + compact_offsets_bytes(M) + compact_block_bytes(M));
    const MeshRoot root{label, referenced};
    hipLaunchKernelGGL(compact_count_kernel<MeshRoot>, dim3(compact_workgroups(M)), dim3(CP_THREADS), 0, st, root, M, chunk);
    compact_scan_blocks(chunk, M, block, num_components, st);
    hipLaunchKernelGGL(mesh_rank_roots_kernel, dim3(compact_workgroups(M)), dim3(CP_THREADS), 0, st, label, referenced, (int)M, chunk, rank);
    hipLaunchKernelGGL(mesh_vertex_component_kernel, dim3(mc_blocks(M)), dim3(MC_THREADS), 0, st, label, referenced, (int)M, rank,
                       vertex_component);
    return launch_status("mesh_component_rank");
}

extern "C" int mvd_mesh_component_table(const int* vertex_component, const int* triangles, long long T, long long M, long long C,
                                        int* triangle_component, int* num_vertices, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_component_table", "triangles", T);
    MVD_REQUIRE_COUNT("mesh_component_table", "vertices", M);
    MVD_REQUIRE(C >= 0 && C <= M, "mesh_component_table: %lld components of %lld vertices", C, M);
    MVD_REQUIRE(M == 0 || vertex_component, "mesh_component_table: NULL argument");
    MVD_REQUIRE(T == 0 || (triangles && triangle_component && M > 0), "mesh_component_table: NULL argument");
    MVD_REQUIRE(C == 0 || num_vertices, "mesh_component_table: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (T > 0)
        hipLaunchKernelGGL(mesh_triangle_component_kernel, dim3(mc_blocks(T)), dim3(MC_THREADS), 0, st, triangles, (int)T, (int)M,
                           vertex_component, triangle_component);
    if (C > 0) {
        if (hipMemsetAsync(num_vertices, 0, (size_t)C * sizeof(int), st) != hipSuccess) return launch_status("mesh_component_table");
        hipLaunchKernelGGL(mesh_vertex_count_kernel, dim3(mc_blocks((M + VC_PER - 1) / VC_PER)), dim3(MC_THREADS), 0, st, vertex_component,
                           (int)M, (int)C, num_vertices);
    }
    return launch_status("mesh_component_table");
}

static size_t mesh_sums_area_bytes(long long T) { return mvd::align_up((size_t)T * sizeof(double), 256); }
static size_t mesh_sums_block_bytes(long long T) {
    return mvd::align_up((size_t)((T + mvd::MA_BLOCK - 1) / mvd::MA_BLOCK) * sizeof(double), 256);
}

extern "C" size_t mvd_mesh_component_sums_workspace_bytes(long long T, long long C) {
    if (T <= 0 || C <= 0) return 0;
    return mesh_sums_area_bytes(T) + mesh_sums_block_bytes(T) + mvd::align_up((size_t)(C + 1) * sizeof(int), 256);
}

extern "C" int mvd_mesh_component_sums_f64(const float* vertices, long long M, const int* triangles, long long T, const int* sorted_component,
                                           const long long* perm, long long C, int* num_triangles, double* area, void* workspace,
                                           size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_component_sums", "triangles", T);
    MVD_REQUIRE_COUNT("mesh_component_sums", "vertices", M);
    MVD_REQUIRE(C >= 0 && C <= T, "mesh_component_sums: %lld components of %lld triangles", C, T);
    if (C == 0) return MVD_OK;
    MVD_REQUIRE(vertices && triangles && sorted_component && perm && num_triangles && area, "mesh_component_sums: NULL argument");
    MVD_REQUIRE(((uintptr_t)area & 7) == 0, "mesh_component_sums: area must be 8-byte aligned");
    MVD_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= mvd_mesh_component_sums_workspace_bytes(T, C),
                "mesh_component_sums: workspace too small or not 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = static_cast<unsigned char*>(workspace);
    double* tri_area = reinterpret_cast<double*>(w);
    double* block_sum = reinterpret_cast<double*>(w + mesh_sums_area_bytes(T));
    int* seg = reinterpret_cast<int*>(w + mesh_sums_area_bytes(T) + mesh_sums_block_bytes(T));
    // a key sequence that skips a component (not a sorted labelling) leaves its entry at 0; the sum kernel clamps every segment into 0 .. T
    if (hipMemsetAsync(seg, 0, (size_t)(C + 1) * sizeof(int), st) != hipSuccess) return launch_status("mesh_component_sums");
    hipLaunchKernelGGL(mesh_area_kernel, dim3((unsigned)((T + MA_BLOCK - 1) / MA_BLOCK)), dim3(MC_THREADS), 0, st, vertices, triangles, (int)T,
                       (int)M, sorted_component, perm, (int)C, tri_area, block_sum, seg);
    hipLaunchKernelGGL(mesh_component_sum_kernel, dim3(mc_blocks(C)), dim3(MC_THREADS), 0, st, seg, (int)C, (int)T, tri_area, block_sum,
                       num_triangles, area);
    return launch_status("mesh_component_sums");
}

// workspace: [triangle chunk offsets | vertex chunk offsets | block sums (the larger of the two) | used (M bytes) | totals (2 int64)]
namespace {
struct FilterLayout {
    size_t tri, vtx, block, used, totals, bytes;
};
FilterLayout filter_layout(long long M, long long T) {
    FilterLayout l;
    l.tri = 0;
    l.vtx = l.tri + mvd::compact_offsets_bytes(T);
    l.block = l.vtx + mvd::compact_offsets_bytes(M);
    l.used = l.block + mvd::compact_block_bytes(M > T ? M : T);
    l.totals = l.used + mvd::align_up((size_t)M, 256);
    l.bytes = l.totals + 256;
    return l;
}
}  // namespace

extern "C" size_t mvd_mesh_filter_workspace_bytes(long long M, long long T) {
    if (M < 0 || T < 0) return 0;
    return filter_layout(M, T).bytes;
}

extern "C" int mvd_mesh_filter(const int* triangles, long long T, long long M, const int* triangle_component,
                               const unsigned char* keep_component, long long C, int remove_unreferenced, int counted, int* out_triangles,
                               int* kept_triangles, int* vertex_remap, long long max_triangles, long long* counts, void* workspace,
                               size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_filter", "triangles", T);
    MVD_REQUIRE_COUNT("mesh_filter", "vertices", M);
    MVD_REQUIRE(counts && ((uintptr_t)counts & 15) == 0, "mesh_filter: counts must be given and 16-byte aligned");
    MVD_REQUIRE(!keep_component || (C >= 0 && C <= 0x7fffffffLL && (T == 0 || triangle_component)),
                "mesh_filter: keep_component needs triangle_component and 0 <= C < 2^31");
    MVD_REQUIRE(T == 0 || (triangles && M > 0), "mesh_filter: triangles without vertices");
    MVD_REQUIRE(!out_triangles == !kept_triangles && !out_triangles == !vertex_remap,
                "mesh_filter: out_triangles, kept_triangles and vertex_remap go together");
    MVD_REQUIRE(max_triangles >= 0 && max_triangles <= 0x7fffffffLL, "mesh_filter: max_triangles must be in 0 .. 2^31 - 1");
    MVD_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= mvd_mesh_filter_workspace_bytes(M, T),
                "mesh_filter: workspace too small or not 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const FilterLayout l = filter_layout(M, T);
    unsigned char* w = static_cast<unsigned char*>(workspace);
    unsigned* tri_off = reinterpret_cast<unsigned*>(w + l.tri);
    unsigned* vtx_off = reinterpret_cast<unsigned*>(w + l.vtx);
    unsigned* block = reinterpret_cast<unsigned*>(w + l.block);
    unsigned char* used = remove_unreferenced ? w + l.used : nullptr;
    long long* totals = reinterpret_cast<long long*>(w + l.totals);  // kept vertices, kept triangles
    const KeptTriangle kt{triangle_component, keep_component, (int)C};
    const KeptVertex kv{used};
    if (!counted) {
        if (hipMemsetAsync(totals, 0, 2 * sizeof(long long), st) != hipSuccess) return launch_status("mesh_filter");
        if (used && M > 0 && hipMemsetAsync(used, 0, (size_t)M, st) != hipSuccess) return launch_status("mesh_filter");
        if (T > 0) {
            hipLaunchKernelGGL(compact_count_kernel<KeptTriangle>, dim3(compact_workgroups(T)), dim3(CP_THREADS), 0, st, kt, T, tri_off);
            compact_scan_blocks(tri_off, T, block, totals + 1, st);
            if (used) hipLaunchKernelGGL(mesh_mark_used_kernel, dim3(mc_blocks(T)), dim3(MC_THREADS), 0, st, triangles, (int)T, (int)M, kt, used);
        }
        if (M > 0) {
            hipLaunchKernelGGL(compact_count_kernel<KeptVertex>, dim3(compact_workgroups(M)), dim3(CP_THREADS), 0, st, kv, M, vtx_off);
            compact_scan_blocks(vtx_off, M, block, totals, st);
        }
    }
    hipLaunchKernelGGL(mesh_store_counts_kernel, dim3(1), dim3(MC_THREADS), 0, st, totals, counts);
    if (out_triangles) {
        if (M > 0)
            hipLaunchKernelGGL(mesh_vertex_remap_kernel, dim3(compact_workgroups(M)), dim3(CP_THREADS), 0, st, kv, (int)M, vtx_off, vertex_remap);
        if (T > 0)
            hipLaunchKernelGGL(mesh_triangle_write_kernel, dim3(compact_workgroups(T)), dim3(CP_THREADS), 0, st, kt, triangles, (int)T, (int)M,
                               tri_off, vertex_remap, max_triangles, out_triangles, kept_triangles);
    }
    return launch_status("mesh_filter");
}

extern "C" int mvd_mesh_gather_rows_f32(const float* src, const int* vertex_remap, long long M, int k, long long max_rows, float* dst,
                                        mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_gather_rows", "vertices", M);
    MVD_REQUIRE(k >= 1 && k <= 65536, "mesh_gather_rows: %d columns, supported 1 .. 65536", k);
    MVD_REQUIRE(max_rows >= 0 && max_rows <= M, "mesh_gather_rows: %lld rows out of %lld", max_rows, M);
    MVD_REQUIRE(M * k <= 0x7fffffffLL, "mesh_gather_rows: M k = %lld values, supported up to 2^31 - 1 (one lane each)", M * k);
    if (M == 0 || max_rows == 0) return MVD_OK;
    MVD_REQUIRE(src && vertex_remap && dst, "mesh_gather_rows: NULL argument");
    hipLaunchKernelGGL(mesh_gather_rows_kernel, dim3(mc_blocks(M * k)), dim3(MC_THREADS), 0, (hipStream_t)stream, src, vertex_remap, (int)M, k,
                       max_rows, dst);
    return launch_status("mesh_gather_rows");
}

extern "C" int mvd_mesh_vertex_normals_f32(const float* vertices, long long M, const int* triangles, long long T, const int* sorted_vertex,
                                           const long long* perm, float* normals, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE_COUNT("mesh_vertex_normals", "vertices", M);
    MVD_REQUIRE(T >= 0 && 3 * T <= 0x7fffffffLL, "mesh_vertex_normals: %lld triangles, 3 T must be below 2^31", T);
    if (M == 0) return MVD_OK;
    MVD_REQUIRE(vertices && normals, "mesh_vertex_normals: NULL argument");
    MVD_REQUIRE(T == 0 || (triangles && sorted_vertex && perm), "mesh_vertex_normals: NULL argument");
    hipLaunchKernelGGL(mesh_vertex_normals_kernel, dim3(mc_blocks(M)), dim3(MC_THREADS), 0, (hipStream_t)stream, vertices, (int)M, triangles,
                       (int)T, sorted_vertex, perm, normals);
    return launch_status("mesh_vertex_normals");
}
