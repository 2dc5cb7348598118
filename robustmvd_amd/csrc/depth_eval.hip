// Device-side scoring of the multi-view depth evaluation (rmvd/eval/multi_view_depth_evaluation.py:469-547,583-610 and
// rmvd/eval/metrics.py:32-220): the prediction (h,w) is scored against the ground truth (H,W) where the model left it.
//   mvd_depth_align_stats_f32   the alignment parameters (ratio of medians by an exact radix select, or the least-squares scale and
//                               shift in inverse depth from float64 sums) and the minimum of the resized uncertainty
//   mvd_depth_score_f32         alignment, clipping, inverse depth, relative error and inlier test of one run in one pass
//   mvd_rank_keys_f32           the sparsification's ranking key ((u - u_min) + 1) * mask
//   mvd_ranked_step_sums_f64    the sums of the ranked errors from each of the 100 sparsification steps to the end
// The nearest resize of the prediction to (H,W) is a gather through two index tables, row[H] and col[W], in every kernel that reads
// the prediction; the resized map is only written where the caller asks for it.
// Every float reduction across workgroups is a buffer of per-workgroup partials summed in a fixed order by one workgroup, so two calls
// give the same bits.  Counts, histograms and minima (on order-preserving integer keys) use integer atomics, whose result does not
// depend on the order.  Every float32 step is one rounding, in the reference's order (the library is built without contraction).
#include "mvd_common.h"

namespace mvd {

constexpr int EV_THREADS = 256;
constexpr int EV_PIX = 2048;  // pixels per workgroup: 8 per lane; 768 x 1152 is 432 workgroups
constexpr int EV_STEPS = 100;

// float -> uint32 whose unsigned order is the float order (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN)
__device__ __forceinline__ unsigned order_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_key_inv(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// np.nan_to_num(v, nan=r, posinf=r, neginf=r)
__device__ __forceinline__ float finite_or(float v, float r) { return finite_f32(v) ? v : r; }

// The four selections of the median alignment: sel = 2 * array + which, array 0 = gt, 1 = prediction; which 0 = the lower middle
// element (rank (n - 1) / 2), 1 = the upper one (rank n / 2).  For an odd count the two are the same element.
struct SelectState {
    unsigned hist[4][256];
    unsigned prefix[4];  // the key's digits chosen so far, in place
    unsigned k[4];       // rank of the wanted element among the keys that share the prefix
    unsigned n;          // pixels in the mask
    unsigned nan_count;  // NaN predictions in the mask (gt > 0 is false for a NaN)
    unsigned umin_key;   // order_key of the smallest resized uncertainty
    unsigned u_nan;      // a resized uncertainty is NaN
};

struct ScoreResult {  // what mvd_depth_score_f32 writes: 40 bytes
    double sum_rel_ae;
    long long n_mask, n_inliers, n_eval;
    float min_rel_ae;
    unsigned min_key;  // scratch of the minimum while the pass runs
};
static_assert(sizeof(ScoreResult) == 40, "include/mvd.h documents 40 bytes");

struct Maps {  // gt (H,W) and the prediction (h,w) seen through the index tables
    const float* gt;
    const float* pred;
    const int* row;
    const int* col;
    int W, w;
    long long N;
    __device__ __forceinline__ long long src(long long p) const {
        const long long y = p / W;
        return (long long)row[y] * w + col[p - y * W];
    }
};

__device__ __forceinline__ double block_sum(double v, double* lds) {  // fixed-order tree over the workgroup's 256 lanes
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int s = EV_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] = lds[t] + lds[t + s];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(EV_THREADS) align_init_kernel(SelectState* st) {
    unsigned* p = reinterpret_cast<unsigned*>(st);
    for (unsigned i = threadIdx.x; i < sizeof(SelectState) / 4; i += EV_THREADS) p[i] = 0u;
    __syncthreads();
    if (threadIdx.x == 0) st->umin_key = 0xffffffffu;
}

// minimum of the resized uncertainty over ALL pixels (metrics.py:169 takes uncertainty.min() of the whole map)
__global__ void __launch_bounds__(EV_THREADS) umin_kernel(Maps m, const float* __restrict__ unc, SelectState* st) {
    __shared__ unsigned s_min, s_nan;
    if (threadIdx.x == 0) { s_min = 0xffffffffu; s_nan = 0u; }
    __syncthreads();
    unsigned kmin = 0xffffffffu, isnan = 0u;
    const long long base = (long long)blockIdx.x * EV_PIX;
    for (int i = threadIdx.x; i < EV_PIX && base + i < m.N; i += EV_THREADS) {
        const float u = unc[m.src(base + i)];
        if (u != u) isnan = 1u; else kmin = min(kmin, order_key(u));
    }
    atomicMin(&s_min, kmin);
    if (isnan) atomicOr(&s_nan, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(&st->umin_key, s_min);
        if (s_nan) atomicOr(&st->u_nan, 1u);
    }
}

// One 8-bit digit of the radix select, most significant first: histograms of that digit over the masked keys that carry the prefix
// chosen by the earlier passes, for the four selections at once, in LDS and then added to the global ones.
__global__ void __launch_bounds__(EV_THREADS) median_hist_kernel(Maps m, int sparse, int pass, SelectState* st) {
    __shared__ unsigned lh[4][256];
    __shared__ unsigned s_nan;
    const int t = threadIdx.x;
    for (int s = 0; s < 4; ++s) lh[s][t] = 0u;
    if (t == 0) s_nan = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    unsigned pre[4];
    for (int s = 0; s < 4; ++s) pre[s] = st->prefix[s];
    unsigned nans = 0u;
    const long long base = (long long)blockIdx.x * EV_PIX;
    for (int i = t; i < EV_PIX && base + i < m.N; i += EV_THREADS) {
        const long long p = base + i;
        const float g = m.gt[p], q = m.pred[m.src(p)];
        if (!(g > 0.f) || (sparse && q == 0.f)) continue;
        const unsigned kg = order_key(g), kq = order_key(q);
        if (q != q) ++nans;
        for (int which = 0; which < 2; ++which) {
            if ((kg & himask) == pre[which]) atomicAdd(&lh[which][(kg >> shift) & 255u], 1u);
            if ((kq & himask) == pre[2 + which]) atomicAdd(&lh[2 + which][(kq >> shift) & 255u], 1u);
        }
    }
    if (pass == 0 && nans) atomicAdd(&s_nan, nans);
    __syncthreads();
    for (int s = 0; s < 4; ++s)
        if (lh[s][t]) atomicAdd(&st->hist[s][t], lh[s][t]);
    if (t == 0 && s_nan) atomicAdd(&st->nan_count, s_nan);
}

// Chooses each selection's bin of this pass from the global histograms, clears them for the next pass, and after the last pass
// forms the medians as np.median does on float32 and the ratio (multi_view_depth_evaluation.py:478-487).
__global__ void __launch_bounds__(EV_THREADS) median_select_kernel(SelectState* st, int pass, float* __restrict__ params) {
    __shared__ unsigned h[256];
    const int t = threadIdx.x;
    const int shift = 24 - 8 * pass;
    for (int s = 0; s < 4; ++s) {
        h[t] = st->hist[s][t];
        st->hist[s][t] = 0u;
        __syncthreads();
        if (t == 0) {
            unsigned k;
            if (pass == 0) {
                unsigned n = 0u;
                for (int b = 0; b < 256; ++b) n += h[b];
                if (s == 0) st->n = n;
                k = (s & 1) ? n / 2u : (n ? (n - 1u) / 2u : 0u);
            } else {
                k = st->k[s];
            }
            unsigned cum = 0u, bin = 255u;
            for (unsigned b = 0; b < 256u; ++b) {
                if (k < cum + h[b]) { bin = b; break; }
                cum += h[b];
            }
            st->k[s] = k - min(cum, k);
            st->prefix[s] |= bin << shift;
        }
        __syncthreads();
    }
    if (pass == 3 && t == 0) {
        const unsigned n = st->n;
        const float nan = __uint_as_float(0x7fc00000u);
        float mg = nan, mp = nan;
        if (n) {
            const float g0 = order_key_inv(st->prefix[0]), g1 = order_key_inv(st->prefix[1]);
            const float p0 = order_key_inv(st->prefix[2]), p1 = order_key_inv(st->prefix[3]);
            mg = (n & 1u) ? g0 : (g0 + g1) / 2.0f;  // np.mean of the two middle values in float32
            mp = (n & 1u) ? p0 : (p0 + p1) / 2.0f;
            if (st->nan_count) mp = nan;
        }
        const float ratio = mg / mp;
        params[0] = (n && finite_f32(ratio)) ? ratio : nan;  // NaN = "do not scale"
        params[1] = 0.f;
        params[2] = mg;
        params[3] = mp;
        params[4] = (float)(n != 0u);
    }
}

// least_squares_scale_shift (:489-529): per-workgroup float64 partials of  sum p^2, sum p, sum g p, sum g  over the mask, with
// p = nan_to_num(1 / pred), g = nan_to_num(1 / gt)
__global__ void __launch_bounds__(EV_THREADS) lsq_partial_kernel(Maps m, int sparse, double* __restrict__ partials, SelectState* st) {
    __shared__ double lds[EV_THREADS];
    __shared__ unsigned s_n;
    if (threadIdx.x == 0) s_n = 0u;
    __syncthreads();
    double a00 = 0.0, a01 = 0.0, b0 = 0.0, b1 = 0.0;
    unsigned cnt = 0u;
    const long long base = (long long)blockIdx.x * EV_PIX;
    for (int i = threadIdx.x; i < EV_PIX && base + i < m.N; i += EV_THREADS) {
        const long long p = base + i;
        const float g = m.gt[p], q = m.pred[m.src(p)];
        if (!(g > 0.f) || (sparse && q == 0.f)) continue;
        const double pi = (double)finite_or(1.0f / q, 0.f), gi = (double)finite_or(1.0f / g, 0.f);
        a00 = a00 + pi * pi;
        a01 = a01 + pi;
        b0 = b0 + gi * pi;
        b1 = b1 + gi;
        ++cnt;
    }
    if (cnt) atomicAdd(&s_n, cnt);
    a00 = block_sum(a00, lds);
    a01 = block_sum(a01, lds);
    b0 = block_sum(b0, lds);
    b1 = block_sum(b1, lds);
    if (threadIdx.x == 0) {
        double* o = partials + 4 * (long long)blockIdx.x;
        o[0] = a00; o[1] = a01; o[2] = b0; o[3] = b1;
        if (s_n) atomicAdd(&st->n, s_n);
    }
}

__global__ void __launch_bounds__(EV_THREADS) lsq_final_kernel(const double* __restrict__ partials, int nwg, const SelectState* st,
                                                               float* __restrict__ params, double* __restrict__ sums) {
    __shared__ double lds[EV_THREADS];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nwg; i += EV_THREADS)
        for (int c = 0; c < 4; ++c) acc[c] = acc[c] + partials[4 * (long long)i + c];
    for (int c = 0; c < 4; ++c) acc[c] = block_sum(acc[c], lds);
    if (threadIdx.x == 0) {
        const double a00 = acc[0], a01 = acc[1], b0 = acc[2], b1 = acc[3], a11 = (double)st->n;
        const float nan = __uint_as_float(0x7fc00000u);
        float scale = nan, shift = nan;
        int valid = 0;
        if (st->n) {
            const double det = a00 * a11 - a01 * a01;
            valid = det > 0.0;
            if (valid) {
                scale = (float)((a11 * b0 - a01 * b1) / det);
                shift = (float)((-a01 * b0 + a00 * b1) / det);
            }
        }
        params[0] = scale;
        params[1] = shift;
        params[2] = nan;
        params[3] = nan;
        params[4] = (float)valid;
        if (sums) { sums[0] = a00; sums[1] = a01; sums[2] = a11; sums[3] = b0; sums[4] = b1; }
    }
}

__global__ void align_umin_kernel(const SelectState* st, int have_unc, int mode, float* __restrict__ params) {
    const float nan = __uint_as_float(0x7fc00000u);
    if (mode == MVD_ALIGN_NONE) {
        params[0] = nan; params[1] = 0.f; params[2] = nan; params[3] = nan; params[4] = 0.f;
    }
    params[5] = !have_unc || st->u_nan ? nan : order_key_inv(st->umin_key);
    params[6] = 0.f;
    params[7] = 0.f;
}

__global__ void score_init_kernel(ScoreResult* r) {
    r->sum_rel_ae = 0.0;
    r->n_mask = r->n_inliers = r->n_eval = 0;
    r->min_rel_ae = 0.f;
    r->min_key = 0xffffffffu;
}

struct ScoreArgs {
    int mode, sparse, clip;
    float clip_lo, clip_hi, thresh, thresh_p1;
    const float* params;
    const float* unc;
    float *pred_out, *invdepth_out, *rel_ae_out, *unc_out;
};

// One run's post-processing and metrics, one lane per pixel (_postprocess_sample_and_output :531-547, _compute_metrics :583-610,
// metrics.py:32-135)
__global__ void __launch_bounds__(EV_THREADS) score_kernel(Maps m, ScoreArgs a, double* __restrict__ partials, ScoreResult* res) {
    __shared__ double lds[EV_THREADS];
    __shared__ unsigned s_cnt[3], s_min;
    if (threadIdx.x == 0) { s_cnt[0] = s_cnt[1] = s_cnt[2] = 0u; s_min = 0xffffffffu; }
    __syncthreads();
    const float p0 = a.mode != MVD_ALIGN_NONE ? a.params[0] : 0.f, p1 = a.mode == MVD_ALIGN_LSQ ? a.params[1] : 0.f;
    double sum = 0.0;
    unsigned n_mask = 0u, n_inl = 0u, n_eval = 0u, kmin = 0xffffffffu;
    const long long base = (long long)blockIdx.x * EV_PIX;
    for (int i = threadIdx.x; i < EV_PIX && base + i < m.N; i += EV_THREADS) {
        const long long p = base + i, sp = m.src(p);
        const float g = m.gt[p];
        float q = m.pred[sp];
        const float pm = (a.sparse && q == 0.f) ? 0.f : 1.f;  // prediction mask of the raw resized map
        if (a.mode == MVD_ALIGN_MEDIAN) {
            if (p0 == p0) q = q * p0;
        } else if (a.mode == MVD_ALIGN_LSQ) {
            float inv = finite_or(1.0f / q, 0.f);
            inv = p0 * inv;
            inv = inv + p1;
            q = finite_or(1.0f / inv, 0.f);
        }
        if (a.clip) {
            if (q == q) q = fminf(fmaxf(q, a.clip_lo), a.clip_hi);  // np.clip keeps a NaN
            q = q * pm;
        }
        const float inv = finite_or(1.0f / q, 0.f);
        const bool em = !(a.sparse && q == 0.f);  // evaluation mask of the final map
        const float mf = (g > 0.f ? 1.f : 0.f) * (em ? 1.f : 0.f);
        const float rel = finite_or(fabsf(q - g) / g, 0.f) * mf;
        const float mx = fmaxf(finite_or(g / q, a.thresh_p1), finite_or(q / g, 0.f));
        const bool inl = 0.f < mx && mx < a.thresh;
        n_mask += mf != 0.f;
        n_inl += inl && mf != 0.f;
        n_eval += em;
        sum = sum + (double)rel;
        kmin = min(kmin, order_key(rel));
        if (a.pred_out) a.pred_out[p] = q;
        if (a.invdepth_out) a.invdepth_out[p] = inv;
        if (a.rel_ae_out) a.rel_ae_out[p] = rel;
        if (a.unc_out) a.unc_out[p] = a.unc[sp];
    }
    if (n_mask) atomicAdd(&s_cnt[0], n_mask);
    if (n_inl) atomicAdd(&s_cnt[1], n_inl);
    if (n_eval) atomicAdd(&s_cnt[2], n_eval);
    atomicMin(&s_min, kmin);
    sum = block_sum(sum, lds);  // its barriers also order the LDS atomics above before the reads below
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = sum;
        if (s_cnt[0]) atomicAdd(reinterpret_cast<unsigned long long*>(&res->n_mask), (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(reinterpret_cast<unsigned long long*>(&res->n_inliers), (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(reinterpret_cast<unsigned long long*>(&res->n_eval), (unsigned long long)s_cnt[2]);
        atomicMin(&res->min_key, s_min);
    }
}

__global__ void __launch_bounds__(EV_THREADS) score_final_kernel(const double* __restrict__ partials, int nwg, ScoreResult* res) {
    __shared__ double lds[EV_THREADS];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nwg; i += EV_THREADS) acc = acc + partials[i];
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) {
        res->sum_rel_ae = acc;
        res->min_rel_ae = order_key_inv(res->min_key);
    }
}

__global__ void __launch_bounds__(EV_THREADS) rank_keys_kernel(const float* __restrict__ u, const float* __restrict__ u_min,
                                                               const float* __restrict__ gt, const float* __restrict__ pred_aligned,
                                                               int sparse, long long N, float* __restrict__ keys) {
    const long long p = (long long)blockIdx.x * EV_THREADS + threadIdx.x;
    if (p >= N) return;
    const float mf = (gt[p] > 0.f ? 1.f : 0.f) * ((sparse && pred_aligned[p] == 0.f) ? 0.f : 1.f);
    keys[p] = ((u[p] - u_min[0]) + 1.0f) * mf;  // metrics.py:169
}

// step i of metrics.py:176, int((num_valid / 100) * i): a float64 division, a float64 product, a truncation
__device__ __forceinline__ long long sparsification_step(long long n, int i) {
    const double per = (double)n / 100.0;
    return (long long)(per * (double)i);
}

// workgroup j sums the ranked errors between step j and step j + 1 (the count for j = 99)
__global__ void __launch_bounds__(EV_THREADS) step_segment_kernel(const float* __restrict__ ranked, long long len,
                                                                  const long long* __restrict__ count, double* __restrict__ seg) {
    __shared__ double lds[EV_THREADS];
    long long n = count[0];
    n = n < 0 ? 0 : (n > len ? len : n);
    const int j = blockIdx.x;
    const long long s = sparsification_step(n, j), e = j + 1 < EV_STEPS ? sparsification_step(n, j + 1) : n;
    double acc = 0.0;
    for (long long i = s + threadIdx.x; i < e; i += EV_THREADS) acc = acc + (double)ranked[i];
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) seg[j] = acc;
}

__global__ void step_suffix_kernel(const double* __restrict__ seg, double* __restrict__ out) {
    double acc = 0.0;
    for (int j = EV_STEPS - 1; j >= 0; --j) {
        acc = acc + seg[j];
        out[j] = acc;
    }
}

static inline long long eval_workgroups(long long N) { return (N + EV_PIX - 1) / EV_PIX; }
static inline size_t state_bytes() { return align_up(sizeof(SelectState), 256); }

}  // namespace mvd

extern "C" size_t mvd_depth_eval_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    const long long nwg = mvd::eval_workgroups((long long)H * W);
    const size_t partials = (size_t)(nwg > mvd::EV_STEPS ? nwg : mvd::EV_STEPS) * 4 * sizeof(double);
    return mvd::state_bytes() + partials;
}

#define MVD_EVAL_SHAPES(what)                                                                                          \
    MVD_REQUIRE(H > 0 && W > 0 && h > 0 && w > 0, what ": bad dimension");                                             \
    MVD_REQUIRE((long long)H * W <= 0x7fffffffLL && (long long)h * w <= 0x7fffffffLL, what ": map too large");       \
    MVD_REQUIRE(workspace && workspace_bytes >= mvd_depth_eval_workspace_bytes(H, W), what ": workspace too small")

extern "C" int mvd_depth_align_stats_f32(const float* gt, const float* pred, const float* uncertainty, const int* row, const int* col,
                                         int H, int W, int h, int w, int mode, int sparse_pred, float* params, double* sums,
                                         void* workspace, size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(gt && pred && row && col && params, "depth_align_stats: NULL argument");
    MVD_EVAL_SHAPES("depth_align_stats");
    MVD_REQUIRE(mode == MVD_ALIGN_NONE || mode == MVD_ALIGN_MEDIAN || mode == MVD_ALIGN_LSQ, "depth_align_stats: bad mode %d", mode);
    hipStream_t st = (hipStream_t)stream;
    const Maps m{gt, pred, row, col, W, w, (long long)H * W};
    const unsigned nwg = (unsigned)eval_workgroups(m.N);
    SelectState* state = static_cast<SelectState*>(workspace);
    double* partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + state_bytes());
    hipLaunchKernelGGL(align_init_kernel, dim3(1), dim3(EV_THREADS), 0, st, state);
    if (uncertainty) hipLaunchKernelGGL(umin_kernel, dim3(nwg), dim3(EV_THREADS), 0, st, m, uncertainty, state);
    if (mode == MVD_ALIGN_MEDIAN) {
        for (int pass = 0; pass < 4; ++pass) {
            hipLaunchKernelGGL(median_hist_kernel, dim3(nwg), dim3(EV_THREADS), 0, st, m, sparse_pred, pass, state);
            hipLaunchKernelGGL(median_select_kernel, dim3(1), dim3(EV_THREADS), 0, st, state, pass, params);
        }
    } else if (mode == MVD_ALIGN_LSQ) {
        hipLaunchKernelGGL(lsq_partial_kernel, dim3(nwg), dim3(EV_THREADS), 0, st, m, sparse_pred, partials, state);
        hipLaunchKernelGGL(lsq_final_kernel, dim3(1), dim3(EV_THREADS), 0, st, partials, (int)nwg, state, params, sums);
    }
    hipLaunchKernelGGL(align_umin_kernel, dim3(1), dim3(1), 0, st, state, uncertainty != nullptr, mode, params);
    return launch_status("depth_align_stats");
}

extern "C" int mvd_depth_score_f32(const float* gt, const float* pred, const float* uncertainty, const int* row, const int* col, int H,
                                   int W, int h, int w, int mode, int sparse_pred, int clip, float clip_lo, float clip_hi,
                                   float thresh, float thresh_plus_one, const float* params, void* result, float* pred_out,
                                   float* invdepth_out, float* rel_ae_out, float* uncertainty_out, void* workspace,
                                   size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(gt && pred && row && col && result, "depth_score: NULL argument");
    MVD_EVAL_SHAPES("depth_score");
    MVD_REQUIRE(mode == MVD_ALIGN_NONE || mode == MVD_ALIGN_MEDIAN || mode == MVD_ALIGN_LSQ, "depth_score: bad mode %d", mode);
    MVD_REQUIRE(mode == MVD_ALIGN_NONE || params, "depth_score: an alignment needs its parameters");
    MVD_REQUIRE(!uncertainty_out || uncertainty, "depth_score: uncertainty_out without uncertainty");
    MVD_REQUIRE(((uintptr_t)result & 7) == 0, "depth_score: result must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const Maps m{gt, pred, row, col, W, w, (long long)H * W};
    const unsigned nwg = (unsigned)eval_workgroups(m.N);
    double* partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + state_bytes());
    ScoreResult* res = static_cast<ScoreResult*>(result);
    const ScoreArgs a{mode, sparse_pred, clip, clip_lo, clip_hi, thresh, thresh_plus_one, params, uncertainty,
                      pred_out, invdepth_out, rel_ae_out, uncertainty_out};
    hipLaunchKernelGGL(score_init_kernel, dim3(1), dim3(1), 0, st, res);
    hipLaunchKernelGGL(score_kernel, dim3(nwg), dim3(EV_THREADS), 0, st, m, a, partials, res);
    hipLaunchKernelGGL(score_final_kernel, dim3(1), dim3(EV_THREADS), 0, st, partials, (int)nwg, res);
    return launch_status("depth_score");
}

extern "C" int mvd_rank_keys_f32(const float* u, const float* u_min, const float* gt, const float* pred_aligned, int sparse_pred,
                                 long long n, float* keys, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(u && u_min && gt && pred_aligned && keys, "rank_keys: NULL argument");
    MVD_REQUIRE(n > 0 && n <= 0x7fffffffLL, "rank_keys: bad dimension");
    hipLaunchKernelGGL(rank_keys_kernel, dim3((unsigned)((n + EV_THREADS - 1) / EV_THREADS)), dim3(EV_THREADS), 0, (hipStream_t)stream,
                       u, u_min, gt, pred_aligned, sparse_pred, n, keys);
    return launch_status("rank_keys");
}

extern "C" int mvd_ranked_step_sums_f64(const float* ranked, long long n, const long long* count, double* step_sums, void* workspace,
                                        size_t workspace_bytes, mvd_stream_t stream) {
    using namespace mvd;
    MVD_REQUIRE(ranked && count && step_sums, "ranked_step_sums: NULL argument");
    MVD_REQUIRE(n > 0 && n <= 0x7fffffffLL, "ranked_step_sums: bad dimension");
    MVD_REQUIRE(workspace && workspace_bytes >= state_bytes() + EV_STEPS * sizeof(double), "ranked_step_sums: workspace too small");
    MVD_REQUIRE(((uintptr_t)count & 7) == 0, "ranked_step_sums: count must be 8-byte aligned");
    double* seg = reinterpret_cast<double*>(static_cast<char*>(workspace) + state_bytes());
    hipLaunchKernelGGL(step_segment_kernel, dim3(EV_STEPS), dim3(EV_THREADS), 0, (hipStream_t)stream, ranked, n, count, seg);
    hipLaunchKernelGGL(step_suffix_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, seg, step_sums);
    return launch_status("ranked_step_sums");
}
