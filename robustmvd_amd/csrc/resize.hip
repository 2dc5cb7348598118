// Input resize of the model adapters on the device.
// Replaces ResizeInputs / UpscaleInputsToNextMultipleOf (rmvd/data/transforms.py:40-98), i.e.
// skimage.transform.resize(image, (..., ht, wd), order=1) for the only case the adapters produce: UPSCALING to the next
// multiple of 64 / 32 (robust_mvd.py:104-113, mvsnet.py:178).  For that case skimage applies no anti-aliasing filter,
// keeps float32 and delegates to scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True), whose arithmetic this
// kernel follows operation for operation in float64:
//   zoom = n_in / n_out;  c = (o + 0.5) * zoom - 0.5;  mirror c into [0, n_in - 1];  i0 = floor(c), w1 = c - i0,
//   w0 = 1 - w1, i1 = i0 + 1 (mirrored);  t = ((a00*wy0)*wx0 + (a01*wy0)*wx1) + (a10*wy1)*wx0 + (a11*wy1)*wx1.
// HBM-bound, trivially small (5 images of 3.7 MB per frame): one thread per output pixel.
#include "mvd_common.h"

namespace mvd {

struct AxisTap {
    int i0, i1;
    double w0, w1;
};

__device__ __forceinline__ AxisTap axis_tap(int o, int n_in, int n_out) {
    AxisTap t;
    if (n_in <= 1) {
        t.i0 = t.i1 = 0; t.w0 = 1.0; t.w1 = 0.0;
        return t;
    }
    const double zoom = (double)n_in / (double)n_out;
    double c = ((double)o + 0.5) * zoom - 0.5;
    const double last = (double)(n_in - 1), sz2 = 2.0 * last;
    if (c < 0.0) c = -c;          // upscaling: |c| < 0.5, one reflection is enough
    if (c > last) c = sz2 - c;
    const double st = floor(c);
    t.w1 = c - st;
    t.w0 = 1.0 - t.w1;
    t.i0 = (int)st;
    t.i1 = t.i0 + 1;
    if (t.i1 > n_in - 1) t.i1 = 2 * (n_in - 1) - t.i1;
    return t;
}

__global__ void __launch_bounds__(256) resize_order1_kernel(const float* __restrict__ src, float* __restrict__ dst, int hi, int wi,
                                                            int ho, int wo) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    const size_t plane = blockIdx.z;
    if (x >= wo) return;
    const AxisTap ty = axis_tap(y, hi, ho), tx = axis_tap(x, wi, wo);
    const float* __restrict__ s = src + plane * (size_t)hi * wi;
    const double a00 = s[(size_t)ty.i0 * wi + tx.i0], a01 = s[(size_t)ty.i0 * wi + tx.i1];
    const double a10 = s[(size_t)ty.i1 * wi + tx.i0], a11 = s[(size_t)ty.i1 * wi + tx.i1];
    double t = (a00 * ty.w0) * tx.w0;  // -ffp-contract=off: one rounding per operation, like the reference's C loop
    t = t + (a01 * ty.w0) * tx.w1;
    t = t + (a10 * ty.w1) * tx.w0;
    t = t + (a11 * ty.w1) * tx.w1;
    dst[(plane * ho + y) * (size_t)wo + x] = (float)t;
}

// the zero border of K3's staging map (B, h + 3, w + 3, C): row 0, rows h + 1 and h + 2, column 0, columns w + 1 and w + 2.  One
// thread = 4 channels of a border pixel; pixels 0 .. 3 (w + 3) - 1 are the three whole rows, the rest the three columns of rows 1 .. h
__global__ void __launch_bounds__(256) zero_border_nhwc_kernel(float* __restrict__ y, int h, int w, int c4n, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c4 = i % c4n, bp = i / c4n, wp = w + 3;
    int row, col;
    if (bp < 3 * wp) {
        const int r = bp / wp;
        row = r == 0 ? 0 : h + r;
        col = bp - r * wp;
    } else {
        const int q = bp - 3 * wp, r = q / 3, k = q - 3 * r;
        row = 1 + r;
        col = k == 0 ? 0 : w + k;
    }
    float* o = y + (((size_t)blockIdx.y * (h + 3) + row) * wp + col) * (4 * (size_t)c4n) + 4 * c4;
    *reinterpret_cast<float4*>(o) = float4{0.f, 0.f, 0.f, 0.f};
}

}  // namespace mvd

extern "C" int mvd_zero_border_nhwc_f32(float* y, int B, int h, int w, int C, mvd_stream_t stream) {
    MVD_REQUIRE(y, "zero_border_nhwc: NULL argument");
    MVD_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && C > 0 && C % 4 == 0, "zero_border_nhwc: bad dimensions (C a multiple of 4, B 1..65535)");
    MVD_REQUIRE(((uintptr_t)y & 15) == 0, "zero_border_nhwc: y must be 16-byte aligned");
    const long long n = (3LL * (w + 3) + 3LL * h) * (C / 4);
    MVD_REQUIRE(n < 0x7fffffffLL, "zero_border_nhwc: %lld border items", n);
    hipLaunchKernelGGL(mvd::zero_border_nhwc_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, y, h, w,
                       C / 4, (int)n);
    return mvd::launch_status("zero_border_nhwc");
}

extern "C" int mvd_resize_order1_f32(const float* src, float* dst, long long planes, int hi, int wi, int ho, int wo,
                                     mvd_stream_t stream) {
    MVD_REQUIRE(src && dst, "resize_order1: NULL argument");
    MVD_REQUIRE(planes > 0 && planes <= 65535 && hi > 0 && wi > 0, "resize_order1: bad dimensions (planes 1..65535)");
    MVD_REQUIRE(ho >= hi && wo >= wi && ho <= 65535,
                "resize_order1: only upscaling is built (%dx%d -> %dx%d): downscaling takes skimage's anti-aliasing filter", hi,
                wi, ho, wo);
    const dim3 grid((unsigned)((wo + 255) / 256), (unsigned)ho, (unsigned)planes);
    hipLaunchKernelGGL(mvd::resize_order1_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, dst, hi, wi, ho, wo);
    return mvd::launch_status("resize_order1");
}
