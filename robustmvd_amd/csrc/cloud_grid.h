// The uniform grid shared by the point-cloud kernels (cloud_eval.hip) and the mesh-evaluation kernels (mesh_eval.hip): the cell index
// of a coordinate, the 63-bit key of a cell and the binary search over sorted keys.  One copy, so that a point and a triangle's box
// are put into cells by the same operations.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mvd_common.h"

namespace mvd {

constexpr int CE_BITS = 21;
constexpr int CE_LIMIT = (1 << CE_BITS) - 1;  // a cell index is in [0, CE_LIMIT): the all-ones key is the invalid points' own
constexpr long long CE_INVALID_KEY = 0x7fffffffffffffffLL;

// floor((double(v) - o) * inv), two IEEE double operations and a floor (the library is built without contraction): numpy forms the
// same bits.  Clamped to [lo, hi] before the conversion, so that a far point cannot overflow the int.
__device__ __forceinline__ int cell_index(float v, double o, double inv, double lo, double hi) {
    const double t = floor(((double)v - o) * inv);
    return (int)fmin(fmax(t, lo), hi);
}

__device__ __forceinline__ long long cell_key(int ix, int iy, int iz) {
    return ((long long)ix << (2 * CE_BITS)) | ((long long)iy << CE_BITS) | (long long)iz;
}

__device__ __forceinline__ int lower_bound(const long long* __restrict__ keys, int m, long long key) {
    int lo = 0, hi = m;  // the first position whose key is >= key
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace mvd
