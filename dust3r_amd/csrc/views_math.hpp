// dust3r_amd -- host/device arithmetic of the view-preparation kernels (csrc/views.hip): the integer tap sum and rounding of the
// separable 8-bit resampler (Pillow's ImagingResample: 22-bit coefficients, a uint8 intermediate between the two passes), the
// nearest-neighbour source index, and the back-projection of a depth sample. Written once for both sides, so the CPU test-suite runs
// the same arithmetic through d3r_selftest_resample_host / d3r_selftest_depth_host before any kernel does.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define D3R_VW_HD __host__ __device__ inline
#else
#define D3R_VW_HD inline
#endif

namespace d3r {
namespace vw {

constexpr int PRECISION_BITS = 32 - 8 - 2;      // coefficients are rounded to this many fractional bits on the host

// (2^21 + sum) >> 22, clipped to a byte
D3R_VW_HD uint8_t clip8(int acc) {
    const int v = acc >> PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// one channel of one output sample: n taps k[0..n) on bytes p[0], p[stride], ...
D3R_VW_HD int tap_sum(const uint8_t* p, int stride, const int32_t* k, int n) {
    int acc = 1 << (PRECISION_BITS - 1);
    for (int i = 0; i < n; ++i) acc += (int)p[(long)i * stride] * k[i];
    return acc;
}

// a row of the bounds table {first source sample, number of taps}, clamped so that no tap leaves [0, in) or the table row
D3R_VW_HD void clamp_bounds(int first, int count, int in, int ksize, int* first_out, int* count_out) {
    first = first < 0 ? 0 : (first > in ? in : first);
    count = count < 0 ? 0 : (count > ksize ? ksize : count);
    if (count > in - first) count = in - first;
    *first_out = first;
    *count_out = count;
}

// OpenCV's INTER_NEAREST with a given dsize: floor(d * in / out) evaluated in double, capped at in - 1. d * in is an exact integer far
// below 2^53 and the quotient is never within an ulp of an integer it does not reach, so this is the integer floor division.
D3R_VW_HD int nearest_index(int d, int in, int out) {
    const long long s = ((long long)d * in) / out;
    return (int)(s < in - 1 ? s : in - 1);
}

// camera-frame point of pixel (u, v) with depth z: fp64 arithmetic rounded to fp32 (numpy promotes the integer grid minus an fp32
// principal point to fp64), then the fp32 cam2world rotation and translation. pose = the first three rows of cam2world, row-major [3][4].
D3R_VW_HD void backproject(int u, int v, float z, float fu, float fv, float cu, float cv, const float* pose, float* world) {
    const float x = (float)(((double)u - (double)cu) * (double)z / (double)fu);
    const float y = (float)(((double)v - (double)cv) * (double)z / (double)fv);
    for (int r = 0; r < 3; ++r) world[r] = pose[r * 4] * x + pose[r * 4 + 1] * y + pose[r * 4 + 2] * z + pose[r * 4 + 3];
}

D3R_VW_HD bool finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

}  // namespace vw
}  // namespace d3r
