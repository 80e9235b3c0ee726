// dust3r_amd -- host/device arithmetic of the demo's depth / confidence gallery (csrc/gallery.hip): the colour-table row that a
// confidence ratio selects, and the affine map + clip that the reference's rgb() applies to a float picture. Written once for both
// sides, so the CPU test-suite runs the index rule through d3r_selftest_gallery_index_host before any kernel does.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define D3R_GL_HD __host__ __device__ inline
#else
#define D3R_GL_HD inline
#endif

namespace d3r {
namespace gallery {

constexpr int LUT_N = 256;          // rows of the colour table proper
constexpr int LUT_BAD = LUT_N;      // the row behind them: the "bad" colour, taken by NaN
constexpr int LUT_ROWS = LUT_N + 1;

// matplotlib's Colormap.__call__ on a float: x = r * N in the input's precision (a power of two: exact), x == N counts as N - 1, every
// other x is truncated towards zero, x < 0 takes the "under" colour and x >= N the "over" colour (jet leaves both at their defaults: the
// first and the last row), NaN the "bad" colour. -0.0 is not below zero and truncates to row 0.
D3R_GL_HD int lut_index(float r) {
    if (r != r) return LUT_BAD;
    const float x = r * (float)LUT_N;
    if (x < 0.f) return 0;
    if (x >= (float)LUT_N) return LUT_N - 1;
    return (int)x;
}

// NaN-propagating maximum (numpy.max): a NaN on either side wins
D3R_GL_HD float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

}  // namespace gallery
}  // namespace d3r
