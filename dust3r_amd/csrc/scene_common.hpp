// dust3r_amd -- what the kernels over a scene's padded stacks share (mesh.hip, fuse.hip): the tile size, a view's pixel count, the colour
// rule of a pixel and the fixed-order bounds reduction of a 1024-thread workgroup.
#pragma once
#include "common.hpp"

namespace d3r {
namespace scene {

constexpr int NT = 1024;        // threads of the tile / pixel workgroups = elements per tile

// a view's pixel count; 0 (the view is treated as empty) when its size is negative or does not fit its row of max_area
D3R_DEV int area_of(int H, int W, int max_area) { return H >= 0 && W >= 0 && (long long)H * W <= max_area ? H * W : 0; }

// colour q of a pixel, packed r | g << 8 | b << 16: the byte itself (uint8 input), else floor(255 c + 1/2) clamped to [0, 255] (fp32
// product and sum, no contraction; NaN -> 0)
D3R_DEV uint32_t q8(float c) { return (uint32_t)fminf(fmaxf(floorf(__fadd_rn(__fmul_rn(255.f, c), 0.5f)), 0.f), 255.f); }
D3R_DEV uint32_t pixel_q(const void* rgb, int is_u8, size_t g) {
    if (is_u8) {
        const uint8_t* q = (const uint8_t*)rgb + 3 * g;
        return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    }
    const float* q = (const float*)rgb + 3 * g;
    return q8(q[0]) | (q8(q[1]) << 8) | (q8(q[2]) << 16);
}

D3R_DEV void bounds_add(float (&b)[6], const float* p) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        b[c] = fminf(b[c], p[c]);
        b[3 + c] = fmaxf(b[3 + c], p[c]);
    }
}

// the workgroup's bounds (wave butterflies, then wave 0's lanes 0-5 over the 16 waves in order) -> out[6]
D3R_DEV void block_bounds(float (&b)[6], float* lds, float* out) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float t = __shfl_xor(b[c], o);
            b[c] = c < 3 ? fminf(b[c], t) : fmaxf(b[c], t);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) lds[wave * 6 + c] = b[c];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        float r = lds[c];
        for (int w = 1; w < NT / 64; ++w) r = c < 3 ? fminf(r, lds[w * 6 + c]) : fmaxf(r, lds[w * 6 + c]);
        out[c] = r;
    }
}

D3R_DEV void bounds_init(float (&b)[6]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        b[c] = __builtin_huge_valf();
        b[3 + c] = -__builtin_huge_valf();
    }
}

}  // namespace scene
}  // namespace d3r
