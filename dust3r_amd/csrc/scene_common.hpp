// dust3r_amd -- what the kernels over a scene's padded stacks share (mesh.hip, fuse.hip, tracks.hip, the cloud files; sky.hip for area_of):
// the tile size, a view's pixel count, the colour rule of a pixel, and the bounds: their per-point update, the reduction of a 1024-thread
// workgroup and the body of the final kernel over the partials. The reductions are reduce.hpp's, whose header states their order.
#pragma once
#include "common.hpp"
#include "reduce.hpp"

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

// min over columns 0-2, max over 3-5: fminf / fmaxf, so a NaN coordinate loses against any number (callers admit finite points only)
struct BoundsOp {
    D3R_DEV float operator()(float a, float b, int c) const { return c < 3 ? fminf(a, b) : fmaxf(a, b); }
};

// the workgroup's bounds -> out[6], in the order of reduce.hpp (column c by thread c); lds: NT / 64 * 6 floats
D3R_DEV void block_bounds(float (&b)[6], float* lds, float* out) { block_reduce_columns<NT, 6>(b, lds, BoundsOp(), out); }

D3R_DEV void bounds_init(float (&b)[6]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        b[c] = __builtin_huge_valf();
        b[3 + c] = -__builtin_huge_valf();
    }
}

// The body of the two final bounds kernels (mesh_bounds_kernel, fuse_bounds_final_kernel), ONE workgroup of 256: thread t folds the
// partials t, t + 256, ... in index order, then the workgroup's reduction -> bounds_out[6]; COUNT: the int64 sum of part_cnt -> *count_out
template <bool COUNT>
D3R_DEV void bounds_final(int n_parts, const float* __restrict__ partials, const int* __restrict__ part_cnt, float* __restrict__ bounds_out,
                          long long* __restrict__ count_out) {
    __shared__ float lds[4 * 6];
    __shared__ long long lds_n[COUNT ? 4 : 1];
    float b[6];
    bounds_init(b);
    long long n[1] = {0};
    for (int i = threadIdx.x; i < n_parts; i += 256) {
        const float* p = partials + (size_t)i * 6;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            b[c] = fminf(b[c], p[c]);
            b[3 + c] = fmaxf(b[3 + c], p[3 + c]);
        }
        if (COUNT) n[0] += part_cnt[i];
    }
    block_reduce_stage(b, lds, BoundsOp());
    if (COUNT) block_reduce_stage(n, lds_n, Sum());
    __syncthreads();
    if (threadIdx.x < 6) bounds_out[threadIdx.x] = block_reduce_column<256, 6>(lds, threadIdx.x, BoundsOp());
    if (COUNT && threadIdx.x == 6) *count_out = block_reduce_column<256, 1>(lds_n, 0, Sum());
}

}  // namespace scene
}  // namespace d3r
