// dust3r_amd -- scene.fuse(): the per-view pointmaps of a scene merged into ONE voxel-fused, confidence-weighted cloud (new; the reference
// exports every masked pixel of every view). Inputs are the scene's padded stacks, as for d3r_scene_mesh (utils/padded.py): view v is
// elements [0, h w) of row v, flat index g = v row + e; what lies behind h w is never read.
//
// A pixel is VALID when its mask is nonzero, its three coordinates are finite and its weight is finite and > 0 (no weights: 1).
//   d3r_fuse_bounds   fuse_bounds_kernel        per workgroup, the bounds and the count of the valid points of its pixels
//                     fuse_bounds_final_kernel  one workgroup over the partials in index order
//   d3r_fuse_voxels   1. key and compact: fuse_flag_kernel<KEYS, false> counts the valid pixels of every tile, fuse_scan_kernel scans the tile
//                        counts, fuse_flag_kernel<KEYS, true> places (key, g) of every valid pixel, view then raster order;
//                        key = q_x | q_y << bits_x | q_z << (bits_x + bits_y), q_c = (int)floorf((p_c - lo_c) / voxel) in fp32
//                     2. stable LSD radix sort by key, 4 bits per pass, over bits_x + bits_y + bits_z bits only. Per pass three launches:
//                        fuse_hist_kernel (per tile of SUB x 1024 pairs the count of each digit, digit-major), fuse_scan_kernel over the
//                        16 x tiles counts, fuse_scatter_kernel (rank inside the tile from wave ballots, tiles in order)
//                     3. segment heads: key[i] != key[i - 1], compacted with the pattern of stage 1 (fuse_flag_kernel<HEADS, ...>)
//                     4. fuse_reduce_kernel: one thread per voxel walks its points in sorted order (= view, then raster: the sort is
//                        stable) and sums in fp64
// Stages 1-3 (kernels, workspace, launch sequence) live in fuse_grid.hpp, shared with cloud_nn.hip; the bounds and stage 4 are here.
// No kernel waits on another workgroup: every scan over tiles is a launch of its own (ONE workgroup, chunks in order), there is no
// atomic, no look-back, no grid barrier. Integer placement and fixed-order fp64 sums: the same bytes on every run, and the bytes of the
// numpy restatement (tests/test_fuse_cpu.py). A voxel as large as the scene makes one thread walk every point: slow but finite, not a target.
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "scene_common.hpp"
#include "fuse_grid.hpp"

namespace d3r {
namespace fuse {

__global__ __launch_bounds__(NT) void fuse_bounds_kernel(const float* __restrict__ pts, const uint8_t* __restrict__ mask, const float* __restrict__ weight,
                                                        const int* __restrict__ img_h, const int* __restrict__ img_w, int row,
                                                        float* __restrict__ partials, int* __restrict__ part_cnt) {
    __shared__ float lds_b[WAVES * 6];
    __shared__ int wave_cnt[WAVES];
    const int v = blockIdx.y;
    const long long area = area_of(img_h[v], img_w[v], row);
    const size_t base = (size_t)v * row;
    float b[6];
    bounds_init(b);
    int cnt[1] = {0};
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < area; e += (long long)gridDim.x * NT) {
        if (valid_at(pts, mask, weight, base + e)) {
            bounds_add(b, pts + 3 * (base + e));
            ++cnt[0];
        }
    }
    const size_t part = (size_t)v * gridDim.x + blockIdx.x;
    block_bounds(b, lds_b, partials + part * 6);
    block_reduce_gather<NT, false>(cnt, wave_cnt, Sum());
    if (threadIdx.x == 0) part_cnt[part] = cnt[0];
}

__global__ __launch_bounds__(256) void fuse_bounds_final_kernel(int n_parts, const float* __restrict__ partials, const int* __restrict__ part_cnt,
                                                               float* __restrict__ bounds_out, long long* __restrict__ count_out) {
    bounds_final<true>(n_parts, partials, part_cnt, bounds_out, count_out);
}

// voxel j = the sorted pairs [starts[j], starts[j + 1]) (the last: up to N), walked in order
__global__ __launch_bounds__(256) void fuse_reduce_kernel(const int* __restrict__ idx, const int* __restrict__ starts, const int* __restrict__ n_dev,
                                                         const int* __restrict__ m_dev, int cap, const float* __restrict__ pts,
                                                         const float* __restrict__ weight, const void* __restrict__ rgb, int is_u8,
                                                         float* __restrict__ positions, uint32_t* __restrict__ colors, float* __restrict__ weight_out,
                                                         int* __restrict__ count_out, long long* __restrict__ totals_out) {
    const int N = count_of(n_dev, cap), M = count_of(m_dev, cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        totals_out[0] = N;
        totals_out[1] = M;
    }
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < M; j += (long long)gridDim.x * 256) {
        const int s = starts[j], e = j + 1 < M ? starts[j + 1] : N;
        double W = 0.0, S[3] = {0.0, 0.0, 0.0}, C[3] = {0.0, 0.0, 0.0};
        for (int i = s; i < e; ++i) {
            const size_t g = (size_t)idx[i];
            const double w = weight ? (double)weight[g] : 1.0;
            const float* p = pts + 3 * g;
            const uint32_t q = pixel_q(rgb, is_u8, g);
            W += w;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                S[c] += w * (double)p[c];                               // exact products (24 + 24 bits), one rounding per sum
                C[c] += w * (double)((q >> (8 * c)) & 0xFFu);
            }
        }
        uint32_t rgba = 0xFF000000u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            positions[3 * j + c] = (float)(S[c] / W);
            rgba |= (uint32_t)fmin(fmax(floor(C[c] / W + 0.5), 0.0), 255.0) << (8 * c);
        }
        colors[j] = rgba;
        weight_out[j] = (float)W;
        count_out[j] = e - s;
    }
}

}  // namespace fuse
}  // namespace d3r

using namespace d3r;
using namespace d3r::fuse;

extern "C" size_t d3r_fuse_bounds_workspace_bytes(int n_views, int row) {
    if (n_views <= 0 || row <= 0) return 0;
    const size_t parts = (size_t)n_views * blocks_of(tiles_of(row, NT), MAX_BLOCKS);
    Carver c(nullptr);                                                  // as d3r_fuse_bounds carves it
    c.take<float>(parts * 6);
    c.take<int>(parts);
    return c.bytes;
}

extern "C" int d3r_fuse_bounds(int n_views, const float* pts, const uint8_t* mask, const float* weight, const int* img_h_dev, const int* img_w_dev, int row,
                               float* bounds_out, long long* count_out, void* workspace, void* stream) {
    if (n_views <= 0 || n_views > 65535 || !pts || !mask || !img_h_dev || !img_w_dev || row <= 0 || (long long)n_views * row > 2147483647LL ||
        !bounds_out || !count_out || !workspace)
        return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int bx = blocks_of(tiles_of(row, NT), MAX_BLOCKS);
    const size_t parts = (size_t)n_views * bx;
    Carver c(workspace);
    float* partials = c.take<float>(parts * 6);
    int* part_cnt = c.take<int>(parts);
    hipLaunchKernelGGL(fuse_bounds_kernel, dim3(bx, n_views), dim3(NT), 0, st, pts, mask, weight, img_h_dev, img_w_dev, row, partials, part_cnt);
    hipLaunchKernelGGL(fuse_bounds_final_kernel, dim3(1), dim3(256), 0, st, (int)parts, partials, part_cnt, bounds_out, count_out);
    return rc_of(hipGetLastError());
}

extern "C" size_t d3r_fuse_voxels_workspace_bytes(int n_views, int row, int capacity) {
    if (!fuse_shape_ok(n_views, row, capacity)) return 0;
    return fuse_workspace(nullptr, n_views, row, capacity).bytes;
}

extern "C" int d3r_fuse_voxels(int n_views, const float* pts, const uint8_t* mask, const float* weight, const void* rgb, int rgb_is_u8, const int* img_h_dev,
                               const int* img_w_dev, int row, const float* lo, float voxel, const int* bits, int capacity, float* positions_out,
                               uint32_t* colors_out, float* weight_out, int* count_out, long long* totals_out, void* workspace, void* stream) {
    if (!fuse_shape_ok(n_views, row, capacity) || !pts || !mask || !rgb || !img_h_dev || !img_w_dev || !lo || !bits || !positions_out || !colors_out ||
        !weight_out || !count_out || !totals_out || !workspace || !(voxel > 0.f) || !(voxel <= 3.0e38f))
        return D3R_ERR_INVALID;
    FlagArgs a;
    int total_bits = 0;
    if (!fuse_key_params(lo, voxel, bits, &a.key, &total_bits)) return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const FuseWorkspace w = fuse_workspace(workspace, n_views, row, capacity);
    a.pts = pts; a.mask = mask; a.weight = weight; a.img_h = img_h_dev; a.img_w = img_w_dev;
    a.row = row;
    // 1.-3. key and compact, sort, segment heads (fuse_grid.hpp)
    const int cur = fuse_key_and_sort(a, w, n_views, capacity, total_bits, st);
    const int* starts = fuse_segment_heads(a, w, cur, capacity, st);
    // 4. reduce
    hipLaunchKernelGGL(fuse_reduce_kernel, dim3(blocks_of(tiles_of(capacity, 256), MAX_BLOCKS)), dim3(256), 0, st, w.idx[cur], starts, w.n_dev, w.n_dev + 1, capacity,
                       pts, weight, rgb, rgb_is_u8, positions_out, colors_out, weight_out, count_out, totals_out);
    return rc_of(hipGetLastError());
}
