// dust3r_amd -- cloud-to-cloud metrics (new; the reference has none): the uniform grid over a reference cloud on which cloud_knn.hip
// searches (d3r_cloud_nearest, d3r_cloud_knn), and the reduction of nearest-neighbour distances to the sums and counts of accuracy /
// completeness / precision / recall (dust3r_amd/cloud_metrics.py). The grid only limits which reference points a search LOOKS AT; the
// contracts of the searches do not mention it (include/dust3r_hip.h; DESIGN.md, "Cloud metrics").
//   d3r_cloud_grid_build     cloud_shape_kernel   the flat cloud as one view of 1 x n (the tables stages 1-3 read)
//                            stages 1-3 of fuse_grid.hpp on the reference cloud: (key, index) of the valid points, sorted, the cell heads
//                            cloud_gather_kernel  the points in sorted order as float4 (x, y, z, original index), so a cell is one run
//                            cloud_cells_kernel   the key and the first point of every cell; one more start = N behind the last
//   d3r_cloud_distance_stats cloud_stats_kernel / cloud_sums_final_kernel<2, 10>   per-workgroup partials, then one workgroup in index order
// As in fuse.hip: no atomics, no kernel waits on another workgroup, no scratch; the same bytes on every run. The workspace layout, the
// checks of cell and radius and the ordered sum are in cloud_grid.hpp, shared with cloud_knn.hip and cloud_icp.hip.
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "scene_common.hpp"
#include "fuse_grid.hpp"
#include "cloud_grid.hpp"

namespace d3r {
namespace cloud {

using namespace d3r::fuse;

constexpr int STAT_I = 2 + D3R_CLOUD_MAX_THRESHOLDS, STAT_D = 2;

// sorted pair i -> (point, original index)
__global__ __launch_bounds__(QT) void cloud_gather_kernel(const float* __restrict__ pts, const int* __restrict__ idx, const int* __restrict__ n_dev, int cap,
                                                         float4* __restrict__ pts4) {
    const int N = count_of(n_dev, cap);
    for (long long i = (long long)blockIdx.x * QT + threadIdx.x; i < N; i += (long long)gridDim.x * QT) {
        const int g = idx[i];
        const float* p = pts + 3 * (size_t)g;
        pts4[i] = make_float4(p[0], p[1], p[2], __int_as_float(g));
    }
}

// cell j -> its key and its first sorted point; cell_start[M] = N
__global__ __launch_bounds__(QT) void cloud_cells_kernel(const uint64_t* __restrict__ sorted, const int* __restrict__ starts, const int* __restrict__ n_dev,
                                                        int cap, uint64_t* __restrict__ cell_key, int* __restrict__ cell_start) {
    const int N = count_of(n_dev, cap), M = count_of(n_dev + 1, cap);
    for (long long j = (long long)blockIdx.x * QT + threadIdx.x; j <= M; j += (long long)gridDim.x * QT) {
        if (j == M) {
            cell_start[j] = N;
        } else {
            const int s = starts[j];
            cell_key[j] = sorted[s];
            cell_start[j] = s;
        }
    }
}

struct StatArgs {
    int n, n_tau;
    float tau2[D3R_CLOUD_MAX_THRESHOLDS];
    const float* query;                 // optional: n_valid counts the finite points; without it every query counts
    const float* d2;
    const int* idx;
};

// partial b = the sums of the queries b QT + thread + k gridDim QT: a fixed set in a fixed order, whatever the run
__global__ __launch_bounds__(QT) void cloud_stats_kernel(const StatArgs a, double* __restrict__ part_d, long long* __restrict__ part_i) {
    double sd[STAT_D] = {0.0, 0.0};
    long long si[STAT_I];
#pragma unroll
    for (int k = 0; k < STAT_I; ++k) si[k] = 0;
    for (long long q = (long long)blockIdx.x * QT + threadIdx.x; q < a.n; q += (long long)gridDim.x * QT) {
        bool valid = true;
        if (a.query) {
            valid = finite3(a.query + 3 * (size_t)q);
        }
        si[0] += valid;
        if (a.idx[q] < 0) continue;
        const float d2 = a.d2[q];
        si[1] += 1;
        sd[0] += __dsqrt_rn((double)d2);
        sd[1] += (double)d2;
#pragma unroll
        for (int j = 0; j < D3R_CLOUD_MAX_THRESHOLDS; ++j) si[2 + j] += (j < a.n_tau && d2 <= a.tau2[j]);
    }
    cloud_block_sum<STAT_D, STAT_I>(sd, si, part_d + (size_t)blockIdx.x * STAT_D, part_i + (size_t)blockIdx.x * STAT_I);
}

}  // namespace cloud
}  // namespace d3r

using namespace d3r::cloud;

extern "C" size_t d3r_cloud_grid_workspace_bytes(int n_ref, int n_query) {
    if (!fuse_shape_ok(1, n_ref, n_ref) || !fuse_shape_ok(1, n_query, n_query)) return 0;
    return cloud_workspace(nullptr, n_ref, n_query).bytes;
}

extern "C" int d3r_cloud_grid_build(int n_ref, const float* ref, const float* lo, float cell, const int* bits, void* workspace, void* stream) {
    if (!fuse_shape_ok(1, n_ref, n_ref) || !ref || !lo || !bits || !workspace || !cloud_cell_ok(cell)) return D3R_ERR_INVALID;
    FlagArgs a;
    int total_bits = 0;
    if (!fuse_key_params(lo, cell, bits, &a.key, &total_bits)) return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    // the layout in front of the query buffers does not depend on n_query
    const CloudWorkspace w = cloud_workspace(workspace, n_ref, 1);
    hipLaunchKernelGGL(cloud_shape_kernel, dim3(1), dim3(64), 0, st, w.shape, n_ref);
    a.pts = ref; a.mask = nullptr; a.weight = nullptr; a.img_h = w.shape; a.img_w = w.shape + 1;
    a.row = n_ref;
    const int cur = fuse_key_and_sort(a, w.ref, 1, n_ref, total_bits, st);
    const int* starts = fuse_segment_heads(a, w.ref, cur, n_ref, st);
    hipLaunchKernelGGL(cloud_gather_kernel, dim3(cloud_blocks(n_ref)), dim3(QT), 0, st, ref, w.ref.idx[cur], w.ref.n_dev, n_ref, w.pts4);
    hipLaunchKernelGGL(cloud_cells_kernel, dim3(cloud_blocks((long long)n_ref + 1)), dim3(QT), 0, st, w.ref.keys[cur], starts, w.ref.n_dev, n_ref, w.cell_key,
                       w.cell_start);
    return rc_of(hipGetLastError());
}

extern "C" size_t d3r_cloud_distance_stats_workspace_bytes(int n) {
    if (n <= 0) return 0;
    return cloud_sum_parts(nullptr, n, STAT_D, STAT_I).bytes;
}

extern "C" int d3r_cloud_distance_stats(int n, const float* query, const float* d2, const int* idx, int n_tau, const float* tau, long long* counts_out,
                                        double* sums_out, void* workspace, void* stream) {
    if (n <= 0 || !d2 || !idx || n_tau < 0 || n_tau > D3R_CLOUD_MAX_THRESHOLDS || (n_tau > 0 && !tau) || !counts_out || !sums_out || !workspace)
        return D3R_ERR_INVALID;
    StatArgs a;
    a.n = n; a.n_tau = n_tau; a.query = query; a.d2 = d2; a.idx = idx;
    for (int j = 0; j < D3R_CLOUD_MAX_THRESHOLDS; ++j) {
        if (j < n_tau && !(tau[j] >= 0.f && tau[j] <= 3.0e38f)) return D3R_ERR_INVALID;
        a.tau2[j] = j < n_tau ? tau[j] * tau[j] : 0.f;                 // host code of a file built without contraction: one fp32 product
    }
    hipStream_t st = (hipStream_t)stream;
    const SumParts p = cloud_sum_parts(workspace, n, STAT_D, STAT_I);
    hipLaunchKernelGGL(cloud_stats_kernel, dim3(p.parts), dim3(QT), 0, st, a, p.d, p.i);
    hipLaunchKernelGGL((cloud_sums_final_kernel<STAT_D, STAT_I>), dim3(1), dim3(QT), 0, st, p.parts, p.d, p.i, counts_out, sums_out);
    return rc_of(hipGetLastError());
}
