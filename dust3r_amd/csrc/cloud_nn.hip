// dust3r_amd -- cloud-to-cloud metrics (new; the reference has none): the truncated exact nearest neighbour of every point of a query
// cloud in a reference cloud, on a uniform grid, and the reduction of the distances to the sums and counts of accuracy / completeness /
// precision / recall (dust3r_amd/cloud_metrics.py). The contract does not mention the grid (include/dust3r_hip.h): for a valid query the
// lowest index among the valid reference points of minimal fp32 d2, when that minimum is <= r2 = r r; else -1 and +inf. The grid only
// limits which reference points are LOOKED AT, and the looked-at set always holds every point with d2 <= r2 ("Cloud metrics").
//   d3r_cloud_grid_build     cloud_shape_kernel   the flat cloud as one view of 1 x n (the tables stages 1-3 read)
//                            stages 1-3 of fuse_grid.hpp on the reference cloud: (key, index) of the valid points, sorted, the cell heads
//                            cloud_gather_kernel  the points in sorted order as float4 (x, y, z, original index), so a cell is one run
//                            cloud_cells_kernel   the key and the first point of every cell; one more start = N behind the last
//   d3r_cloud_nearest        cloud_init_kernel    (-1, +inf) everywhere, or, with only_unresolved, the mask idx < 0 of what is still open
//                            stages 1-2 on the queries with the grid's own key: the queries in the order of their cells
//                            cloud_query_kernel   one thread per query, in that order: the lanes of a wave walk the same runs
//   d3r_cloud_distance_stats cloud_stats_kernel / cloud_stats_final_kernel   per-workgroup partials, then one workgroup in index order
// As in fuse.hip: no atomics, no kernel waits on another workgroup, no scratch; the same bytes on every run. A cell that holds most of
// the cloud is walked point by point by every query near it: slow, not wrong. The workspace layout, the checks of cell and radius and the
// padded cell range's arithmetic are in cloud_grid.hpp, shared with cloud_knn.hip (the k nearest neighbours on the same grid).
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "scene_common.hpp"
#include "fuse_grid.hpp"
#include "cloud_grid.hpp"

namespace d3r {
namespace cloud {

using namespace d3r::fuse;

constexpr int STAT_BLOCKS = 1024;       // grid cap of the statistics pass = the partials of the final pass
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

// a fresh call: every query (-1, +inf). only_unresolved: the results stay, mask[q] = the query is still open
__global__ __launch_bounds__(QT) void cloud_init_kernel(int n, int only_unresolved, float* __restrict__ d2_out, int* __restrict__ idx_out,
                                                       uint8_t* __restrict__ mask) {
    for (long long q = (long long)blockIdx.x * QT + threadIdx.x; q < n; q += (long long)gridDim.x * QT) {
        if (only_unresolved) {
            mask[q] = idx_out[q] < 0;
        } else {
            d2_out[q] = __builtin_huge_valf();
            idx_out[q] = -1;
        }
    }
}

struct QueryArgs {
    KeyParams key;
    float r;
    const float4* pts4;                 // the grid
    const uint64_t* cell_key;
    const int* cell_start;
    const int* n_ref_dev;               // [2]: the valid reference points N, the cells M
    int cap_ref;
    const float* query;
    const int* order;                   // the valid (and open) queries in the order of their cells
    const int* n_query_dev;
    int cap_query;
    float* d2_out;
    int* idx_out;
    int* evals;                         // optional: += the distances this query evaluated
};

__global__ __launch_bounds__(QT) void cloud_query_kernel(const QueryArgs a) {
    const int M = count_of(a.n_ref_dev + 1, a.cap_ref);
    const int Nq = count_of(a.n_query_dev, a.cap_query);
    const float r2 = __fmul_rn(a.r, a.r);
    const float rp = __fmul_rn(a.r, 1.0009765625f);                     // r (1 + 2^-10)
    for (long long t = (long long)blockIdx.x * QT + threadIdx.x; t < Nq; t += (long long)gridDim.x * QT) {
        const int q = a.order[t];
        const float* p = a.query + 3 * (size_t)q;
        const float ax = p[0], ay = p[1], az = p[2];
        const float pa[3] = {ax, ay, az};
        int c0[3], c1[3];
        bool outside = false;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float lo = next_down(__fsub_rn(pa[c], rp)), hi = next_up(__fadd_rn(pa[c], rp));
            // every reference point has 0 <= floorf(.) <= qmax (lo = the bounds' minimum, bits from their extent) and floorf(.) is monotone:
            // an interval that ends below cell 0 or starts above the last cell holds none
            outside = outside || axis_f(hi, a.key, c) < 0.f || axis_f(lo, a.key, c) > (float)a.key.qmax[c];
            c0[c] = axis_q(lo, a.key, c);
            c1[c] = axis_q(hi, a.key, c);
        }
        float best = __builtin_huge_valf();
        int best_i = 0x7FFFFFFF, evals = 0;
        if (!outside) {
            int from = 0;                                                  // the rows come in ascending key order: each search starts where the last ended
            for (int z = c0[2]; z <= c1[2]; ++z) {
                for (int y = c0[1]; y <= c1[1]; ++y) {
                    const uint64_t row = ((uint64_t)y << a.key.shift[1]) | ((uint64_t)z << a.key.shift[2]);
                    const uint64_t k_lo = row | (uint64_t)c0[0], k_hi = row | (uint64_t)c1[0];
                    int l = from, h = M;                                   // the first cell with key >= k_lo
                    while (l < h) {
                        const int m = l + ((h - l) >> 1);
                        if (a.cell_key[m] < k_lo) l = m + 1; else h = m;
                    }
                    int j = l;
                    while (j < M && a.cell_key[j] <= k_hi) ++j;           // at most c1 - c0 + 1 cells: one run of points
                    from = j;
                    if (j == l) continue;
                    const int s = a.cell_start[l], e = a.cell_start[j];
                    for (int i = s; i < e; ++i) {
                        const float4 v = a.pts4[i];
                        const float dx = __fsub_rn(ax, v.x), dy = __fsub_rn(ay, v.y), dz = __fsub_rn(az, v.z);
                        const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                        const int g = __float_as_int(v.w);
                        if (d2 < best || (d2 == best && g < best_i)) {
                            best = d2;
                            best_i = g;
                        }
                    }
                    evals += e - s;
                }
            }
        }
        const bool found = best <= r2;
        a.d2_out[q] = found ? best : __builtin_huge_valf();
        a.idx_out[q] = found ? best_i : -1;
        if (a.evals) a.evals[q] += evals;
    }
}

struct StatArgs {
    int n, n_tau;
    float tau2[D3R_CLOUD_MAX_THRESHOLDS];
    const float* query;                 // optional: n_valid counts the finite points; without it every query counts
    const float* d2;
    const int* idx;
};

// the wave's sums by butterflies, then thread 0 over the waves in order: the workgroup's totals, valid in thread 0
template <int THREADS>
D3R_DEV void stats_block_sum(double (&sd)[STAT_D], long long (&si)[STAT_I], double* lds_d, long long* lds_i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < STAT_D; ++k) sd[k] += __shfl_xor(sd[k], o);
#pragma unroll
        for (int k = 0; k < STAT_I; ++k) si[k] += __shfl_xor(si[k], o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < STAT_D; ++k) lds_d[wave * STAT_D + k] = sd[k];
#pragma unroll
        for (int k = 0; k < STAT_I; ++k) lds_i[wave * STAT_I + k] = si[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < THREADS / 64; ++w) {
#pragma unroll
            for (int k = 0; k < STAT_D; ++k) sd[k] += lds_d[w * STAT_D + k];
#pragma unroll
            for (int k = 0; k < STAT_I; ++k) si[k] += lds_i[w * STAT_I + k];
        }
    }
}

// partial b = the sums of the queries b QT + thread + k gridDim QT: a fixed set in a fixed order, whatever the run
__global__ __launch_bounds__(QT) void cloud_stats_kernel(const StatArgs a, double* __restrict__ part_d, long long* __restrict__ part_i) {
    __shared__ double lds_d[QT / 64 * STAT_D];
    __shared__ long long lds_i[QT / 64 * STAT_I];
    double sd[STAT_D] = {0.0, 0.0};
    long long si[STAT_I];
#pragma unroll
    for (int k = 0; k < STAT_I; ++k) si[k] = 0;
    for (long long q = (long long)blockIdx.x * QT + threadIdx.x; q < a.n; q += (long long)gridDim.x * QT) {
        bool valid = true;
        if (a.query) {
            const float* p = a.query + 3 * (size_t)q;
            valid = finite_f(p[0]) && finite_f(p[1]) && finite_f(p[2]);
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
    stats_block_sum<QT>(sd, si, lds_d, lds_i);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < STAT_D; ++k) part_d[(size_t)blockIdx.x * STAT_D + k] = sd[k];
#pragma unroll
        for (int k = 0; k < STAT_I; ++k) part_i[(size_t)blockIdx.x * STAT_I + k] = si[k];
    }
}

__global__ __launch_bounds__(QT) void cloud_stats_final_kernel(int n_parts, const double* __restrict__ part_d, const long long* __restrict__ part_i,
                                                              long long* __restrict__ counts_out, double* __restrict__ sums_out) {
    __shared__ double lds_d[QT / 64 * STAT_D];
    __shared__ long long lds_i[QT / 64 * STAT_I];
    double sd[STAT_D] = {0.0, 0.0};
    long long si[STAT_I];
#pragma unroll
    for (int k = 0; k < STAT_I; ++k) si[k] = 0;
    for (int b = threadIdx.x; b < n_parts; b += QT) {
#pragma unroll
        for (int k = 0; k < STAT_D; ++k) sd[k] += part_d[(size_t)b * STAT_D + k];
#pragma unroll
        for (int k = 0; k < STAT_I; ++k) si[k] += part_i[(size_t)b * STAT_I + k];
    }
    stats_block_sum<QT>(sd, si, lds_d, lds_i);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < STAT_I; ++k) counts_out[k] = si[k];
#pragma unroll
        for (int k = 0; k < STAT_D; ++k) sums_out[k] = sd[k];
    }
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

extern "C" int d3r_cloud_nearest(int n_ref, int n_query, const float* query, float r, const float* lo, float cell, const int* bits, int only_unresolved,
                                 float* d2_out, int* idx_out, int* evals, void* workspace, void* stream) {
    if (!fuse_shape_ok(1, n_ref, n_ref) || !fuse_shape_ok(1, n_query, n_query) || !query || !lo || !bits || !d2_out || !idx_out || !workspace ||
        !cloud_radius_ok(r) || !cloud_cell_ok(cell))
        return D3R_ERR_INVALID;
    QueryArgs qa;
    FlagArgs a;
    int total_bits = 0;
    if (!fuse_key_params(lo, cell, bits, &a.key, &total_bits)) return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const CloudWorkspace w = cloud_workspace(workspace, n_ref, n_query);
    hipLaunchKernelGGL(cloud_init_kernel, dim3(cloud_blocks(n_query)), dim3(QT), 0, st, n_query, only_unresolved, d2_out, idx_out, w.mask);
    hipLaunchKernelGGL(cloud_shape_kernel, dim3(1), dim3(64), 0, st, w.shape + 2, n_query);
    a.pts = query; a.mask = only_unresolved ? w.mask : nullptr; a.weight = nullptr; a.img_h = w.shape + 2; a.img_w = w.shape + 3;
    a.row = n_query;
    const int cur = fuse_key_and_sort(a, w.qry, 1, n_query, total_bits, st);
    qa.key = a.key; qa.r = r;
    qa.pts4 = w.pts4; qa.cell_key = w.cell_key; qa.cell_start = w.cell_start; qa.n_ref_dev = w.ref.n_dev; qa.cap_ref = n_ref;
    qa.query = query; qa.order = w.qry.idx[cur]; qa.n_query_dev = w.qry.n_dev; qa.cap_query = n_query;
    qa.d2_out = d2_out; qa.idx_out = idx_out; qa.evals = evals;
    hipLaunchKernelGGL(cloud_query_kernel, dim3(cloud_blocks(n_query)), dim3(QT), 0, st, qa);
    return rc_of(hipGetLastError());
}

extern "C" size_t d3r_cloud_distance_stats_workspace_bytes(int n) {
    if (n <= 0) return 0;
    const size_t parts = (size_t)std::min(cloud_blocks(n), STAT_BLOCKS);
    return align256(parts * STAT_D * sizeof(double)) + align256(parts * STAT_I * sizeof(long long));
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
    const int parts = std::min(cloud_blocks(n), STAT_BLOCKS);
    double* part_d = (double*)workspace;
    long long* part_i = (long long*)((char*)workspace + align256((size_t)parts * STAT_D * sizeof(double)));
    hipLaunchKernelGGL(cloud_stats_kernel, dim3(parts), dim3(QT), 0, st, a, part_d, part_i);
    hipLaunchKernelGGL(cloud_stats_final_kernel, dim3(1), dim3(QT), 0, st, parts, part_d, part_i, counts_out, sums_out);
    return rc_of(hipGetLastError());
}
