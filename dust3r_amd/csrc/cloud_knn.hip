// dust3r_amd -- the search on the grid of d3r_cloud_grid_build (cloud_nn.hip, cloud_grid.hpp) for both of its entry points, the k nearest
// neighbours of every point of a cloud (d3r_cloud_knn) and the nearest one (d3r_cloud_nearest, the same search at k = 1), and
// the three kernels that consume them: mean neighbour distances (statistical outlier removal), normals, the orientation of the normals by
// the scene's cameras (new; the reference has none; dust3r_amd/cloud_metrics.py nearest_in_cloud / k_nearest, viz.FusedCloud.estimate_normals /
// remove_outliers). The contract does not mention the grid (include/dust3r_hip.h): the candidates of a valid query are the valid reference
// points with fp32 d2 <= r2 (the query's own index left out with exclude_self), and its row holds the k smallest (d2, index) pairs in
// lexicographic order, padded with (+inf, -1); the nearest neighbour, the lowest index among the points of minimal d2 when that minimum is
// <= r2, is the row of one column. The grid only limits which points are LOOKED AT, and the looked-at set holds every point with d2 <= r2
// ("Cloud metrics"): the walk itself is cloud_grid.hpp's cloud_walk, which the clustering runs too. A cell that holds most of
// the cloud is walked point by point by every query near it: slow, not wrong.
//   d3r_cloud_knn             cloud_knn_init_kernel      every row padded, or, with only_unresolved, the mask idx[q][k - 1] < 0 of the open rows
//   d3r_cloud_nearest         stages 1-2 of fuse_grid.hpp on the queries with the grid's own key: the queries in the order of their cells
//                             cloud_knn_kernel<1|8|16|32>   one thread per query, in that order: the lanes of a wave walk the same runs; the
//                                                        sorted list lives in registers
//   d3r_cloud_knn_distances   cloud_knn_mean_kernel / cloud_sums_final_kernel<2, 1>   the row means; per-workgroup partials, then one workgroup
//   d3r_cloud_normals         cloud_normals_kernel       fp64 scatter matrix of the point and its neighbours, cyclic Jacobi on named scalars
//   d3r_cloud_orient_normals  cloud_orient_kernel        one thread per point walks the views in order: projection in fp32, the vote in fp64
// As in fuse.hip and cloud_nn.hip: no atomics, no kernel waits on another workgroup, no scratch; the same bytes on every run. The list is
// never indexed by a runtime value: insertion is an unrolled compare-and-shift over all slots, so it stays in VGPRs (2 K of them: a slot
// is the 64-bit key (d2 bits, index), whose unsigned order is the pair's lexicographic order).
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "scene_common.hpp"
#include "fuse_grid.hpp"
#include "cloud_grid.hpp"

namespace d3r {
namespace cloud {

constexpr int JACOBI_SWEEPS = 8;        // cyclic Jacobi on 3 x 3 converges quadratically: 4-5 sweeps reach fp64 rounding, 8 leave a margin

// a fresh call: every row (+inf, -1). only_unresolved: the rows stay, mask[q] = the row is still short of k neighbours
__global__ __launch_bounds__(QT) void cloud_knn_init_kernel(int n, int k, int only_unresolved, float* __restrict__ d2_out, int* __restrict__ idx_out,
                                                           uint8_t* __restrict__ mask) {
    for (long long q = (long long)blockIdx.x * QT + threadIdx.x; q < n; q += (long long)gridDim.x * QT) {
        if (only_unresolved) {
            mask[q] = idx_out[(size_t)q * k + (k - 1)] < 0;
        } else {
            for (int j = 0; j < k; ++j) {
                d2_out[(size_t)q * k + j] = __builtin_huge_valf();
                idx_out[(size_t)q * k + j] = -1;
            }
        }
    }
}

struct KnnArgs {
    GridWalk grid;                      // the reference cloud's grid and the radius (cloud_grid.hpp)
    int k, exclude_self;
    const float* query;
    const int* order;                   // the valid (and open) queries in the order of their cells
    const int* n_query_dev;
    int cap_query;
    float* d2_out;                      // [n_query][k]
    int* idx_out;
    int* evals;                         // optional: += the distances this query evaluated
};

// K list slots, k <= K columns written. Slot K - 1 is the pruning bound.
template <int K>
__global__ __launch_bounds__(QT) void cloud_knn_kernel(const KnnArgs a) {
    const int M = count_of(a.grid.n_dev + 1, a.grid.cap);
    const int Nq = count_of(a.n_query_dev, a.cap_query);
    const float r2 = __fmul_rn(a.grid.r, a.grid.r);
    for (long long t = (long long)blockIdx.x * QT + threadIdx.x; t < Nq; t += (long long)gridDim.x * QT) {
        const int q = a.order[t];
        const float* p = a.query + 3 * (size_t)q;
        uint64_t list[K];
#pragma unroll
        for (int j = 0; j < K; ++j) list[j] = pair_key(__builtin_huge_valf(), NO_INDEX);
        const int self = a.exclude_self ? q : -1;
        const int evals = cloud_walk(a.grid, M, p[0], p[1], p[2], [&](int, float d2, const float4& v) {
            const int g = __float_as_int(v.w);
            const uint64_t cand = pair_key(d2, g);
            if (d2 <= r2 && g != self && cand < list[K - 1]) {
                // slot j takes its left neighbour when the candidate sorts before that one, else the candidate when it sorts before slot j
                // itself; from the right, so every read sees the old list. Static indices only.
#pragma unroll
                for (int j = K - 1; j > 0; --j) list[j] = cand < list[j - 1] ? list[j - 1] : (cand < list[j] ? cand : list[j]);
                list[0] = cand < list[0] ? cand : list[0];
            }
        });
        float* d2_row = a.d2_out + (size_t)q * a.k;
        int* idx_row = a.idx_out + (size_t)q * a.k;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (j < a.k) {
                const int g = (int)(uint32_t)list[j];
                const bool found = g != NO_INDEX;
                d2_row[j] = found ? __uint_as_float((uint32_t)(list[j] >> 32)) : __builtin_huge_valf();
                idx_row[j] = found ? g : -1;
            }
        }
        if (a.evals) a.evals[q] += evals;
    }
}

// ---- mean neighbour distance ------------------------------------------------------------------------------------------------------------
constexpr int MEAN_D = 2, MEAN_I = 1;

// mean_out[q], and partial b = the sums over the full rows q = b QT + thread + j gridDim QT: a fixed set in a fixed order, whatever the run
__global__ __launch_bounds__(QT) void cloud_knn_mean_kernel(int n, int k, const float* __restrict__ d2, const int* __restrict__ idx, float* __restrict__ mean_out,
                                                           double* __restrict__ part_d, long long* __restrict__ part_i) {
    double sd[MEAN_D] = {0.0, 0.0};
    long long si[MEAN_I] = {0};
    for (long long q = (long long)blockIdx.x * QT + threadIdx.x; q < n; q += (long long)gridDim.x * QT) {
        double s = 0.0;
        int found = 0;
        for (int j = 0; j < k; ++j) {
            if (idx[(size_t)q * k + j] < 0) continue;
            s += __dsqrt_rn((double)d2[(size_t)q * k + j]);
            ++found;
        }
        const bool full = found == k;
        const float mean = full ? (float)__ddiv_rn(s, (double)found) : __builtin_nanf("");
        mean_out[q] = mean;
        if (full) {
            const double m = (double)mean;
            si[0] += 1;
            sd[0] += m;
            sd[1] += __dmul_rn(m, m);
        }
    }
    cloud_block_sum<MEAN_D, MEAN_I>(sd, si, part_d + (size_t)blockIdx.x * MEAN_D, part_i + (size_t)blockIdx.x * MEAN_I);
}

// ---- normals ----------------------------------------------------------------------------------------------------------------------------
// one Jacobi rotation in the (p, q) plane of the symmetric matrix: app, aqq the diagonal, apq the entry it annihilates, apr / aqr the two
// entries of the third index r; v?p / v?q the columns p and q of the accumulated eigenvectors. Named scalars: nothing is indexed.
D3R_DEV void jacobi_rotate(double& app, double& aqq, double& apq, double& apr, double& aqr, double& v0p, double& v0q, double& v1p, double& v1q, double& v2p,
                           double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + __dsqrt_rn(theta * theta + 1.0));       // |theta| huge: t -> 0
    const double c = 1.0 / __dsqrt_rn(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double npr = c * apr - s * aqr, nqr = s * apr + c * aqr;
    apr = npr;
    aqr = nqr;
    const double n0p = c * v0p - s * v0q, n0q = s * v0p + c * v0q;
    const double n1p = c * v1p - s * v1q, n1q = s * v1p + c * v1q;
    const double n2p = c * v2p - s * v2q, n2q = s * v2p + c * v2q;
    v0p = n0p; v0q = n0q; v1p = n1p; v1q = n1q; v2p = n2p; v2q = n2q;
}

struct NormalArgs {
    int n, n_ref, k, min_neighbors;
    const float* points;                // [n][3]
    const float* ref;                   // [n_ref][3]: what idx points into
    const int* idx;                     // [n][k]
    float* normals;                     // [n][3]
    float* curvature;                   // [n]
};

__global__ __launch_bounds__(QT) void cloud_normals_kernel(const NormalArgs a) {
    for (long long q = (long long)blockIdx.x * QT + threadIdx.x; q < a.n; q += (long long)gridDim.x * QT) {
        const float* p = a.points + 3 * (size_t)q;
        const int* row = a.idx + (size_t)q * a.k;
        // the mean of the sample: the point, then its found neighbours in column order
        double mx = (double)p[0], my = (double)p[1], mz = (double)p[2];
        int found = 0;
        for (int j = 0; j < a.k; ++j) {
            const int g = row[j];
            if (g < 0 || g >= a.n_ref) continue;
            const float* v = a.ref + 3 * (size_t)g;
            mx += (double)v[0]; my += (double)v[1]; mz += (double)v[2];
            ++found;
        }
        float nx = 0.f, ny = 0.f, nz = 0.f, curv = __builtin_nanf("");
        if (found >= a.min_neighbors) {
            const double m = (double)(found + 1);
            mx /= m; my /= m; mz /= m;
            double dx = (double)p[0] - mx, dy = (double)p[1] - my, dz = (double)p[2] - mz;
            double a00 = dx * dx, a01 = dx * dy, a02 = dx * dz, a11 = dy * dy, a12 = dy * dz, a22 = dz * dz;
            for (int j = 0; j < a.k; ++j) {
                const int g = row[j];
                if (g < 0 || g >= a.n_ref) continue;
                const float* v = a.ref + 3 * (size_t)g;
                dx = (double)v[0] - mx; dy = (double)v[1] - my; dz = (double)v[2] - mz;
                a00 += dx * dx; a01 += dx * dy; a02 += dx * dz; a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
            }
            double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
            for (int s = 0; s < JACOBI_SWEEPS; ++s) {
                jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
                jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
                jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
            }
            // the smallest eigenvalue's column; of equal ones the first
            const bool c1 = a11 < a00 && a11 <= a22, c2 = a22 < a00 && a22 < a11;
            const double l0 = c2 ? a22 : (c1 ? a11 : a00);
            double ex = c2 ? v02 : (c1 ? v01 : v00), ey = c2 ? v12 : (c1 ? v11 : v10), ez = c2 ? v22 : (c1 ? v21 : v20);
            const double len = __dsqrt_rn(ex * ex + ey * ey + ez * ez);
            ex /= len; ey /= len; ez /= len;
            // the sign: the first component of largest magnitude is positive
            const double fx = fabs(ex), fy = fabs(ey), fz = fabs(ez);
            const double lead = (fx >= fy && fx >= fz) ? ex : (fy >= fz ? ey : ez);
            if (lead < 0.0) { ex = -ex; ey = -ey; ez = -ez; }
            nx = (float)ex; ny = (float)ey; nz = (float)ez;
            curv = (float)(l0 / (a00 + a11 + a22));
        }
        a.normals[3 * (size_t)q] = nx;
        a.normals[3 * (size_t)q + 1] = ny;
        a.normals[3 * (size_t)q + 2] = nz;
        a.curvature[q] = curv;
    }
}

// ---- orientation ------------------------------------------------------------------------------------------------------------------------
struct OrientArgs {
    int n, n_views, max_area;
    float tol;
    const float* points;                // [n][3]
    float* normals;                     // [n][3], in place
    int* n_seen;                        // [n]
    const float* depth;                 // [n_views][max_area]
    const float* conf;                  // [n_views][max_area]
    const float* K;                     // [n_views][9]
    const float* w2c;                   // [n_views][16]
    const float* centers;               // [n_views][3]
    const int *Hs, *Ws;
};

__global__ __launch_bounds__(QT) void cloud_orient_kernel(const OrientArgs a) {
    for (long long q = (long long)blockIdx.x * QT + threadIdx.x; q < a.n; q += (long long)gridDim.x * QT) {
        const float* X = a.points + 3 * (size_t)q;
        const float x = X[0], y = X[1], z = X[2];
        float* N = a.normals + 3 * (size_t)q;
        const double nx = (double)N[0], ny = (double)N[1], nz = (double)N[2];
        double s_seen = 0.0, s_all = 0.0;
        int seen = 0;
        for (int v = 0; v < a.n_views; ++v) {
            const float* C = a.centers + 3 * v;
            const double dx = (double)C[0] - (double)x, dy = (double)C[1] - (double)y, dz = (double)C[2] - (double)z;
            const double len = __dsqrt_rn(dx * dx + dy * dy + dz * dz);
            const double cosine = len > 0.0 ? (nx * dx + ny * dy + nz * dz) / len : 0.0;      // a point at the centre has no direction: no vote
            s_all += cosine;
            const float* M = a.w2c + 16 * v;
            // rows of the 3 x 4 / 3 x 3 products as clean_pointcloud_kernel writes them, left to right (fuse_grid.hpp)
            const float px = affine_row(M, x, y, z), py = affine_row(M + 4, x, y, z), pz = affine_row(M + 8, x, y, z);
            if (!(pz > 0.f)) continue;
            const float* Kv = a.K + 9 * v;
            const float ku = row3(Kv, px, py, pz), kv = row3(Kv + 3, px, py, pz), kw = row3(Kv + 6, px, py, pz);
            const float uu = rintf(__fdiv_rn(ku, kw)), vv = rintf(__fdiv_rn(kv, kw));        // half to even, as torch.round
            const int Wv = a.Ws[v], Hv = a.Hs[v];
            if (!(uu >= 0.f && uu < (float)Wv && vv >= 0.f && vv < (float)Hv)) continue;
            const long long pix = (long long)(int)vv * Wv + (int)uu;
            if (pix >= a.max_area) continue;                               // a table that does not fit its stack: nothing is read behind a row
            const size_t e = (size_t)v * a.max_area + (size_t)pix;
            const float d = a.depth[e];
            if (!(fabsf(__fsub_rn(pz, d)) <= __fmul_rn(a.tol, d))) continue;
            ++seen;
            s_seen += (double)a.conf[e] * cosine;
        }
        const double s = seen > 0 ? s_seen : s_all;
        if (s < 0.0) {
            N[0] = -N[0]; N[1] = -N[1]; N[2] = -N[2];
        }
        a.n_seen[q] = seen;
    }
}

}  // namespace cloud
}  // namespace d3r

using namespace d3r::cloud;

extern "C" int d3r_cloud_knn(int n_ref, int n_query, const float* query, int k, float r, const float* lo, float cell, const int* bits, int exclude_self,
                             int only_unresolved, float* d2_out, int* idx_out, int* evals, void* workspace, void* stream) {
    if (!fuse_shape_ok(1, n_ref, n_ref) || !fuse_shape_ok(1, n_query, n_query) || !query || !lo || !bits || !d2_out || !idx_out || !workspace ||
        !cloud_radius_ok(r) || !cloud_cell_ok(cell) || k < 1 || k > D3R_CLOUD_MAX_K)
        return D3R_ERR_INVALID;
    KnnArgs qa;
    FlagArgs a;
    int total_bits = 0;
    if (!fuse_key_params(lo, cell, bits, &a.key, &total_bits)) return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const CloudWorkspace w = cloud_workspace(workspace, n_ref, n_query);
    hipLaunchKernelGGL(cloud_knn_init_kernel, dim3(cloud_blocks(n_query)), dim3(QT), 0, st, n_query, k, only_unresolved, d2_out, idx_out, w.mask);
    hipLaunchKernelGGL(cloud_shape_kernel, dim3(1), dim3(64), 0, st, w.shape + 2, n_query);
    a.pts = query; a.mask = only_unresolved ? w.mask : nullptr; a.weight = nullptr; a.img_h = w.shape + 2; a.img_w = w.shape + 3;
    a.row = n_query;
    const int cur = fuse_key_and_sort(a, w.qry, 1, n_query, total_bits, st);
    qa.grid.key = a.key; qa.grid.r = r; qa.k = k; qa.exclude_self = exclude_self != 0;
    qa.grid.pts4 = w.pts4; qa.grid.cell_key = w.cell_key; qa.grid.cell_start = w.cell_start; qa.grid.n_dev = w.ref.n_dev; qa.grid.cap = n_ref;
    qa.query = query; qa.order = w.qry.idx[cur]; qa.n_query_dev = w.qry.n_dev; qa.cap_query = n_query;
    qa.d2_out = d2_out; qa.idx_out = idx_out; qa.evals = evals;
    const dim3 grid(cloud_blocks(n_query)), block(QT);
    if (k == 1) hipLaunchKernelGGL(cloud_knn_kernel<1>, grid, block, 0, st, qa);
    else if (k <= 8) hipLaunchKernelGGL(cloud_knn_kernel<8>, grid, block, 0, st, qa);
    else if (k <= 16) hipLaunchKernelGGL(cloud_knn_kernel<16>, grid, block, 0, st, qa);
    else hipLaunchKernelGGL(cloud_knn_kernel<32>, grid, block, 0, st, qa);
    return rc_of(hipGetLastError());
}

// the first column of the search at k = 1: the smallest (d2, index) pair among those with d2 <= r2; outputs (n,) are rows of one column
extern "C" int d3r_cloud_nearest(int n_ref, int n_query, const float* query, float r, const float* lo, float cell, const int* bits, int only_unresolved,
                                 float* d2_out, int* idx_out, int* evals, void* workspace, void* stream) {
    return d3r_cloud_knn(n_ref, n_query, query, 1, r, lo, cell, bits, 0, only_unresolved, d2_out, idx_out, evals, workspace, stream);
}

extern "C" size_t d3r_cloud_knn_distances_workspace_bytes(int n) {
    if (n <= 0) return 0;
    return cloud_sum_parts(nullptr, n, MEAN_D, MEAN_I).bytes;
}

extern "C" int d3r_cloud_knn_distances(int n, int k, const float* d2, const int* idx, float* mean_out, long long* count_out, double* sums_out,
                                       void* workspace, void* stream) {
    if (n <= 0 || k < 1 || k > D3R_CLOUD_MAX_K || !d2 || !idx || !mean_out || !count_out || !sums_out || !workspace) return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const SumParts p = cloud_sum_parts(workspace, n, MEAN_D, MEAN_I);
    hipLaunchKernelGGL(cloud_knn_mean_kernel, dim3(p.parts), dim3(QT), 0, st, n, k, d2, idx, mean_out, p.d, p.i);
    hipLaunchKernelGGL((cloud_sums_final_kernel<MEAN_D, MEAN_I>), dim3(1), dim3(QT), 0, st, p.parts, p.d, p.i, count_out, sums_out);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_cloud_normals(int n, const float* points, int n_ref, const float* ref, int k, const int* idx, int min_neighbors, float* normals_out,
                                 float* curvature_out, void* stream) {
    if (n <= 0 || n_ref <= 0 || k < 1 || k > D3R_CLOUD_MAX_K || !points || !ref || !idx || min_neighbors < 2 || !normals_out || !curvature_out)
        return D3R_ERR_INVALID;
    NormalArgs a;
    a.n = n; a.n_ref = n_ref; a.k = k; a.min_neighbors = min_neighbors;
    a.points = points; a.ref = ref; a.idx = idx; a.normals = normals_out; a.curvature = curvature_out;
    hipLaunchKernelGGL(cloud_normals_kernel, dim3(cloud_blocks(n)), dim3(QT), 0, (hipStream_t)stream, a);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_cloud_orient_normals(int n, const float* points, float* normals, int* n_seen, int n_views, const float* depth, const float* conf,
                                        const float* intrinsics, const float* world2cam, const float* centers, const int* img_h_dev,
                                        const int* img_w_dev, int max_area, float tol, void* stream) {
    if (n <= 0 || !points || !normals || !n_seen || n_views <= 0 || n_views > 65535 || !depth || !conf || !intrinsics || !world2cam || !centers ||
        !img_h_dev || !img_w_dev || max_area <= 0 || !(tol >= 0.f && tol < 1.f))
        return D3R_ERR_INVALID;
    OrientArgs a;
    a.n = n; a.n_views = n_views; a.max_area = max_area; a.tol = tol;
    a.points = points; a.normals = normals; a.n_seen = n_seen; a.depth = depth; a.conf = conf; a.K = intrinsics; a.w2c = world2cam;
    a.centers = centers; a.Hs = img_h_dev; a.Ws = img_w_dev;
    hipLaunchKernelGGL(cloud_orient_kernel, dim3(cloud_blocks(n)), dim3(QT), 0, (hipStream_t)stream, a);
    return rc_of(hipGetLastError());
}
