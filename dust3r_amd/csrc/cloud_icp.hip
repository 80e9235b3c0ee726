// dust3r_amd -- cloud registration (new; the reference has none): what one iteration of Sim(3) ICP does on the device besides the nearest
// neighbour search of cloud_knn.hip (dust3r_amd/cloud_metrics.py, register_clouds).
//   d3r_cloud_transform    cloud_transform_kernel            p' = A p + t per point, m = R n per normal, one thread per row
//   d3r_cloud_icp_sums     cloud_icp_sums_kernel<METRIC>     the gates of every row and the fp64 sums of the used rows: per-workgroup partials
//                          cloud_sums_final_kernel<18|36, 1> one workgroup adds the partials in index order (cloud_grid.hpp)
// METRIC 0 (point to point): the 17 moments of bootstrap.hip's layout and the squared residual, 18 sums. METRIC 1 (point to plane): the
// upper triangle of sum J J^T, sum J e and sum e e, 36 sums. One instance per metric: neither carries the other's accumulators.
// As in cloud_nn.hip: no atomics, no kernel waits on another workgroup, no scratch; partial b holds the rows b QT + thread + k gridDim QT,
// a fixed set in a fixed order, so every run gives the same bytes. Built without contraction: every product and sum below is one IEEE
// rounding, which is what the numpy restatement of tests/test_cloud_icp_cpu.py computes.
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "scene_common.hpp"
#include "fuse_grid.hpp"
#include "cloud_grid.hpp"

namespace d3r {
namespace cloud {

using namespace d3r::fuse;

constexpr int ICP_POINT = 18, ICP_PLANE = 36;
template <int METRIC> struct IcpSums { static constexpr int N = METRIC ? ICP_PLANE : ICP_POINT; };

struct TransformArgs {
    int n;
    float m[12], r[9];                  // [A | t] row-major; the rotation of the normals
    const float* pts;
    float* out;
    const float* normals_in;
    float* normals_out;
};

// out may be pts and normals_out may be normals_in: a thread reads its row before it writes it
__global__ __launch_bounds__(QT) void cloud_transform_kernel(const TransformArgs a) {
    for (long long i = (long long)blockIdx.x * QT + threadIdx.x; i < a.n; i += (long long)gridDim.x * QT) {
        const float* p = a.pts + 3 * (size_t)i;
        const float x = p[0], y = p[1], z = p[2];
        float* o = a.out + 3 * (size_t)i;
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = affine_row(a.m + 4 * r, x, y, z);
        if (a.normals_in) {
            const float* q = a.normals_in + 3 * (size_t)i;
            const float nx = q[0], ny = q[1], nz = q[2];
            float* m = a.normals_out + 3 * (size_t)i;
#pragma unroll
            for (int r = 0; r < 3; ++r) m[r] = row3(a.r + 3 * r, nx, ny, nz);
        }
    }
}

struct IcpArgs {
    int n, n_ref;
    const float* moved;
    const float* ref;
    const float* ref_normals;           // NULL for the point metric without the cosine gate
    const float* moved_normals;         // NULL: no cosine gate
    const float* d2;
    const int* idx;
    float gate2, cos_min;
    float centre[3];
    uint8_t* used_out;                  // optional
};

template <int METRIC>
__global__ __launch_bounds__(QT) void cloud_icp_sums_kernel(const IcpArgs a, double* __restrict__ part_d, long long* __restrict__ part_i) {
    constexpr int NS = IcpSums<METRIC>::N;
    double s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = 0.0;
    long long cnt[1] = {0};
    const double cx = (double)a.centre[0], cy = (double)a.centre[1], cz = (double)a.centre[2];
    for (long long i = (long long)blockIdx.x * QT + threadIdx.x; i < a.n; i += (long long)gridDim.x * QT) {
        const int g = a.idx[i];
        bool used = g >= 0 && g < a.n_ref && a.d2[i] <= a.gate2;
        const float* p = a.moved + 3 * (size_t)i;
        const float px = p[0], py = p[1], pz = p[2];
        used = used && finite3(px, py, pz);
        float qx = 0.f, qy = 0.f, qz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
        if (used) {
            const float* q = a.ref + 3 * (size_t)g;
            qx = q[0]; qy = q[1]; qz = q[2];
            used = finite3(qx, qy, qz);
        }
        if (used && (METRIC == 1 || a.moved_normals)) {
            const float* nr = a.ref_normals + 3 * (size_t)g;
            nx = nr[0]; ny = nr[1]; nz = nr[2];
            if (METRIC == 1) used = normal_ok(nx, ny, nz);
        }
        if (used && a.moved_normals) {
            const float* m = a.moved_normals + 3 * (size_t)i;
            used = row3(m, nx, ny, nz) >= a.cos_min;           // a NaN cosine fails
        }
        if (a.used_out) a.used_out[i] = used;
        if (!used) continue;
        cnt[0] += 1;
        const double ax = (double)px - cx, ay = (double)py - cy, az = (double)pz - cz;
        const double yx = (double)qx - cx, yy = (double)qy - cy, yz = (double)qz - cz;
        const double dx = ax - yx, dy = ay - yy, dz = az - yz;
        if (METRIC == 0) {
            const double x[3] = {ax, ay, az}, y[3] = {yx, yy, yz};
            s[0] += 1.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                s[1 + c] += x[c];
                s[4 + c] += y[c];
#pragma unroll
                for (int e = 0; e < 3; ++e) s[7 + 3 * c + e] += x[c] * y[e];
            }
            s[16] += (ax * ax + ay * ay) + az * az;
            s[17] += (dx * dx + dy * dy) + dz * dz;
        } else {
            const double ux = (double)nx, uy = (double)ny, uz = (double)nz;
            const double J[7] = {ay * uz - az * uy, az * ux - ax * uz, ax * uy - ay * ux, ux, uy, uz, (ax * ux + ay * uy) + az * uz};
            const double e = (ux * dx + uy * dy) + uz * dz;
            int k = 0;
#pragma unroll
            for (int r = 0; r < 7; ++r)
#pragma unroll
                for (int c = r; c < 7; ++c) s[k++] += J[r] * J[c];
#pragma unroll
            for (int r = 0; r < 7; ++r) s[28 + r] += J[r] * e;
            s[35] += e * e;
        }
    }
    cloud_block_sum<NS, 1>(s, cnt, part_d + (size_t)blockIdx.x * NS, part_i + blockIdx.x);
}

static inline bool all_finite(const float* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!(v[k] >= -3.4028234e38f && v[k] <= 3.4028234e38f)) return false;
    return true;
}

template <int METRIC>
static void icp_launch(const IcpArgs& a, long long* count_out, double* sums_out, void* workspace, hipStream_t st) {
    const SumParts p = cloud_sum_parts(workspace, a.n, ICP_PLANE, 1);        // as d3r_cloud_icp_sums_workspace_bytes, which does not know the metric
    hipLaunchKernelGGL(cloud_icp_sums_kernel<METRIC>, dim3(p.parts), dim3(QT), 0, st, a, p.d, p.i);
    hipLaunchKernelGGL((cloud_sums_final_kernel<IcpSums<METRIC>::N, 1>), dim3(1), dim3(QT), 0, st, p.parts, p.d, p.i, count_out, sums_out);
}

}  // namespace cloud
}  // namespace d3r

using namespace d3r::cloud;

extern "C" int d3r_cloud_transform(int n, const float* pts, const float* M, float* out, const float* normals_in, const float* R, float* normals_out,
                                   void* stream) {
    if (n <= 0 || !pts || !M || !out || !all_finite(M, 12)) return D3R_ERR_INVALID;
    if ((normals_in != nullptr) != (normals_out != nullptr) || (normals_in && (!R || !all_finite(R, 9)))) return D3R_ERR_INVALID;
    TransformArgs a;
    a.n = n; a.pts = pts; a.out = out; a.normals_in = normals_in; a.normals_out = normals_out;
    for (int k = 0; k < 12; ++k) a.m[k] = M[k];
    for (int k = 0; k < 9; ++k) a.r[k] = normals_in ? R[k] : 0.f;
    hipLaunchKernelGGL(cloud_transform_kernel, dim3(cloud_blocks(n)), dim3(QT), 0, (hipStream_t)stream, a);
    return rc_of(hipGetLastError());
}

extern "C" size_t d3r_cloud_icp_sums_workspace_bytes(int n) {
    if (n <= 0) return 0;
    return cloud_sum_parts(nullptr, n, ICP_PLANE, 1).bytes;
}

extern "C" int d3r_cloud_icp_sums(int n, const float* moved, const float* moved_normals, int n_ref, const float* ref, const float* ref_normals,
                                  const float* d2, const int* idx, int metric, float gate, float cos_min, const float* centre, long long* count_out,
                                  double* sums_out, uint8_t* used_out, void* workspace, void* stream) {
    if (n <= 0 || n_ref <= 0 || !moved || !ref || !d2 || !idx || !centre || !count_out || !sums_out || !workspace) return D3R_ERR_INVALID;
    if (metric != 0 && metric != 1) return D3R_ERR_INVALID;
    if ((metric == 1 || moved_normals) && !ref_normals) return D3R_ERR_INVALID;
    const float gate2 = gate * gate;                                    // host code of a file built without contraction: one fp32 product
    if (!(gate > 0.f && gate2 <= 3.4028234e38f) || !all_finite(centre, 3) || (moved_normals && !(cos_min == cos_min))) return D3R_ERR_INVALID;
    IcpArgs a;
    a.n = n; a.n_ref = n_ref; a.moved = moved; a.ref = ref; a.ref_normals = ref_normals; a.moved_normals = moved_normals; a.d2 = d2; a.idx = idx;
    a.gate2 = gate2; a.cos_min = cos_min; a.used_out = used_out;
    for (int c = 0; c < 3; ++c) a.centre[c] = centre[c];
    if (metric == 0) icp_launch<0>(a, count_out, sums_out, workspace, (hipStream_t)stream);
    else icp_launch<1>(a, count_out, sums_out, workspace, (hipStream_t)stream);
    return rc_of(hipGetLastError());
}
