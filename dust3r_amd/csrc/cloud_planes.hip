// dust3r_amd -- plane detection on a cloud (new; the reference has none): the device stages of dust3r_amd/cloud_metrics.py, plane_ransac,
// segment_plane and detect_planes. Both entry points are DEFINED in include/dust3r_hip.h without reference to how they are
// computed; tests/test_cloud_planes_cpu.py restates them in numpy.
//   d3r_plane_ransac       plane_hyp_kernel           one thread per hypothesis: counter-based sample of 3 points (ransac.hpp), fp64 plane
//                          plane_score_kernel<NRM>    grid (point chunk, round of RND hypotheses): ransac.hpp's round scorer: THE HOT KERNEL
//                          plane_select_kernel        one workgroup: the largest count, then the lowest hypothesis (ransac.hpp's selection)
//                          plane_mask_kernel          the winner's inlier mask (ransac.hpp's loop)
//   d3r_plane_support      plane_support_kernel       the inlier test of a given plane and the fp64 moments of its inliers: per-workgroup partials
//                          cloud_sums_final_kernel<9, 1>  one workgroup adds the partials in index order (cloud_grid.hpp)
// No floating-point atomics, no kernel waits on another workgroup, no scratch. The only atomics are integer additions of inlier counts
// (plane_score_kernel), whose result does not depend on their order: the same bytes on every run. Built without contraction: every
// product and sum below is one IEEE rounding, which is what the numpy restatements compute; the fp32 3-vector arithmetic is fuse_grid.hpp's.
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "scene_common.hpp"
#include "fuse_grid.hpp"
#include "cloud_grid.hpp"
#include "ransac.hpp"

namespace d3r {
namespace cloud {

using namespace d3r::fuse;

constexpr int RND = 256;                // hypotheses of a round = the rows a scoring workgroup holds in LDS
// scoring: threads, points per lane, points per workgroup. A lane keeps 8 points (24 VGPRs, 48 with normals): a round's row costs one
// 16-byte LDS broadcast per wave and hypothesis, paid once for 512 plane tests
constexpr int SPT = 256, SPL = 8, SCHUNK = SPT * SPL;
constexpr int MAX_HYP = D3R_SIM3_MAX_HYPOTHESES;      // the rounds are the second grid dimension of the scoring kernel
constexpr int MOMENTS = 9;              // sum a [3], the upper triangle of sum a a^T [6]

struct PlaneBest {
    int h, count, n_valid, pad;
    float row[4];
};

struct PlaneWs {
    double* planes;         // [n_hyp][4]
    float* rows;            // [n_hyp][12]: float32(n, d), then zeros
    int* valid;             // [n_hyp]
    int* counts;            // [n_hyp]
    PlaneBest* best;
    size_t bytes;
};

static inline PlaneWs plane_workspace(void* base, int n_hyp) {
    PlaneWs w;
    Carver c(base);
    w.planes = c.take<double>((size_t)n_hyp * 4);
    w.rows = c.take<float>((size_t)n_hyp * 12);
    w.valid = c.take<int>(n_hyp);
    w.counts = c.take<int>(n_hyp);
    w.best = c.take<PlaneBest>(1);
    w.bytes = c.bytes;
    return w;
}

struct PlaneArgs {
    int n, n_hyp, min_inliers;
    uint64_t seed;
    float thr, cos_min;
    double min_area2;
    const float* pts;
    const float* normals;               // NULL: no condition on the normals
};

D3R_DEV bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }       // false for a NaN

__global__ __launch_bounds__(RND) void plane_hyp_kernel(const PlaneArgs a, const PlaneWs w) {
    const int h = blockIdx.x * RND + threadIdx.x;
    if (h >= a.n_hyp) return;
    w.counts[h] = 0;
    int i[3];
    bool ok = ransac::draw_distinct(a.seed, h, a.n, i);
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    if (ok) {
        float P[3][3];
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int c = 0; c < 3; ++c) P[s][c] = a.pts[(size_t)i[s] * 3 + c];
        ok = finite3(P[0][0], P[0][1], P[0][2]) && finite3(P[1][0], P[1][1], P[1][2]) && finite3(P[2][0], P[2][1], P[2][2]);
        const double p0x = (double)P[0][0], p0y = (double)P[0][1], p0z = (double)P[0][2];
        const double ux = (double)P[1][0] - p0x, uy = (double)P[1][1] - p0y, uz = (double)P[1][2] - p0z;
        const double vx = (double)P[2][0] - p0x, vy = (double)P[2][1] - p0y, vz = (double)P[2][2] - p0z;
        const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        const double l = sqrt((cx * cx + cy * cy) + cz * cz);
        ok = ok && l >= a.min_area2;                                      // false for a NaN; min_area2 > 0, so l > 0
        m[0] = cx / l; m[1] = cy / l; m[2] = cz / l;
        m[3] = -((m[0] * p0x + m[1] * p0y) + m[2] * p0z);
        ok = ok && finite_d(m[0]) && finite_d(m[1]) && finite_d(m[2]) && finite_d(m[3]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) w.planes[(size_t)h * 4 + c] = ok ? m[c] : 0.0;
#pragma unroll
    for (int c = 0; c < 12; ++c) w.rows[(size_t)h * 12 + c] = ok && c < 4 ? (float)m[c] : 0.f;
    w.valid[h] = ok ? 1 : 0;
}

// |e| <= thr, e = ((nx x + ny y) + nz z) + d: false for a NaN, so for a point whose x was replaced by a NaN
D3R_DEV bool plane_near(const float* m, float x, float y, float z, float thr) { return fabsf(affine_row(m, x, y, z)) <= thr; }
// |n . m| >= cos_min: sign-free, false for a NaN
D3R_DEV bool plane_facing(const float* m, float mx, float my, float mz, float cos_min) { return fabsf(row3(m, mx, my, mz)) >= cos_min; }

// the whole test for point i of a cloud in memory: what the mask and the support kernels run
D3R_DEV bool plane_inlier(const float* m, const float* __restrict__ pts, const float* __restrict__ normals, long long i, float thr, float cos_min) {
    const float* p = pts + 3 * (size_t)i;
    const float x = p[0], y = p[1], z = p[2];
    bool in = finite3(x, y, z) && plane_near(m, x, y, z, thr);
    if (in && normals) {
        const float* q = normals + 3 * (size_t)i;
        const float mx = q[0], my = q[1], mz = q[2];
        in = normal_ok(mx, my, mz) && plane_facing(m, mx, my, mz, cos_min);
    }
    return in;
}

// A lane holds its SPL points, and with NRM their normals, in registers. A point that cannot be an inlier (past the end, non-finite) gets
// x = NaN and a normal that cannot pass (non-finite, zero) gets mx = NaN: every comparison with them is false, no flag register is kept.
template <bool NRM>
__global__ __launch_bounds__(SPT) void plane_score_kernel(const PlaneArgs a, const PlaneWs w) {
    __shared__ int any_valid;
    const int h0 = blockIdx.y * RND, n_slots = min(RND, a.n_hyp - h0);
    const long long p0 = (long long)blockIdx.x * SCHUNK;
    if (threadIdx.x == 0) any_valid = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < n_slots; t += SPT)
        if (w.valid[h0 + t]) any_valid = 1;                               // every writer stores the same value
    __syncthreads();
    if (!any_valid) return;
    const float nan_f = __uint_as_float(0x7FC00000u);
    float px[SPL], py[SPL], pz[SPL], mx[NRM ? SPL : 1], my[NRM ? SPL : 1], mz[NRM ? SPL : 1];
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const long long i = p0 + k * SPT + threadIdx.x;
        const size_t j = i < a.n ? (size_t)i : 0;
        const float* p = a.pts + j * 3;
        const float x = p[0], y = p[1], z = p[2];
        px[k] = i < a.n && finite3(x, y, z) ? x : nan_f;
        py[k] = y; pz[k] = z;
        if (NRM) {
            const float* q = a.normals + j * 3;
            const float u = q[0], v = q[1], s = q[2];
            mx[k] = normal_ok(u, v, s) ? u : nan_f;
            my[k] = v; mz[k] = s;
        }
    }
    ransac::score_round<SPT, SPL, RND>(w.rows + (size_t)h0 * 12, w.valid + h0, n_slots, w.counts + h0, [&](const float* row, int k) {
        bool in = plane_near(row, px[k], py[k], pz[k], a.thr);
        if (NRM) in = in && plane_facing(row, mx[k], my[k], mz[k], a.cos_min);
        return in;
    });
}

__global__ __launch_bounds__(QT) void plane_select_kernel(const PlaneArgs a, const PlaneWs w, double* __restrict__ best_out) {
    const ransac::Winner b = ransac::select_winner<QT>(a.n_hyp, w.valid, w.counts, a.min_inliers);
    if (threadIdx.x != 0) return;
    const bool found = b.h >= 0;
    w.best->h = b.h;
    w.best->count = b.count;
    w.best->n_valid = b.n_valid;
    best_out[0] = (double)b.h;
    best_out[1] = (double)b.count;
    best_out[2] = (double)b.n_valid;
    for (int c = 0; c < 4; ++c) {
        best_out[3 + c] = found ? w.planes[(size_t)b.h * 4 + c] : 0.0;
        w.best->row[c] = found ? w.rows[(size_t)b.h * 12 + c] : 0.f;
    }
}

__global__ __launch_bounds__(QT) void plane_mask_kernel(const PlaneArgs a, const PlaneWs w, uint8_t* __restrict__ inliers_out) {
    float m[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) m[c] = w.best->row[c];
    ransac::write_mask<QT>(a.n, w.best->h >= 0, inliers_out, [&](long long i) { return plane_inlier(m, a.pts, a.normals, i, a.thr, a.cos_min); });
}

struct SupportArgs {
    int n;
    float plane[4], centre[3];
    float thr, cos_min;
    const float* pts;
    const float* normals;
    uint8_t* mask_out;                  // optional
};

// partial b holds the rows b QT + thread + k gridDim QT, a fixed set in a fixed order
__global__ __launch_bounds__(QT) void plane_support_kernel(const SupportArgs a, double* __restrict__ part_d, long long* __restrict__ part_i) {
    double s[MOMENTS];
#pragma unroll
    for (int k = 0; k < MOMENTS; ++k) s[k] = 0.0;
    long long cnt[1] = {0};
    const double cx = (double)a.centre[0], cy = (double)a.centre[1], cz = (double)a.centre[2];
    for (long long i = (long long)blockIdx.x * QT + threadIdx.x; i < a.n; i += (long long)gridDim.x * QT) {
        const bool in = plane_inlier(a.plane, a.pts, a.normals, i, a.thr, a.cos_min);
        if (a.mask_out) a.mask_out[i] = in;
        if (!in) continue;
        const float* p = a.pts + 3 * (size_t)i;
        const double ax = (double)p[0] - cx, ay = (double)p[1] - cy, az = (double)p[2] - cz;
        cnt[0] += 1;
        s[0] += ax; s[1] += ay; s[2] += az;
        s[3] += ax * ax; s[4] += ax * ay; s[5] += ax * az;
        s[6] += ay * ay; s[7] += ay * az; s[8] += az * az;
    }
    cloud_block_sum<MOMENTS, 1>(s, cnt, part_d + (size_t)blockIdx.x * MOMENTS, part_i + blockIdx.x);
}

static inline bool finite_host(float v) { return v >= -3.4028234e38f && v <= 3.4028234e38f; }

}  // namespace cloud
}  // namespace d3r

using namespace d3r::cloud;

static bool plane_sizes_ok(int n, int n_hyp) { return n >= 3 && n_hyp >= 1 && n_hyp <= MAX_HYP; }

extern "C" size_t d3r_plane_ransac_workspace_bytes(int n, int n_hyp) {
    if (!plane_sizes_ok(n, n_hyp)) return 0;
    return plane_workspace(nullptr, n_hyp).bytes;
}

extern "C" int d3r_plane_ransac(int n, const float* points, const float* normals, unsigned long long seed, int n_hyp, float thr, float cos_min,
                                double min_area2, int min_inliers, double* best_out, uint8_t* inliers_out, void* workspace, void* stream) {
    if (!plane_sizes_ok(n, n_hyp) || !points || !best_out || !inliers_out || !workspace) return D3R_ERR_INVALID;
    if (!(thr > 0.f && finite_host(thr)) || !(cos_min == cos_min) || !(min_area2 > 0.0) || min_inliers < 3) return D3R_ERR_INVALID;
    PlaneArgs a;
    a.n = n; a.n_hyp = n_hyp; a.min_inliers = min_inliers; a.seed = seed; a.thr = thr; a.cos_min = cos_min; a.min_area2 = min_area2;
    a.pts = points; a.normals = normals;
    const PlaneWs w = plane_workspace(workspace, n_hyp);
    hipStream_t st = (hipStream_t)stream;
    const int rounds = (int)d3r::tiles_of(n_hyp, RND);
    const dim3 grid((unsigned)d3r::tiles_of(n, SCHUNK), rounds);
    hipLaunchKernelGGL(plane_hyp_kernel, dim3(rounds), dim3(RND), 0, st, a, w);
    if (normals) hipLaunchKernelGGL(plane_score_kernel<true>, grid, dim3(SPT), 0, st, a, w);
    else hipLaunchKernelGGL(plane_score_kernel<false>, grid, dim3(SPT), 0, st, a, w);
    hipLaunchKernelGGL(plane_select_kernel, dim3(1), dim3(QT), 0, st, a, w, best_out);
    hipLaunchKernelGGL(plane_mask_kernel, dim3(cloud_blocks(n)), dim3(QT), 0, st, a, w, inliers_out);
    return rc_of(hipGetLastError());
}

extern "C" size_t d3r_plane_support_workspace_bytes(int n) {
    if (n <= 0) return 0;
    return cloud_sum_parts(nullptr, n, MOMENTS, 1).bytes;
}

extern "C" int d3r_plane_support(int n, const float* points, const float* normals, const float* plane, float thr, float cos_min, const float* centre,
                                 uint8_t* mask_out, long long* count_out, double* sums_out, void* workspace, void* stream) {
    if (n <= 0 || !points || !plane || !centre || !count_out || !sums_out || !workspace) return D3R_ERR_INVALID;
    if (!(thr > 0.f && finite_host(thr)) || !(cos_min == cos_min)) return D3R_ERR_INVALID;
    SupportArgs a;
    a.n = n; a.thr = thr; a.cos_min = cos_min; a.pts = points; a.normals = normals; a.mask_out = mask_out;
    for (int c = 0; c < 4; ++c) {
        if (!finite_host(plane[c])) return D3R_ERR_INVALID;
        a.plane[c] = plane[c];
    }
    for (int c = 0; c < 3; ++c) {
        if (!finite_host(centre[c])) return D3R_ERR_INVALID;
        a.centre[c] = centre[c];
    }
    const SumParts p = cloud_sum_parts(workspace, n, MOMENTS, 1);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(plane_support_kernel, dim3(p.parts), dim3(QT), 0, st, a, p.d, p.i);
    hipLaunchKernelGGL((cloud_sums_final_kernel<MOMENTS, 1>), dim3(1), dim3(QT), 0, st, p.parts, p.d, p.i, count_out, sums_out);
    return rc_of(hipGetLastError());
}
