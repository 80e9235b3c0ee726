// dust3r_amd -- visual localization (the reference's visloc.py:72-165 per-query loop and dust3r_visloc/localization.py run_pnp),
// batched over many (query, map view) pairs and many queries.
//
// d3r_match_pairs: mutual nearest neighbours between the query pointmap and the map view's pointmap of every pair, each side masked
// by its confidence (and the map's validity), in one launch sequence:
//   match_compact_kernel  one 1024-thread workgroup per (pair, side): a block-wide prefix scan in raster order compacts the used
//                         pixels into (x, y, z, -) float4 rows and their flat pixel indices
//   match_nn_kernel       exact fp32 nearest neighbour of every compacted point on the other side. Grid = (query tile, side, pair):
//                         a workgroup owns 1024 queries (4 per lane, in registers) and streams the other side through LDS in
//                         1024-point tiles; every LDS read (a broadcast float4) feeds 4 distance evaluations. Same d = dx^2 + dy^2
//                         + dz^2 expression and strict-less scan as d3r_nearest_neighbors, so ties go to the lowest index.
//   match_mutual_kernel   one workgroup per pair: map point j is kept when nn_q(nn_m(j)) == j; a prefix scan writes the kept
//                         (query pixel, map pixel) pairs in ascending map order and the count.
// Tiles past a side's count exit at once, so the host sizes the grid by the largest pair and never reads a count.
//
// d3r_pnp_ransac: PnP-RANSAC with full intrinsics for many jobs (queries) in one call, no host synchronisation inside:
//   pnp_init_kernel        per-job state (iteration budget, best support)
//   per round of RND hypotheses:
//     pnp_hyp_kernel       one lane per hypothesis: counter-based sample (seed, hypothesis) -> 4 distinct points (ransac.hpp), fp64 P3P
//                          on the first three, the root that best reprojects the fourth; written as fp32 rows pre-scaled by fx / fy
//     pnp_score_kernel     grid (point chunk, job): ransac.hpp's round scorer (hypotheses in LDS, 4 points per lane, ballots, integer atomics);
//                          a point is an inlier when it is in front of the camera and ex^2 + ey^2 <= thr^2 z^2 (the squared pixel error
//                          against the squared threshold, multiplied through by z^2).
//     pnp_select_kernel    the round's best hypothesis (largest support, then lowest index) replaces the job's best when its support
//                          is strictly larger and updates the budget (RANSACUpdateNumIters); the job is done once the rounds so far
//                          cover the budget. The budget is checked between rounds, so every job scores at least one full round.
//   pnp_lm_kernel x LM_ITERS  Levenberg-Marquardt on the reprojection error over the best hypothesis's inliers: fp64 J^T J, J^T r and
//                          cost per 1024-point chunk (fixed-order block reduction) ...
//   pnp_lm_step_kernel     ... summed over chunks in order, damped 6x6 Cholesky solve, accept / reject
//   pnp_count_kernel       inliers of the refined pose (same fp32 test), optional per-point mask
//   pnp_output_kernel      pose, inlier count, status (and, on request, hypotheses drawn and the best one's index)
// The host launches rounds up to the largest max_iters of the batch; rounds of finished jobs exit at their first read of the done flag.
// Every quantity of a job depends only on that job's record: the same bits whether it runs alone or in any batch.
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "reduce.hpp"
#include "ransac.hpp"
#include "visloc_math.hpp"

namespace d3r {
namespace vl {

// ---- matching ------------------------------------------------------------------------------------------------------------------
constexpr int CNT = 1024;       // threads of the compaction / mutual workgroups
constexpr int QT = 256;         // threads of the scan workgroup
constexpr int QPL = 4;          // queries per lane
constexpr int QTILE = QT * QPL; // queries per workgroup
constexpr int RTILE = 1024;     // other-side points per LDS tile

// per pair, inside the workspace (stride = max_pixels): pts[2] float4, then per side pix, nn int32, then count[2]. Addressed by
// arithmetic on `side` (a per-workgroup value): an array of pointers indexed by it would go to scratch.
__host__ __device__ inline size_t pix_offset(int max_pixels, int side) { return 2 * (size_t)max_pixels * sizeof(float4) + (size_t)(2 * side) * max_pixels * sizeof(int); }
// a pair's record ends 16 bytes behind the start of its last field, count[2] (where the pix of a third side would start)
__host__ __device__ inline size_t match_pair_bytes(int max_pixels) { return pix_offset(max_pixels, 2) + 16; }
D3R_DEV char* match_base(void* workspace, int pair, int max_pixels) { return (char*)workspace + (size_t)pair * match_pair_bytes(max_pixels); }
D3R_DEV float4* ws_pts(char* base, int max_pixels, int side) { return (float4*)base + (size_t)side * max_pixels; }
D3R_DEV int* ws_pix(char* base, int max_pixels, int side) { return (int*)(base + pix_offset(max_pixels, side)); }
D3R_DEV int* ws_nn(char* base, int max_pixels, int side) { return ws_pix(base, max_pixels, side) + max_pixels; }
D3R_DEV int* ws_count(char* base, int max_pixels) { return ws_pix(base, max_pixels, 2); }

__global__ __launch_bounds__(CNT) void match_compact_kernel(const d3r_match_job* __restrict__ jobs, int max_pixels, void* workspace) {
    __shared__ int wave_sums[CNT / 64];
    const int side = blockIdx.x, pair = blockIdx.y;
    const d3r_match_job J = jobs[pair];
    char* ws = match_base(workspace, pair, max_pixels);
    float4* out_pts = ws_pts(ws, max_pixels, side);
    int* out_pix = ws_pix(ws, max_pixels, side);
    const int n = min(side == 0 ? J.n_query : J.n_map, max_pixels);      // never past the workspace rows
    const float* pts = side == 0 ? J.pts_query : J.pts_map;
    const float* conf = side == 0 ? J.conf_query : J.conf_map;
    const uint8_t* valid = side == 0 ? nullptr : J.valid_map;
    int base = 0;
    for (int p0 = 0; p0 < n; p0 += CNT) {
        const int p = p0 + threadIdx.x;
        const bool use = p < n && conf[p] >= J.conf_thr && (valid == nullptr || valid[p] != 0);
        int total;
        const int pos = block_scan_1024(use, wave_sums, &total);
        if (use) {
            out_pts[base + pos] = make_float4(pts[(size_t)p * 3], pts[(size_t)p * 3 + 1], pts[(size_t)p * 3 + 2], 0.f);
            out_pix[base + pos] = p;
        }
        base += total;
    }
    if (threadIdx.x == 0) ws_count(ws, max_pixels)[side] = base;
}

__global__ __launch_bounds__(QT) void match_nn_kernel(int max_pixels, void* workspace) {
    __shared__ float4 tile[RTILE];
    const int side = blockIdx.y, pair = blockIdx.z;
    char* ws = match_base(workspace, pair, max_pixels);
    const int* cnt = ws_count(ws, max_pixels);
    const int nq = cnt[side], nr = cnt[1 - side];
    const int q0 = blockIdx.x * QTILE;
    if (q0 >= nq || nr == 0) return;
    const float4* __restrict__ Q = ws_pts(ws, max_pixels, side);
    const float4* __restrict__ R = ws_pts(ws, max_pixels, 1 - side);
    int* __restrict__ nn_out = ws_nn(ws, max_pixels, side);
    float qx[QPL], qy[QPL], qz[QPL], best[QPL];
    int bi[QPL];
#pragma unroll
    for (int k = 0; k < QPL; ++k) {
        const int q = q0 + k * QT + threadIdx.x;
        const float4 v = q < nq ? Q[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        qx[k] = v.x; qy[k] = v.y; qz[k] = v.z;
        best[k] = 3.4e38f;
        bi[k] = 0;
    }
    for (int r0 = 0; r0 < nr; r0 += RTILE) {
        __syncthreads();
        const int tn = min(RTILE, nr - r0);              // the last tile is partial: its unfilled slots are never scanned, so bi < nr
        for (int t = threadIdx.x; t < tn; t += QT) tile[t] = R[r0 + t];
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < tn; ++t) {
            const float4 p = tile[t];
#pragma unroll
            for (int k = 0; k < QPL; ++k) {
                const float dx = qx[k] - p.x, dy = qy[k] - p.y, dz = qz[k] - p.z;
                const float d = dx * dx + dy * dy + dz * dz;
                if (d < best[k]) { best[k] = d; bi[k] = r0 + t; }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < QPL; ++k) {
        const int q = q0 + k * QT + threadIdx.x;
        if (q < nq) nn_out[q] = bi[k];
    }
}

__global__ __launch_bounds__(CNT) void match_mutual_kernel(int max_pixels, void* workspace, int* __restrict__ out_counts,
                                                           int* __restrict__ out_pairs) {
    __shared__ int wave_sums[CNT / 64];
    const int pair = blockIdx.x;
    char* ws = match_base(workspace, pair, max_pixels);
    const int nq = ws_count(ws, max_pixels)[0], nm = ws_count(ws, max_pixels)[1];
    const int* nn_q = ws_nn(ws, max_pixels, 0);
    const int* nn_m = ws_nn(ws, max_pixels, 1);
    const int* pix_q = ws_pix(ws, max_pixels, 0);
    const int* pix_m = ws_pix(ws, max_pixels, 1);
    int* out = out_pairs + (size_t)pair * max_pixels * 2;
    int base = 0;
    if (nq > 0) {
        for (int j0 = 0; j0 < nm; j0 += CNT) {
            const int j = j0 + threadIdx.x;
            int i = 0;
            bool keep = false;
            if (j < nm) {
                i = nn_m[j];
                keep = i >= 0 && i < nq && nn_q[i] == j;
            }
            int total;
            const int pos = block_scan_1024(keep, wave_sums, &total);
            if (keep) {
                out[(size_t)(base + pos) * 2] = pix_q[i];
                out[(size_t)(base + pos) * 2 + 1] = pix_m[j];
            }
            base += total;
        }
    }
    if (threadIdx.x == 0) out_counts[pair] = base;
}

// ---- PnP-RANSAC -----------------------------------------------------------------------------------------------------------------
constexpr int RND = 128;        // hypotheses per round
constexpr int PT = 256;         // threads of the point workgroups
constexpr int PPL = 4;          // points per lane
constexpr int CHUNK = PT * PPL; // points per workgroup
constexpr int LM_ITERS = 24;
constexpr int NSUM = 32;        // J^T J (21, upper triangle row-major), J^T r (6), cost, points, points behind the camera, pad
constexpr int MODEL_POINTS = 4;

struct PnpState {
    double best_pose[12];       // fp64 pose of the best hypothesis
    double cur[12], trial[12];  // LM: accepted pose, pose being evaluated
    double cur_sums[NSUM];
    double lambda;
    float best_rows[12];        // the best hypothesis as scored (fp32 scaled rows): defines the LM inlier set
    float final_rows[12];
    int niters, best_support, best_h, done, status, inliers, drawn, pad;
};

struct PnpWs {
    PnpState* st;
    double* hyp_pose;           // [RND][12]
    float* hyp_rows;            // [RND][12]
    int* hyp_valid;             // [RND]
    int* counts;                // [RND]
    double* partial;            // [chunks][NSUM]
    size_t bytes;
};

__host__ __device__ inline int pnp_chunks(int max_points) { return (max_points + CHUNK - 1) / CHUNK; }

// one job's record carved at base; a null base gives its size (every array is a multiple of 256 bytes, the state is padded to one)
__host__ __device__ inline PnpWs pnp_job(void* base, int max_points) {
    PnpWs w;
    Carver c(base);
    w.st = c.take<PnpState>(1);
    w.hyp_pose = c.take<double>((size_t)RND * 12);
    w.hyp_rows = c.take<float>((size_t)RND * 12);
    w.hyp_valid = c.take<int>(RND);
    w.counts = c.take<int>(RND);
    w.partial = c.take<double>((size_t)pnp_chunks(max_points) * NSUM);
    w.bytes = c.bytes;
    return w;
}

D3R_DEV PnpWs pnp_ws(void* workspace, int job, int max_points) {
    return pnp_job((char*)workspace + (size_t)job * pnp_job(nullptr, max_points).bytes, max_points);
}

// fp32 rows {fx R0, fx t0, fy R1, fy t1, R2, t2} of a world -> camera pose: x = rows0 . (X, 1), y = rows1 . (X, 1), z = rows2 . (X, 1)
D3R_DEV void scaled_rows(const double* pose, const d3r_pnp_ransac_job& J, float* rows) {
    for (int c = 0; c < 4; ++c) {
        rows[c] = (float)(J.fx * pose[c]);
        rows[4 + c] = (float)(J.fy * pose[4 + c]);
        rows[8 + c] = (float)pose[8 + c];
    }
}

// the inlier test of every RANSAC stage: in front of the camera and squared pixel error <= thr^2, multiplied through by z^2. The right side
// must be finite: a world point with an infinite coordinate can give z = +inf, and inf <= inf would make it an inlier (of the LM set too,
// where its NaN residual freezes the polish). A NaN or infinity anywhere else already fails one of the comparisons, so with this term a row
// with a non-finite coordinate is never an inlier; for finite rows the term is true and the rest is the expression it always was.
D3R_DEV bool is_inlier(const float* rows, float X, float Y, float Z, float a, float b, float thr2) {
    const float x = rows[0] * X + rows[1] * Y + rows[2] * Z + rows[3];
    const float y = rows[4] * X + rows[5] * Y + rows[6] * Z + rows[7];
    const float z = rows[8] * X + rows[9] * Y + rows[10] * Z + rows[11];
    const float ex = x - a * z, ey = y - b * z;
    const float lim = thr2 * (z * z);
    return z > 0.f && lim < INFINITY && ex * ex + ey * ey <= lim;
}

__global__ __launch_bounds__(64) void pnp_init_kernel(const d3r_pnp_ransac_job* __restrict__ jobs, int max_points, void* workspace) {
    const int j = blockIdx.x;
    if (threadIdx.x != 0) return;
    const d3r_pnp_ransac_job J = jobs[j];
    PnpState* st = pnp_ws(workspace, j, max_points).st;
    st->niters = J.max_iters;
    st->best_support = 0;
    st->best_h = -1;
    st->drawn = 0;
    st->done = (J.n <= MODEL_POINTS || J.n > max_points || J.max_iters <= 0) ? 1 : 0;
    st->status = 0;
    st->inliers = 0;
    st->lambda = 1e-3;
}

__global__ __launch_bounds__(RND) void pnp_hyp_kernel(const d3r_pnp_ransac_job* __restrict__ jobs, int max_points, void* workspace, int round) {
    const int j = blockIdx.x;
    const PnpWs w = pnp_ws(workspace, j, max_points);
    const int done = w.st->done, niters = w.st->niters;
    if (done) return;
    const d3r_pnp_ransac_job J = jobs[j];
    const int hl = threadIdx.x, h = round * RND + hl;
    w.counts[hl] = 0;
    int valid = 0;
    if (h < niters) {
        int idx[MODEL_POINTS];
        if (ransac::draw_distinct(J.seed, h, J.n, idx)) {
            double uv[4][2], X[4][3], pose[12];
            for (int i = 0; i < 4; ++i) {
                uv[i][0] = J.pts2d[(size_t)idx[i] * 2];
                uv[i][1] = J.pts2d[(size_t)idx[i] * 2 + 1];
                for (int r = 0; r < 3; ++r) X[i][r] = J.pts3d[(size_t)idx[i] * 3 + r];
            }
            if (p3p_pick(uv, X, J.fx, J.fy, J.cx, J.cy, pose)) {
                valid = 1;
                float rows[12];
                scaled_rows(pose, J, rows);
                for (int c = 0; c < 12; ++c) {
                    w.hyp_pose[hl * 12 + c] = pose[c];
                    w.hyp_rows[hl * 12 + c] = rows[c];
                }
            }
        }
    }
    w.hyp_valid[hl] = valid;
}

__global__ __launch_bounds__(PT) void pnp_score_kernel(const d3r_pnp_ransac_job* __restrict__ jobs, int max_points, void* workspace) {
    const int j = blockIdx.y;
    const PnpWs w = pnp_ws(workspace, j, max_points);
    const d3r_pnp_ransac_job J = jobs[j];
    const int p0 = blockIdx.x * CHUNK;
    if (w.st->done || p0 >= J.n) return;
    float X[PPL], Y[PPL], Z[PPL], a[PPL], b[PPL];
    bool live[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
        const int p = p0 + k * PT + threadIdx.x;
        live[k] = p < J.n;
        const int q = live[k] ? p : 0;
        X[k] = J.pts3d[(size_t)q * 3]; Y[k] = J.pts3d[(size_t)q * 3 + 1]; Z[k] = J.pts3d[(size_t)q * 3 + 2];
        a[k] = J.pts2d[(size_t)q * 2] - J.cx;
        b[k] = J.pts2d[(size_t)q * 2 + 1] - J.cy;
    }
    const float thr2 = J.thr * J.thr;
    ransac::score_round<PT, PPL, RND>(w.hyp_rows, w.hyp_valid, RND, w.counts,
                                      [&](const float* row, int k) { return live[k] && is_inlier(row, X[k], Y[k], Z[k], a[k], b[k], thr2); });
}

__global__ __launch_bounds__(64) void pnp_select_kernel(const d3r_pnp_ransac_job* __restrict__ jobs, int max_points, void* workspace, int round) {
    const int j = blockIdx.x;
    if (threadIdx.x != 0) return;
    const PnpWs w = pnp_ws(workspace, j, max_points);
    PnpState* st = w.st;
    if (st->done) return;
    const d3r_pnp_ransac_job J = jobs[j];
    st->drawn += min(RND, max(0, st->niters - round * RND));     // hypotheses this round drew (pnp_hyp_kernel read the same budget)
    // the round's best: largest support, then lowest index (hypotheses past the budget at the round's start were not drawn)
    int bc = -1, bl = -1;
    for (int hl = 0; hl < RND; ++hl) {
        const int c = w.hyp_valid[hl] ? w.counts[hl] : -1;
        if (c > bc) { bc = c; bl = hl; }
    }
    if (bl >= 0 && bc > max(st->best_support, MODEL_POINTS - 1)) {
        st->best_support = bc;
        st->best_h = round * RND + bl;
        for (int k = 0; k < 12; ++k) {
            st->best_pose[k] = w.hyp_pose[bl * 12 + k];
            st->best_rows[k] = w.hyp_rows[bl * 12 + k];
        }
        st->niters = ransac_update_num_iters(J.confidence, (double)(J.n - bc) / J.n, MODEL_POINTS, st->niters);
    }
    if ((round + 1) * RND >= st->niters) st->done = 1;
}

// LM starts from the best hypothesis; a job without a hypothesis supported beyond its minimal sample fails here
__global__ __launch_bounds__(64) void pnp_lm_init_kernel(int n_jobs, int max_points, void* workspace) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n_jobs) return;
    PnpState* st = pnp_ws(workspace, j, max_points).st;
    st->status = st->best_support > MODEL_POINTS ? 1 : 0;
    for (int k = 0; k < 12; ++k) st->cur[k] = st->trial[k] = st->best_pose[k];
    st->lambda = 1e-3;
    st->cur_sums[NSUM - 1] = -1.0;          // no accepted evaluation yet
}

// per chunk: the Gauss-Newton sums of the reprojection error at the trial pose over the best hypothesis's inliers. Parameters: a
// rotation increment w and a translation increment d of the camera-frame point, x' = x + w x x + d (left perturbation).
__global__ __launch_bounds__(PT) void pnp_lm_kernel(const d3r_pnp_ransac_job* __restrict__ jobs, int max_points, void* workspace) {
    __shared__ double red[PT / 64 * (NSUM - 2)];
    const int j = blockIdx.y;
    const PnpWs w = pnp_ws(workspace, j, max_points);
    const d3r_pnp_ransac_job J = jobs[j];
    const int p0 = blockIdx.x * CHUNK;
    if (!w.st->status || p0 >= J.n) return;
    double P[12];
    float rows[12];
    for (int k = 0; k < 12; ++k) { P[k] = w.st->trial[k]; rows[k] = w.st->best_rows[k]; }
    const float thr2 = J.thr * J.thr;
    double s[NSUM - 2];
    for (int k = 0; k < NSUM - 2; ++k) s[k] = 0.0;
    for (int k = 0; k < PPL; ++k) {
        const int p = p0 + k * PT + threadIdx.x;
        if (p >= J.n) break;
        const float Xf = J.pts3d[(size_t)p * 3], Yf = J.pts3d[(size_t)p * 3 + 1], Zf = J.pts3d[(size_t)p * 3 + 2];
        const float uf = J.pts2d[(size_t)p * 2], vf = J.pts2d[(size_t)p * 2 + 1];
        if (!is_inlier(rows, Xf, Yf, Zf, uf - J.cx, vf - J.cy, thr2)) continue;
        const double X = Xf, Y = Yf, Z = Zf;
        const double x = P[0] * X + P[1] * Y + P[2] * Z + P[3];
        const double y = P[4] * X + P[5] * Y + P[6] * Z + P[7];
        const double z = P[8] * X + P[9] * Y + P[10] * Z + P[11];
        s[28] += 1.0;
        if (!(z > 0.0)) { s[29] += 1.0; continue; }
        const double iz = 1.0 / z;
        const double ru = J.fx * x * iz + J.cx - (double)uf, rv = J.fy * y * iz + J.cy - (double)vf;
        // d(u, v)/d(x, y, z), then d(x, y, z)/d(w, d) = [-[x]_x | I]
        const double ux = J.fx * iz, uz = -J.fx * x * iz * iz, vy = J.fy * iz, vz = -J.fy * y * iz * iz;
        double ju[6], jv[6];
        // d(w x x)/dw = -[x]_x, columns: d/dw0 = (0, -z, y), d/dw1 = (z, 0, -x), d/dw2 = (-y, x, 0)
        ju[0] = uz * y;            jv[0] = vy * -z + vz * y;
        ju[1] = ux * z + uz * -x;  jv[1] = vz * -x;
        ju[2] = ux * -y;           jv[2] = vy * x;
        ju[3] = ux;                jv[3] = 0.0;
        ju[4] = 0.0;               jv[4] = vy;
        ju[5] = uz;                jv[5] = vz;
        int m = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) s[m++] += ju[r] * ju[c] + jv[r] * jv[c];
        for (int r = 0; r < 6; ++r) s[21 + r] += ju[r] * ru + jv[r] * rv;
        s[27] += ru * ru + rv * rv;
    }
    // fixed-order reduction (reduce.hpp): wave butterflies, then column k by thread k over the 4 waves in order. The per-thread sums start
    // at +0.0, so no wave's value is -0.0 and starting from wave 0's value gives the bits of starting from 0.0
    block_reduce_columns<PT, NSUM - 2>(s, red, Sum(), w.partial + (size_t)blockIdx.x * NSUM);
}

// x' = exp([w]) x + d applied to the pose: R' = exp([w]) R, t' = exp([w]) t + d
D3R_DEV void apply_increment(const double* P, const double* dx, double* out) {
    const double th = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
    double E[9];
    const double K[9] = {0.0, -dx[2], dx[1], dx[2], 0.0, -dx[0], -dx[1], dx[0], 0.0};
    double K2[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) K2[r * 3 + c] = K[r * 3] * K[c] + K[r * 3 + 1] * K[3 + c] + K[r * 3 + 2] * K[6 + c];
    const double A = th > 1e-8 ? sin(th) / th : 1.0 - th * th / 6.0;
    const double B = th > 1e-8 ? (1.0 - cos(th)) / (th * th) : 0.5 - th * th / 24.0;
    for (int k = 0; k < 9; ++k) E[k] = (k % 4 == 0 ? 1.0 : 0.0) + A * K[k] + B * K2[k];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) out[r * 4 + c] = E[r * 3] * P[c] + E[r * 3 + 1] * P[4 + c] + E[r * 3 + 2] * P[8 + c] + (c == 3 ? dx[3 + r] : 0.0);
}

__global__ __launch_bounds__(64) void pnp_lm_step_kernel(const d3r_pnp_ransac_job* __restrict__ jobs, int n_jobs, int max_points, void* workspace) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n_jobs) return;
    const PnpWs w = pnp_ws(workspace, j, max_points);
    PnpState* st = w.st;
    if (!st->status) return;
    const int nch = (jobs[j].n + CHUNK - 1) / CHUNK;
    double S[NSUM];
    for (int k = 0; k < NSUM; ++k) S[k] = 0.0;
    for (int c = 0; c < nch; ++c)
        for (int k = 0; k < NSUM - 2; ++k) S[k] += w.partial[(size_t)c * NSUM + k];
    const bool first = st->cur_sums[NSUM - 1] < 0.0;
    const bool ok = S[29] == 0.0 && isfinite(S[27]);
    if (first || (ok && S[27] < st->cur_sums[27])) {
        for (int k = 0; k < 12; ++k) st->cur[k] = st->trial[k];
        for (int k = 0; k < NSUM - 1; ++k) st->cur_sums[k] = S[k];
        st->cur_sums[NSUM - 1] = 1.0;
        if (!first) st->lambda = fmax(st->lambda * 0.1, 1e-12);
    } else {
        st->lambda = fmin(st->lambda * 10.0, 1e12);
    }
    // damped normal equations (A + lambda diag(A)) dx = -g, Cholesky
    double A[36], g[6], L[36];
    int m = 0;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) { A[r * 6 + c] = A[c * 6 + r] = st->cur_sums[m++]; }
    for (int r = 0; r < 6; ++r) { g[r] = st->cur_sums[21 + r]; A[r * 6 + r] *= 1.0 + st->lambda; }
    bool pd = true;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            double v = A[r * 6 + c];
#pragma unroll
            for (int k = 0; k < c; ++k) v -= L[r * 6 + k] * L[c * 6 + k];
            if (r == c) {
                pd = pd && v > 0.0;
                L[r * 6 + r] = sqrt(fmax(v, 1e-300));
            } else {
                L[r * 6 + c] = v / L[c * 6 + c];
            }
        }
    if (!pd) { for (int k = 0; k < 12; ++k) st->trial[k] = st->cur[k]; return; }
    double y[6], dx[6];
    for (int r = 0; r < 6; ++r) {
        double v = -g[r];
        for (int k = 0; k < r; ++k) v -= L[r * 6 + k] * y[k];
        y[r] = v / L[r * 6 + r];
    }
    for (int r = 5; r >= 0; --r) {
        double v = y[r];
        for (int k = r + 1; k < 6; ++k) v -= L[k * 6 + r] * dx[k];
        dx[r] = v / L[r * 6 + r];
    }
    apply_increment(st->cur, dx, st->trial);
}

__global__ __launch_bounds__(64) void pnp_final_rows_kernel(const d3r_pnp_ransac_job* __restrict__ jobs, int n_jobs, int max_points, void* workspace) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n_jobs) return;
    PnpState* st = pnp_ws(workspace, j, max_points).st;
    const d3r_pnp_ransac_job J = jobs[j];
    scaled_rows(st->cur, J, st->final_rows);
    st->inliers = 0;
}

__global__ __launch_bounds__(PT) void pnp_count_kernel(const d3r_pnp_ransac_job* __restrict__ jobs, int max_points, void* workspace) {
    __shared__ int cnt;
    const int j = blockIdx.y;
    const PnpWs w = pnp_ws(workspace, j, max_points);
    const d3r_pnp_ransac_job J = jobs[j];
    const int p0 = blockIdx.x * CHUNK;
    if (p0 >= J.n) return;
    const int status = w.st->status;
    float rows[12];
    for (int k = 0; k < 12; ++k) rows[k] = w.st->final_rows[k];
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const float thr2 = J.thr * J.thr;
    int c = 0;
    for (int k = 0; k < PPL; ++k) {
        const int p = p0 + k * PT + threadIdx.x;
        bool inl = false;
        if (p < J.n && status)
            inl = is_inlier(rows, J.pts3d[(size_t)p * 3], J.pts3d[(size_t)p * 3 + 1], J.pts3d[(size_t)p * 3 + 2],
                            J.pts2d[(size_t)p * 2] - J.cx, J.pts2d[(size_t)p * 2 + 1] - J.cy, thr2);
        if (p < J.n && J.inlier_mask) J.inlier_mask[p] = inl ? 1 : 0;
        c += __popcll(__ballot(inl));
    }
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&cnt, c);
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(&w.st->inliers, cnt);
}

__global__ __launch_bounds__(64) void pnp_output_kernel(int n_jobs, int max_points, void* workspace, double* __restrict__ out_poses,
                                                        int* __restrict__ out_inliers, int* __restrict__ out_status, int* __restrict__ out_stats) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n_jobs) return;
    const PnpState* st = pnp_ws(workspace, j, max_points).st;
    for (int k = 0; k < 12; ++k) out_poses[(size_t)j * 12 + k] = st->status ? st->cur[k] : 0.0;
    out_inliers[j] = st->status ? st->inliers : 0;
    out_status[j] = st->status;
    if (out_stats) {
        out_stats[j * 2] = st->drawn;
        out_stats[j * 2 + 1] = st->best_h;
    }
}

}  // namespace vl
}  // namespace d3r

using namespace d3r::vl;

extern "C" size_t d3r_match_pairs_workspace(int n_pairs, int max_pixels) {
    if (n_pairs <= 0 || max_pixels <= 0) return 0;
    return (size_t)n_pairs * match_pair_bytes(max_pixels);
}

extern "C" int d3r_match_pairs(int n_pairs, const d3r_match_job* jobs, int max_pixels, void* workspace, int* out_counts, int* out_pairs,
                               void* stream) {
    if (n_pairs <= 0 || n_pairs > 65535 || max_pixels <= 0 || !jobs || !workspace || !out_counts || !out_pairs) return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(match_compact_kernel, dim3(2, n_pairs), dim3(CNT), 0, st, jobs, max_pixels, workspace);
    hipLaunchKernelGGL(match_nn_kernel, dim3((max_pixels + QTILE - 1) / QTILE, 2, n_pairs), dim3(QT), 0, st, max_pixels, workspace);
    hipLaunchKernelGGL(match_mutual_kernel, dim3(n_pairs), dim3(CNT), 0, st, max_pixels, workspace, out_counts, out_pairs);
    return hipGetLastError() == hipSuccess ? D3R_OK : D3R_ERR_LAUNCH;
}

extern "C" size_t d3r_pnp_ransac_workspace(int n_jobs, int max_points) {
    if (n_jobs <= 0 || max_points <= 0) return 0;
    return (size_t)n_jobs * pnp_job(nullptr, max_points).bytes;
}

extern "C" int d3r_pnp_ransac(int n_jobs, const d3r_pnp_ransac_job* jobs, const d3r_pnp_ransac_params* params, void* workspace,
                              double* out_poses, int* out_inliers, int* out_status, int* out_stats, void* stream) {
    if (n_jobs <= 0 || n_jobs > 65535 || !jobs || !params || !workspace || !out_poses || !out_inliers || !out_status) return D3R_ERR_INVALID;
    const int max_points = params->max_points, max_iters = params->max_iters;
    if (max_points <= 0 || max_iters < 0) return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int chunks = pnp_chunks(max_points), g64 = (n_jobs + 63) / 64;
    hipLaunchKernelGGL(pnp_init_kernel, dim3(n_jobs), dim3(64), 0, st, jobs, max_points, workspace);
    for (int r = 0; r * RND < max_iters; ++r) {
        hipLaunchKernelGGL(pnp_hyp_kernel, dim3(n_jobs), dim3(RND), 0, st, jobs, max_points, workspace, r);
        hipLaunchKernelGGL(pnp_score_kernel, dim3(chunks, n_jobs), dim3(PT), 0, st, jobs, max_points, workspace);
        hipLaunchKernelGGL(pnp_select_kernel, dim3(n_jobs), dim3(64), 0, st, jobs, max_points, workspace, r);
    }
    hipLaunchKernelGGL(pnp_lm_init_kernel, dim3(g64), dim3(64), 0, st, n_jobs, max_points, workspace);
    for (int it = 0; it < LM_ITERS; ++it) {
        hipLaunchKernelGGL(pnp_lm_kernel, dim3(chunks, n_jobs), dim3(PT), 0, st, jobs, max_points, workspace);
        hipLaunchKernelGGL(pnp_lm_step_kernel, dim3(g64), dim3(64), 0, st, jobs, n_jobs, max_points, workspace);
    }
    hipLaunchKernelGGL(pnp_final_rows_kernel, dim3(g64), dim3(64), 0, st, jobs, n_jobs, max_points, workspace);
    hipLaunchKernelGGL(pnp_count_kernel, dim3(chunks, n_jobs), dim3(PT), 0, st, jobs, max_points, workspace);
    hipLaunchKernelGGL(pnp_output_kernel, dim3(g64), dim3(64), 0, st, n_jobs, max_points, workspace, out_poses, out_inliers, out_status, out_stats);
    return hipGetLastError() == hipSuccess ? D3R_OK : D3R_ERR_LAUNCH;
}

// host-only self test of the P3P solver (no GPU touched; all pointers HOST): uv [4][2] pixels, X [4][3] world points
extern "C" int d3r_selftest_p3p_host(const double* uv, const double* X, double fx, double fy, double cx, double cy, double* pose_out) {
    double u[4][2], x[4][3];
    for (int i = 0; i < 4; ++i) {
        u[i][0] = uv[i * 2]; u[i][1] = uv[i * 2 + 1];
        for (int r = 0; r < 3; ++r) x[i][r] = X[i * 3 + r];
    }
    return p3p_pick(u, x, fx, fy, cx, cy, pose_out) ? 1 : 0;
}

extern "C" int d3r_selftest_p3p_roots_host(const double* f, const double* X, double* R_out, double* t_out) {
    double ff[3][3], xx[3][3];
    for (int i = 0; i < 3; ++i)
        for (int r = 0; r < 3; ++r) { ff[i][r] = f[i * 3 + r]; xx[i][r] = X[i * 3 + r]; }
    int n = 0;
    p3p_grunert(ff, xx, [&](const double* R, const double* t) {
        for (int c = 0; c < 9; ++c) R_out[n * 9 + c] = R[c];
        for (int c = 0; c < 3; ++c) t_out[n * 3 + c] = t[c];
        ++n;
    });
    return n;
}

extern "C" int d3r_selftest_ransac_iters_host(double confidence, double ep, int model_points, int max_iters) {
    return ransac_update_num_iters(confidence, ep, model_points, max_iters);
}

// host-only: ransac.hpp's first k distinct draws of hypothesis h (k = 3 or 4) into idx_out[k]; 1 when 64 draws gave them, -1 for another k
extern "C" int d3r_selftest_draw_distinct_host(unsigned long long seed, int h, int n, int k, int* idx_out) {
    if (k == 3) return d3r::ransac::draw_distinct(seed, h, n, *(int(*)[3])idx_out) ? 1 : 0;
    if (k == 4) return d3r::ransac::draw_distinct(seed, h, n, *(int(*)[4])idx_out) ? 1 : 0;
    return -1;
}
