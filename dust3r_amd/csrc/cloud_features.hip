// dust3r_amd -- global (initialisation-free) registration of two clouds (new; the reference has none): the device stages of
// dust3r_amd/cloud_metrics.py, global_registration. Every stage is DEFINED in include/dust3r_hip.h without reference to
// how it is computed; tests/test_cloud_global_cpu.py restates each in numpy.
//   d3r_cloud_grid_heads   cloud_grid_heads_kernel    the lowest original index of every occupied cell of a built grid, in key order
//   d3r_cloud_spfh         cloud_spfh_kernel          per point the 3 x 11 histogram of its pair features (alpha, phi, theta), one thread per point
//   d3r_cloud_fpfh         cloud_fpfh_kernel          per point the distance-weighted sum of its neighbours' histograms, fp64, one thread per point
//   d3r_feature_nearest    feature_nearest_kernel     exhaustive nearest row of b for every row of a in 33 dimensions: THE HOT KERNEL
//   d3r_sim3_ransac        sim3_hyp_kernel            one thread per hypothesis: counter-based sample of 3 correspondences (ransac.hpp), fp64 similarity
//                          sim3_score_kernel          grid (correspondence chunk, round of RND hypotheses): ransac.hpp's round scorer
//                          sim3_select_kernel         one workgroup: the largest count, then the lowest hypothesis (ransac.hpp's selection)
//                          sim3_mask_kernel           the winner's inlier mask (ransac.hpp's loop)
// No floating-point atomics, no kernel waits on another workgroup, no scratch. The only atomics are integer additions of inlier counts
// (sim3_score_kernel), whose result does not depend on their order: the same bytes on every run. Built without contraction: every
// product and sum below is one IEEE rounding, which is what the numpy restatements compute; the fp32 3-vector arithmetic is fuse_grid.hpp's.
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "scene_common.hpp"
#include "fuse_grid.hpp"
#include "cloud_grid.hpp"
#include "ransac.hpp"
#include "visloc_math.hpp"      // triangle_frame: the Sim(3) hypothesis is the motion between the frames of its two sampled triangles

namespace d3r {
namespace cloud {

using namespace d3r::fuse;

// ---- 1. the heads of the grid's cells ---------------------------------------------------------------------------------------------------
// The grid stores the valid points in (key, original index) order: the sort is stable and its input is in index order. So the first point
// of cell j is the cell's lowest original index.
__global__ __launch_bounds__(QT) void cloud_grid_heads_kernel(const float4* __restrict__ pts4, const int* __restrict__ cell_start, const int* __restrict__ n_dev,
                                                             int cap, int* __restrict__ indices_out, int* __restrict__ count_out) {
    const int M = count_of(n_dev + 1, cap);
    for (long long j = (long long)blockIdx.x * QT + threadIdx.x; j < M; j += (long long)gridDim.x * QT) {
        const int s = min(max(cell_start[j], 0), cap - 1);                // a workspace that holds no grid must not send the read outside it
        indices_out[j] = __float_as_int(pts4[s].w);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) count_out[0] = M;
}

// ---- 2. SPFH ----------------------------------------------------------------------------------------------------------------------------
constexpr int BINS = 11, FEAT = 3 * BINS, SPFH_ROW = 36;                  // 33 counts, the pairs counted, two zero bytes

// floorf((x - lo) / width 11) clamped to [0, 10]; a NaN lands in bin 0
D3R_DEV int bin11(float x, float lo, float width) {
    const float t = floorf(__fmul_rn(__fdiv_rn(__fsub_rn(x, lo), width), 11.f));
    return (int)fminf(fmaxf(t, 0.f), 10.f);
}

// eleven 8-bit counters in two words, so that no array is indexed by a run-time value (no scratch)
struct Hist11 {
    uint64_t lo = 0;
    uint32_t hi = 0;
    D3R_DEV void add(int bin) {
        if (bin < 8) lo += 1ull << (8 * bin);
        else hi += 1u << (8 * (bin - 8));
    }
    D3R_DEV uint32_t at(int bin) const { return bin < 8 ? (uint32_t)(lo >> (8 * bin)) & 0xFFu : (hi >> (8 * (bin - 8))) & 0xFFu; }
};

__global__ __launch_bounds__(QT) void cloud_spfh_kernel(int n, const float* __restrict__ pts, const float* __restrict__ normals, int k,
                                                       const int* __restrict__ idx, uint32_t* __restrict__ counts_out) {
    const float PI_F = 3.14159274101257324f;
    for (long long i = (long long)blockIdx.x * QT + threadIdx.x; i < n; i += (long long)gridDim.x * QT) {
        const float* p = pts + 3 * (size_t)i;
        const float* u = normals + 3 * (size_t)i;
        const float px = p[0], py = p[1], pz = p[2], ux = u[0], uy = u[1], uz = u[2];
        const bool own = finite3(px, py, pz) && normal_ok(ux, uy, uz);
        Hist11 h[3];
        uint32_t m = 0;
        for (int j = 0; j < k; ++j) {
            const int g = idx[(size_t)i * k + j];
            if (!own || g < 0 || g >= n) continue;
            const float* q = pts + 3 * (size_t)g;
            const float* nq = normals + 3 * (size_t)g;
            const float qx = q[0], qy = q[1], qz = q[2], nx = nq[0], ny = nq[1], nz = nq[2];
            if (!(finite3(qx, qy, qz) && normal_ok(nx, ny, nz))) continue;
            const float dx = __fsub_rn(qx, px), dy = __fsub_rn(qy, py), dz = __fsub_rn(qz, pz);
            const float dist = __fsqrt_rn(dist2(dx, dy, dz));
            if (!(dist > 0.f)) continue;
            const float ex = __fdiv_rn(dx, dist), ey = __fdiv_rn(dy, dist), ez = __fdiv_rn(dz, dist);      // dn
            const float phi = row3(ux, uy, uz, ex, ey, ez);
            // v = dn x u, normalised
            float vx = __fsub_rn(__fmul_rn(ey, uz), __fmul_rn(ez, uy)), vy = __fsub_rn(__fmul_rn(ez, ux), __fmul_rn(ex, uz)),
                  vz = __fsub_rn(__fmul_rn(ex, uy), __fmul_rn(ey, ux));
            const float vn = __fsqrt_rn(dist2(vx, vy, vz));
            if (!(vn > 0.f)) continue;
            vx = __fdiv_rn(vx, vn); vy = __fdiv_rn(vy, vn); vz = __fdiv_rn(vz, vn);
            // w = u x v
            const float wx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy)), wy = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz)),
                        wz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
            const float alpha = row3(vx, vy, vz, nx, ny, nz);
            const float theta = atan2f(row3(wx, wy, wz, nx, ny, nz), row3(ux, uy, uz, nx, ny, nz));
            h[0].add(bin11(alpha, -1.f, 2.f));
            h[1].add(bin11(phi, -1.f, 2.f));
            h[2].add(bin11(theta, -PI_F, __fsub_rn(PI_F, -PI_F)));
            m += 1;
        }
        // the 36 bytes of the row as nine words; every byte position is a constant after unrolling
        uint32_t* out = counts_out + (size_t)i * (SPFH_ROW / 4);
#pragma unroll
        for (int w = 0; w < SPFH_ROW / 4; ++w) {
            uint32_t word = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int pos = 4 * w + b;
                const uint32_t v = pos < FEAT ? h[pos / BINS].at(pos % BINS) : pos == FEAT ? m : 0u;
                word |= v << (8 * b);
            }
            out[w] = word;
        }
    }
}

// ---- 3. FPFH ----------------------------------------------------------------------------------------------------------------------------
D3R_DEV uint32_t byte_of(const uint32_t (&row)[SPFH_ROW / 4], int pos) { return (row[pos >> 2] >> (8 * (pos & 3))) & 0xFFu; }

D3R_DEV void load_row(const uint32_t* __restrict__ counts, int g, uint32_t (&row)[SPFH_ROW / 4]) {
#pragma unroll
    for (int w = 0; w < SPFH_ROW / 4; ++w) row[w] = counts[(size_t)g * (SPFH_ROW / 4) + w];
}

// does neighbour column j of point i contribute? its point g, its weight 1 / d2 and its pair count
D3R_DEV bool fpfh_neighbour(int n, int k, const int* __restrict__ idx, const float* __restrict__ d2, const uint32_t* __restrict__ counts, long long i, int j,
                            int* g_out, double* w_out) {
    const int g = idx[(size_t)i * k + j];
    const float d = d2[(size_t)i * k + j];
    if (g < 0 || g >= n || !(d > 0.f)) return false;
    if (((counts[(size_t)g * (SPFH_ROW / 4) + FEAT / 4] >> (8 * (FEAT & 3))) & 0xFFu) == 0u) return false;
    *g_out = g;
    *w_out = 1.0 / (double)d;
    return true;
}

__global__ __launch_bounds__(QT) void cloud_fpfh_kernel(int n, int k, const int* __restrict__ idx, const float* __restrict__ d2,
                                                       const uint32_t* __restrict__ counts, float* __restrict__ features_out) {
    for (long long i = (long long)blockIdx.x * QT + threadIdx.x; i < n; i += (long long)gridDim.x * QT) {
        double acc[FEAT];
        uint32_t row[SPFH_ROW / 4];
        load_row(counts, (int)i, row);
        const uint32_t mp = byte_of(row, FEAT);
#pragma unroll
        for (int b = 0; b < FEAT; ++b) acc[b] = mp ? (double)byte_of(row, b) / (double)mp : 0.0;
        double W = 0.0;
        for (int j = 0; j < k; ++j) {
            int g;
            double w;
            if (fpfh_neighbour(n, k, idx, d2, counts, i, j, &g, &w)) W += w;
        }
        for (int j = 0; j < k; ++j) {
            int g;
            double w;
            if (!fpfh_neighbour(n, k, idx, d2, counts, i, j, &g, &w)) continue;
            load_row(counts, g, row);
            const double wn = w / W, mq = (double)byte_of(row, FEAT);
#pragma unroll
            for (int b = 0; b < FEAT; ++b) acc[b] += wn * ((double)byte_of(row, b) / mq);
        }
        float* out = features_out + (size_t)i * FEAT;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            double s = acc[f * BINS];
#pragma unroll
            for (int b = 1; b < BINS; ++b) s += acc[f * BINS + b];
#pragma unroll
            for (int b = 0; b < BINS; ++b) out[f * BINS + b] = s > 0.0 ? (float)((acc[f * BINS + b] * 100.0) / s) : 0.f;
        }
    }
}

// ---- 4. the nearest feature: exhaustive, exact --------------------------------------------------------------------------------------------
// A workgroup owns FQ = 64 queries, one per lane, the same 64 in each of its four waves; a lane keeps its query's 33 values in registers.
// A tile of FT rows of b is staged in LDS (rows padded to 36 floats: nine 16-byte reads); wave w takes rows [w FT / 4, (w + 1) FT / 4) of
// every tile, every lane of a wave reads the same address (a broadcast, no bank conflict). Two running minima per lane (even and odd
// rows), each met in ascending row order and replaced only by a strictly smaller distance, so each holds the lowest index of its minimum;
// the minima are compared as (d2 bits, index) pairs -- d2 is a sum of squares, +0 <= d2 <= +inf, and such floats order as their bits.
// A row of b that is not all finite gets distance bits 0xFFFFFFFF, above +inf, and is never taken.
constexpr int FQ = 64, FT = 128, FW = 4, FROW = 36;

__global__ __launch_bounds__(FQ * FW) void feature_nearest_kernel(int n_a, const float* __restrict__ a, int n_b, const float* __restrict__ b,
                                                                 float* __restrict__ d2_out, int* __restrict__ idx_out) {
    __shared__ float4 tile[FT][FROW / 4];
    __shared__ uint32_t bad[FT];                                          // 0 for a finite row, 0xFFFFFFFF else
    __shared__ uint64_t merged[FW][FQ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long qi = (long long)blockIdx.x * FQ + lane;
    const long long qr = qi < n_a ? qi : (long long)n_a - 1;             // a lane past the end works on the last row and writes nothing
    float q[FEAT];
    bool q_ok = true;
#pragma unroll
    for (int c = 0; c < FEAT; ++c) {
        q[c] = a[(size_t)qr * FEAT + c];
        q_ok = q_ok && finite_f(q[c]);
    }
    uint32_t best[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    int arg[2] = {NO_INDEX, NO_INDEX};
    float* flat = (float*)&tile[0][0];
    for (int base = 0; base < n_b; base += FT) {
        const int rows = min(FT, n_b - base);
        for (int e = threadIdx.x; e < FT * FEAT; e += FQ * FW) {
            const int r = e / FEAT, c = e - r * FEAT;
            flat[r * FROW + c] = r < rows ? b[((size_t)base + r) * FEAT + c] : 0.f;
        }
        __syncthreads();
        if (threadIdx.x < FT) {
            const int r = threadIdx.x;
            bool ok = r < rows;
            for (int c = 0; c < FEAT; ++c) ok = ok && finite_f(flat[r * FROW + c]);
            bad[r] = ok ? 0u : 0xFFFFFFFFu;
        }
        __syncthreads();
        for (int r0 = wave * (FT / FW); r0 < (wave + 1) * (FT / FW); r0 += 2) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int r = r0 + s;
                float t[FROW];
#pragma unroll
                for (int v = 0; v < FROW / 4; ++v) {
                    const float4 x = tile[r][v];
                    t[4 * v] = x.x; t[4 * v + 1] = x.y; t[4 * v + 2] = x.z; t[4 * v + 3] = x.w;
                }
                float e = __fsub_rn(q[0], t[0]);
                float d = __fmul_rn(e, e);
#pragma unroll
                for (int c = 1; c < FEAT; ++c) {
                    e = __fsub_rn(q[c], t[c]);
                    d = __fadd_rn(d, __fmul_rn(e, e));
                }
                const uint32_t bits = __float_as_uint(d) | bad[r];
                if (bits < best[s]) {
                    best[s] = bits;
                    arg[s] = base + r;
                }
            }
        }
        __syncthreads();
    }
    const uint64_t k0 = ((uint64_t)best[0] << 32) | (uint32_t)arg[0], k1 = ((uint64_t)best[1] << 32) | (uint32_t)arg[1];
    merged[wave][lane] = k0 < k1 ? k0 : k1;
    __syncthreads();
    if (wave == 0 && qi < n_a) {
        uint64_t m = merged[0][lane];
#pragma unroll
        for (int w = 1; w < FW; ++w) m = merged[w][lane] < m ? merged[w][lane] : m;
        const int g = (int)(uint32_t)m;
        const bool found = q_ok && g != NO_INDEX;
        idx_out[qi] = found ? g : -1;
        d2_out[qi] = found ? __uint_as_float((uint32_t)(m >> 32)) : __uint_as_float(0x7F800000u);
    }
}

// ---- 5. Sim(3) RANSAC over correspondences -----------------------------------------------------------------------------------------------
constexpr int RND = 256;                // hypotheses of a round = the rows a scoring workgroup holds in LDS
constexpr int SPT = 256, SPL = 4, SCHUNK = SPT * SPL;     // scoring: threads, correspondences per lane, correspondences per workgroup
constexpr int MAX_HYP = 1 << 23;        // D3R_SIM3_MAX_HYPOTHESES: the rounds are the second grid dimension of the scoring kernel

struct Sim3Best {
    int h, count, n_valid, pad;
    float rows[12];
};

struct Sim3Ws {
    double* S;              // [n_hyp][12]
    float* rows;            // [n_hyp][12] = float32(S)
    int* valid;             // [n_hyp]
    int* counts;            // [n_hyp]
    Sim3Best* best;
    size_t bytes;
};

static inline Sim3Ws sim3_workspace(void* base, int n_hyp) {
    Sim3Ws w;
    Carver c(base);
    w.S = c.take<double>((size_t)n_hyp * 12);
    w.rows = c.take<float>((size_t)n_hyp * 12);
    w.valid = c.take<int>(n_hyp);
    w.counts = c.take<int>(n_hyp);
    w.best = c.take<Sim3Best>(1);
    w.bytes = c.bytes;
    return w;
}

struct Sim3Args {
    int n, n_hyp, with_scale;
    uint64_t seed;
    float thr2;
    double ratio_min;
    const float* p;
    const float* q;
};

D3R_DEV double len3(const double* a, const double* b) {
    const double x = b[0] - a[0], y = b[1] - a[1], z = b[2] - a[2];
    return sqrt((x * x + y * y) + z * z);
}

__global__ __launch_bounds__(RND) void sim3_hyp_kernel(const Sim3Args a, const Sim3Ws w) {
    const int h = blockIdx.x * RND + threadIdx.x;
    if (h >= a.n_hyp) return;
    w.counts[h] = 0;
    int i[3];
    bool ok = ransac::draw_distinct(a.seed, h, a.n, i);
    double S[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) S[c] = 0.0;
    if (ok) {
        double P[3][3], Q[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            P[0][c] = (double)a.p[(size_t)i[0] * 3 + c]; P[1][c] = (double)a.p[(size_t)i[1] * 3 + c]; P[2][c] = (double)a.p[(size_t)i[2] * 3 + c];
            Q[0][c] = (double)a.q[(size_t)i[0] * 3 + c]; Q[1][c] = (double)a.q[(size_t)i[1] * 3 + c]; Q[2][c] = (double)a.q[(size_t)i[2] * 3 + c];
        }
        // the edges 0-1, 1-2, 2-0
        const double lp[3] = {len3(P[0], P[1]), len3(P[1], P[2]), len3(P[2], P[0])}, lq[3] = {len3(Q[0], Q[1]), len3(Q[1], Q[2]), len3(Q[2], Q[0])};
        ok = lp[0] > 0.0 && lp[1] > 0.0 && lp[2] > 0.0;                  // false for a NaN too
        const double r[3] = {lq[0] / lp[0], lq[1] / lp[1], lq[2] / lp[2]};
        const double rmin = fmin(r[0], fmin(r[1], r[2])), rmax = fmax(r[0], fmax(r[1], r[2]));
        ok = ok && rmin >= a.ratio_min * rmax;
        if (!a.with_scale) ok = ok && rmin >= a.ratio_min && rmax <= 1.0 / a.ratio_min;
        const double s = a.with_scale ? ((lq[0] + lq[1]) + lq[2]) / ((lp[0] + lp[1]) + lp[2]) : 1.0;
        double Fp[9], Fq[9];
        ok = ok && vl::triangle_frame(P[0], P[1], P[2], Fp) && vl::triangle_frame(Q[0], Q[1], Q[2], Fq);
        if (ok) {
            double mp[3], mq[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                mp[c] = ((P[0][c] + P[1][c]) + P[2][c]) / 3.0;
                mq[c] = ((Q[0][c] + Q[1][c]) + Q[2][c]) / 3.0;
            }
#pragma unroll
            for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    S[rr * 4 + c] = s * ((Fq[rr * 3] * Fp[c * 3] + Fq[rr * 3 + 1] * Fp[c * 3 + 1]) + Fq[rr * 3 + 2] * Fp[c * 3 + 2]);
                S[rr * 4 + 3] = mq[rr] - ((S[rr * 4] * mp[0] + S[rr * 4 + 1] * mp[1]) + S[rr * 4 + 2] * mp[2]);
            }
#pragma unroll
            for (int c = 0; c < 12; ++c) ok = ok && fabs(S[c]) <= 1.0e300;          // finite
            ok = ok && s > 0.0;
        }
    }
#pragma unroll
    for (int c = 0; c < 12; ++c) {
        w.S[(size_t)h * 12 + c] = ok ? S[c] : 0.0;
        w.rows[(size_t)h * 12 + c] = ok ? (float)S[c] : 0.f;
    }
    w.valid[h] = ok ? 1 : 0;
}

// p' = float32(S) p by the row product of d3r_cloud_transform, d2 to q as in the cloud metrics
D3R_DEV bool sim3_inlier(const float* m, float px, float py, float pz, float qx, float qy, float qz, float thr2) {
    const float x = affine_row(m, px, py, pz), y = affine_row(m + 4, px, py, pz), z = affine_row(m + 8, px, py, pz);
    return dist2(__fsub_rn(x, qx), __fsub_rn(y, qy), __fsub_rn(z, qz)) <= thr2;          // false for a NaN
}

__global__ __launch_bounds__(SPT) void sim3_score_kernel(const Sim3Args a, const Sim3Ws w) {
    __shared__ int any_valid;
    const int h0 = blockIdx.y * RND, p0 = blockIdx.x * SCHUNK, n_slots = min(RND, a.n_hyp - h0);
    if (threadIdx.x == 0) any_valid = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < n_slots; t += SPT)
        if (w.valid[h0 + t]) any_valid = 1;                               // every writer stores the same value
    __syncthreads();
    if (!any_valid) return;
    float px[SPL], py[SPL], pz[SPL], qx[SPL], qy[SPL], qz[SPL];
    bool live[SPL];
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int i = p0 + k * SPT + threadIdx.x;
        const int j = i < a.n ? i : 0;
        const float* p = a.p + (size_t)j * 3;
        const float* q = a.q + (size_t)j * 3;
        live[k] = i < a.n && finite3(p) && finite3(q);
        px[k] = p[0]; py[k] = p[1]; pz[k] = p[2];
        qx[k] = q[0]; qy[k] = q[1]; qz[k] = q[2];
    }
    ransac::score_round<SPT, SPL, RND>(w.rows + (size_t)h0 * 12, w.valid + h0, n_slots, w.counts + h0, [&](const float* row, int k) {
        return live[k] && sim3_inlier(row, px[k], py[k], pz[k], qx[k], qy[k], qz[k], a.thr2);
    });
}

__global__ __launch_bounds__(QT) void sim3_select_kernel(const Sim3Args a, const Sim3Ws w, double* __restrict__ best_out) {
    const ransac::Winner b = ransac::select_winner<QT>(a.n_hyp, w.valid, w.counts, 3);
    if (threadIdx.x != 0) return;
    const bool found = b.h >= 0;
    w.best->h = b.h;
    w.best->count = b.count;
    w.best->n_valid = b.n_valid;
    best_out[0] = (double)b.h;
    best_out[1] = (double)b.count;
    best_out[2] = (double)b.n_valid;
    for (int c = 0; c < 12; ++c) {
        best_out[3 + c] = found ? w.S[(size_t)b.h * 12 + c] : 0.0;
        w.best->rows[c] = found ? w.rows[(size_t)b.h * 12 + c] : 0.f;
    }
}

__global__ __launch_bounds__(QT) void sim3_mask_kernel(const Sim3Args a, const Sim3Ws w, uint8_t* __restrict__ inliers_out) {
    float m[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) m[c] = w.best->rows[c];
    ransac::write_mask<QT>(a.n, w.best->h >= 0, inliers_out, [&](long long i) {
        const float* p = a.p + (size_t)i * 3;
        const float* q = a.q + (size_t)i * 3;
        return finite3(p) && finite3(q) && sim3_inlier(m, p[0], p[1], p[2], q[0], q[1], q[2], a.thr2);
    });
}

}  // namespace cloud
}  // namespace d3r

using namespace d3r::cloud;

extern "C" int d3r_cloud_grid_heads(int n_ref, int* indices_out, int* count_out, void* workspace, void* stream) {
    if (!fuse_shape_ok(1, n_ref, n_ref) || !indices_out || !count_out || !workspace) return D3R_ERR_INVALID;
    const CloudWorkspace w = cloud_workspace(workspace, n_ref, 1);       // the layout in front of the query buffers does not depend on n_query
    hipLaunchKernelGGL(cloud_grid_heads_kernel, dim3(cloud_blocks(n_ref)), dim3(QT), 0, (hipStream_t)stream, w.pts4, w.cell_start, w.ref.n_dev, n_ref,
                       indices_out, count_out);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_cloud_spfh(int n, const float* points, const float* normals, int k, const int* idx, uint8_t* counts_out, void* stream) {
    if (n <= 0 || !points || !normals || k < 1 || k > D3R_CLOUD_MAX_K || !idx || !counts_out || ((uintptr_t)counts_out & 3)) return D3R_ERR_INVALID;
    hipLaunchKernelGGL(cloud_spfh_kernel, dim3(cloud_blocks(n)), dim3(QT), 0, (hipStream_t)stream, n, points, normals, k, idx, (uint32_t*)counts_out);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_cloud_fpfh(int n, int k, const int* idx, const float* d2, const uint8_t* counts, float* features_out, void* stream) {
    if (n <= 0 || k < 1 || k > D3R_CLOUD_MAX_K || !idx || !d2 || !counts || ((uintptr_t)counts & 3) || !features_out) return D3R_ERR_INVALID;
    hipLaunchKernelGGL(cloud_fpfh_kernel, dim3(cloud_blocks(n)), dim3(QT), 0, (hipStream_t)stream, n, k, idx, d2, (const uint32_t*)counts, features_out);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_feature_nearest(int n_a, const float* a, int n_b, const float* b, float* d2_out, int* idx_out, void* stream) {
    if (n_a <= 0 || n_b <= 0 || !a || !b || !d2_out || !idx_out) return D3R_ERR_INVALID;
    hipLaunchKernelGGL(feature_nearest_kernel, dim3((unsigned)d3r::tiles_of(n_a, FQ)), dim3(FQ * FW), 0, (hipStream_t)stream, n_a, a, n_b, b, d2_out, idx_out);
    return rc_of(hipGetLastError());
}

static bool sim3_sizes_ok(int n_corr, int n_hyp) { return n_corr >= 3 && n_hyp >= 1 && n_hyp <= MAX_HYP; }

extern "C" size_t d3r_sim3_ransac_workspace_bytes(int n_corr, int n_hyp) {
    if (!sim3_sizes_ok(n_corr, n_hyp)) return 0;
    return sim3_workspace(nullptr, n_hyp).bytes;
}

extern "C" int d3r_sim3_ransac(int n_corr, const float* p, const float* q, unsigned long long seed, int n_hyp, float thr, double ratio_min, int with_scale,
                               double* best_out, uint8_t* inliers_out, void* workspace, void* stream) {
    if (!sim3_sizes_ok(n_corr, n_hyp) || !p || !q || !best_out || !inliers_out || !workspace) return D3R_ERR_INVALID;
    const float thr2 = thr * thr;                                         // host code of a file built without contraction: one fp32 product
    if (!(thr > 0.f && thr2 <= 3.4028234e38f) || !(ratio_min > 0.0 && ratio_min <= 1.0) || (with_scale != 0 && with_scale != 1)) return D3R_ERR_INVALID;
    Sim3Args a;
    a.n = n_corr; a.n_hyp = n_hyp; a.with_scale = with_scale; a.seed = seed; a.thr2 = thr2; a.ratio_min = ratio_min; a.p = p; a.q = q;
    const Sim3Ws w = sim3_workspace(workspace, n_hyp);
    hipStream_t st = (hipStream_t)stream;
    const int rounds = (int)d3r::tiles_of(n_hyp, RND);
    hipLaunchKernelGGL(sim3_hyp_kernel, dim3(rounds), dim3(RND), 0, st, a, w);
    hipLaunchKernelGGL(sim3_score_kernel, dim3((unsigned)d3r::tiles_of(n_corr, SCHUNK), rounds), dim3(SPT), 0, st, a, w);
    hipLaunchKernelGGL(sim3_select_kernel, dim3(1), dim3(QT), 0, st, a, w, best_out);
    hipLaunchKernelGGL(sim3_mask_kernel, dim3(cloud_blocks(n_corr)), dim3(QT), 0, st, a, w, inliers_out);
    return rc_of(hipGetLastError());
}
