// dust3r_amd -- forward-only evaluation of the reference's regression criteria (dust3r/losses.py:158-194 Regr3D, :220-238 ConfLoss,
// :245-294 Regr3D_ShiftInv / _ScaleInv / _ScaleShiftInv with dust3r/utils/geometry.py:249-342 normalize_pointcloud,
// get_joint_pointcloud_depth, get_joint_pointcloud_center_scale) for B pairs in one call. No gradients exist here.
//
// Every pass streams the RAW inputs of both views (ground truth 12 B, prediction 12 B, mask 1 B, in the last pass confidence 4 B per
// pixel) and recomputes the transformed points from the per-pair statistics found so far; nothing per pixel is kept between passes
// (no NaN-padded concatenation, no scratch array of keys). Passes of one call, all enqueued on one stream without a host round trip:
//   prep            valid counts (after dist_clip) and the sums of f(|p|) of the avg_* / sqrt_dis normalisation
//   3 x select      per joint median: radix select over the order-preserving 32-bit key of the fp32 value, digits of 11 / 11 / 10 bits.
//                   A pass builds one LDS histogram per workgroup and per selection, merges it into the pair's global histogram with
//                   INTEGER atomics (order independent), and a small scan kernel picks the digit that holds rank (n - 1) / 2: the lower
//                   median torch.nanmedian returns. Selections that share inputs run together: {prediction, ground truth} for the
//                   median_dis factor, the z shift and the scale, {x, y, z} x {prediction, ground truth} for the centre.
//   loss            per-pixel Euclidean distance, confidence weighting, optional dense maps
// Floating-point sums: fp64 per lane, a fixed shuffle / LDS tree per workgroup, one partial per workgroup, added in workgroup order by
// the reduce kernels. The grid of a pair depends on H x W only, so a pair's outputs do not depend on its neighbours in the batch.
// Non-finite values at VALID pixels are outside the contract (a NaN would be keyed like a large number).
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "reduce.hpp"
#include <algorithm>

namespace d3r {
namespace losses {

constexpr int NT = 256;          // threads per workgroup
constexpr int MAXGX = 64;        // workgroups per (pair, view): 1024 pixels per workgroup and sweep, grid-stride beyond
constexpr int BINS = 2048;       // 11-bit digits (the last one has 10)
constexpr int MAXSEL = 6;        // selections of one pass: {x, y, z} x {prediction, ground truth}
constexpr int NSTAT = D3R_CRIT_NSTAT;
constexpr uint32_t EMPTY = 0xFFFFFFFFu;

enum { M_PREP = 0, M_SEL_NORM, M_SEL_SHIFT, M_SEL_CENTER, M_SEL_SCALE, M_LOSS };
enum { A_NORM_PR = 1, A_NORM_GT = 2, A_WARP = 4, A_SHIFT = 8, A_SCALE_MUL = 16, A_SCALE_DIV = 32, A_NO_CENTER = 64 };

// order-preserving key of a float: negative values complemented, the others get the top bit (-0 sorts just below +0)
D3R_DEV uint32_t key_of(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
D3R_DEV float val_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
D3R_DEV int digit_shift(int d) { return d == 0 ? 21 : (d == 1 ? 10 : 0); }
D3R_DEV uint32_t digit_hmask(int d) { return d == 0 ? 0u : (d == 1 ? 0xFFE00000u : 0xFFFFFC00u); }
D3R_DEV uint32_t digit_bins(int d) { return d == 2 ? 1024u : 2048u; }

struct Args {
    const float *gt1, *gt2, *pr1, *pr2, *conf1, *conf2, *pose;
    const uint8_t *m1, *m2;
    double* out;            // [B][NSTAT]
    double* partial;        // [B][2][MAXGX][4]
    uint32_t* hist;         // [B][MAXSEL][BINS]
    uint32_t* sel;          // [B][MAXSEL][2]: prefix, rank
    float *map1, *map2;
    int N, norm_mode, has_clip, digit;
    unsigned apply;
    float clip, alpha;
};

// the per-pair statistics a pass applies (fp32, as the reference holds them)
struct St {
    float nf[2], sh[2], c[2][3], sc[2], mul;
};
D3R_DEV St load_st(const double* o) {
    St s;
    s.nf[0] = (float)o[D3R_CRIT_NORM_PR]; s.nf[1] = (float)o[D3R_CRIT_NORM_GT];
    s.sh[0] = (float)o[D3R_CRIT_SHIFT_PR]; s.sh[1] = (float)o[D3R_CRIT_SHIFT_GT];
    for (int k = 0; k < 3; ++k) {
        s.c[0][k] = (float)o[D3R_CRIT_CENTER_PR + k];
        s.c[1][k] = (float)o[D3R_CRIT_CENTER_GT + k];
    }
    s.sc[0] = fminf(fmaxf((float)o[D3R_CRIT_SCALE_PR], 1e-3f), 1e3f);      // losses.py:280
    s.sc[1] = (float)o[D3R_CRIT_SCALE_GT];
    s.mul = s.sc[1] / s.sc[0];
    return s;
}

// side 0 = prediction, 1 = ground truth (already in view 1's camera frame)
D3R_DEV void xform(float& x, float& y, float& z, int side, const St& s, unsigned ap) {
    if (ap & (side ? A_NORM_GT : A_NORM_PR)) {
        if (ap & A_WARP) {
            const float d = sqrtf(x * x + y * y + z * z);
            const float w = log1pf(d) / fmaxf(d, 1e-8f);
            x *= w; y *= w; z *= w;
        }
        const float f = s.nf[side];
        x /= f; y /= f; z /= f;
    }
    if (ap & A_SHIFT) z -= s.sh[side];
    if (ap & A_SCALE_MUL) {
        if (side == 0) { x *= s.mul; y *= s.mul; z *= s.mul; }
    } else if (ap & A_SCALE_DIV) {
        const float f = s.sc[side];
        x /= f; y /= f; z /= f;
    }
}

// four consecutive pixels of a [N][3] array: three 16-byte loads when the layout allows
template <bool VEC> D3R_DEV void load_pts4(const float* base, int p0, int N, float (&v)[12]) {
    if constexpr (VEC) {
        const float4* q = reinterpret_cast<const float4*>(base + 3 * (size_t)p0);
        const float4 a = q[0], b = q[1], c = q[2];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = p0 + k < N;
#pragma unroll
            for (int j = 0; j < 3; ++j) v[3 * k + j] = in ? base[3 * (size_t)(p0 + k) + j] : 0.f;
        }
    }
}
template <bool VEC> D3R_DEV uint32_t load_mask4(const uint8_t* m, int p0, int N) {
    if constexpr (VEC) {
        return *reinterpret_cast<const uint32_t*>(m + p0);
    } else {
        uint32_t r = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) r |= (p0 + k < N && m[p0 + k]) ? (0xFFu << (8 * k)) : 0u;
        return r;
    }
}
template <bool VEC> D3R_DEV void load_f4(const float* base, int p0, int N, float (&v)[4]) {
    if constexpr (VEC) {
        const float4 a = *reinterpret_cast<const float4*>(base + p0);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p0 + k < N ? base[p0 + k] : 0.f;
    }
}
template <bool VEC> D3R_DEV void store_f4(float* base, int p0, int N, const float (&v)[4]) {
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(base + p0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (p0 + k < N) base[p0 + k] = v[k];
    }
}

D3R_DEV void hist_add(uint32_t* lh, int s, uint32_t key, uint32_t prefix, uint32_t hmask, int shift, uint32_t bmask) {
    if ((key & hmask) == prefix) atomicAdd(&lh[s * BINS + ((key >> shift) & bmask)], 1u);
}
// merge the workgroup's LDS histograms into the pair's (integer atomics: the result does not depend on arrival order)
D3R_DEV void hist_flush(const uint32_t* lh, uint32_t* gh, int n) {
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += NT) {
        const uint32_t c = lh[i];
        if (c) atomicAdd(&gh[i], c);
    }
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(NT) void pass_kernel(const Args a) {
    constexpr bool SELECT = MODE >= M_SEL_NORM && MODE <= M_SEL_SCALE;
    constexpr int S = MODE == M_SEL_CENTER ? 6 : (SELECT ? 2 : 0);
    constexpr int C = S / 2;                   // selections per side
    __shared__ uint32_t lh[SELECT ? S * BINS : 1];
    __shared__ double red[NT / 64 * 3];
    const int b = blockIdx.y, v = blockIdx.z, N = a.N;
    const float* gt = (v ? a.gt2 : a.gt1) + (size_t)b * N * 3;
    const float* pr = (v ? a.pr2 : a.pr1) + (size_t)b * N * 3;
    const uint8_t* mk = (v ? a.m2 : a.m1) + (size_t)b * N;
    const float* P = a.pose + (size_t)b * 16;
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = P[k];
    const St st = load_st(a.out + (size_t)b * NSTAT);
    const unsigned ap = a.apply;

    uint32_t prefix[S > 0 ? S : 1];
    const int shift = digit_shift(a.digit);
    const uint32_t hmask = digit_hmask(a.digit), bmask = digit_bins(a.digit) - 1u;
    if constexpr (SELECT) {
        for (int i = threadIdx.x; i < S * BINS; i += NT) lh[i] = 0u;
#pragma unroll
        for (int s = 0; s < S; ++s) prefix[s] = a.digit == 0 ? 0u : a.sel[((size_t)b * MAXSEL + s) * 2];
        __syncthreads();
    }
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;

    for (int p0 = (blockIdx.x * NT + threadIdx.x) * 4; p0 < N; p0 += gridDim.x * NT * 4) {
        const uint32_t m4 = load_mask4<VEC>(mk, p0, N);
        float g[12], q[12], cf[4] = {1.f, 1.f, 1.f, 1.f}, lmap[4];
        load_pts4<VEC>(gt, p0, N, g);
        load_pts4<VEC>(pr, p0, N, q);
        if constexpr (MODE == M_LOSS) {
            const float* conf = v ? a.conf2 : a.conf1;
            if (conf) load_f4<VEC>(conf + (size_t)b * N, p0, N, cf);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // ground truth into view 1's camera frame (losses.py:160-162)
            const float wx = g[3 * k], wy = g[3 * k + 1], wz = g[3 * k + 2];
            float gx = T[0] * wx + T[1] * wy + T[2] * wz + T[3];
            float gy = T[4] * wx + T[5] * wy + T[6] * wz + T[7];
            float gz = T[8] * wx + T[9] * wy + T[10] * wz + T[11];
            float px = q[3 * k], py = q[3 * k + 1], pz = q[3 * k + 2];
            bool valid = (m4 >> (8 * k)) & 0xFFu;
            if (a.has_clip) valid = valid && sqrtf(gx * gx + gy * gy + gz * gz) <= a.clip;      // losses.py:167-172
            if constexpr (MODE == M_LOSS) lmap[k] = 0.f;
            if (!valid) continue;
            if constexpr (MODE == M_PREP) {
                float dp = sqrtf(px * px + py * py + pz * pz), dg = sqrtf(gx * gx + gy * gy + gz * gz);
                if (a.norm_mode == D3R_NORM_AVG_LOG1P || a.norm_mode == D3R_NORM_AVG_WARP_LOG1P) { dp = log1pf(dp); dg = log1pf(dg); }
                else if (a.norm_mode == D3R_NORM_SQRT_DIS) { dp = sqrtf(dp); dg = sqrtf(dg); }
                acc0 += (double)dp; acc1 += (double)dg; acc2 += 1.0;
            } else {
                xform(px, py, pz, 0, st, ap);
                xform(gx, gy, gz, 1, st, ap);
                if constexpr (MODE == M_SEL_NORM) {
                    hist_add(lh, 0, key_of(sqrtf(px * px + py * py + pz * pz)), prefix[0], hmask, shift, bmask);
                    hist_add(lh, 1, key_of(sqrtf(gx * gx + gy * gy + gz * gz)), prefix[1], hmask, shift, bmask);
                } else if constexpr (MODE == M_SEL_SHIFT) {
                    hist_add(lh, 0, key_of(pz), prefix[0], hmask, shift, bmask);
                    hist_add(lh, 1, key_of(gz), prefix[1], hmask, shift, bmask);
                } else if constexpr (MODE == M_SEL_CENTER) {
                    hist_add(lh, 0, key_of(px), prefix[0], hmask, shift, bmask);
                    hist_add(lh, 1, key_of(py), prefix[1], hmask, shift, bmask);
                    hist_add(lh, 2, key_of(pz), prefix[2], hmask, shift, bmask);
                    hist_add(lh, 3, key_of(gx), prefix[3], hmask, shift, bmask);
                    hist_add(lh, 4, key_of(gy), prefix[4], hmask, shift, bmask);
                    hist_add(lh, 5, key_of(gz), prefix[5], hmask, shift, bmask);
                } else if constexpr (MODE == M_SEL_SCALE) {
                    if (!(ap & A_NO_CENTER)) {
                        px -= st.c[0][0]; py -= st.c[0][1]; pz -= st.c[0][2];
                        gx -= st.c[1][0]; gy -= st.c[1][1]; gz -= st.c[1][2];
                    }
                    hist_add(lh, 0, key_of(sqrtf(px * px + py * py + pz * pz)), prefix[0], hmask, shift, bmask);
                    hist_add(lh, 1, key_of(sqrtf(gx * gx + gy * gy + gz * gz)), prefix[1], hmask, shift, bmask);
                } else {      // M_LOSS: L21 (losses.py:57-58), confidence weighting (:231)
                    const float dx = px - gx, dy = py - gy, dz = pz - gz;
                    const float l = sqrtf(dx * dx + dy * dy + dz * dz);
                    lmap[k] = l;
                    acc0 += (double)l;
                    acc1 += (double)l * (double)cf[k] - (double)a.alpha * (double)logf(cf[k]);
                }
            }
        }
        if constexpr (MODE == M_LOSS) {
            float* map = v ? a.map2 : a.map1;
            if (map) store_f4<VEC>(map + (size_t)b * N, p0, N, lmap);
        }
    }
    (void)C;
    if constexpr (SELECT) {
        hist_flush(lh, a.hist + (size_t)b * MAXSEL * BINS, S * BINS);
    } else {
        double* part = a.partial + (((size_t)b * 2 + v) * MAXGX + blockIdx.x) * 4;
        // The workgroup's three sums in reduce.hpp's fixed order, in thread 0: bit for bit what a __shfl_down ladder 32..1 read in lane 0 (the
        // butterfly's tree for lane 0) and a combine started from 0.0 give, since every accumulator starts at +0.0 and an IEEE sum is -0.0
        // only when both operands are.
        double acc[3] = {acc0, acc1, acc2};
        block_reduce_gather<NT, false>(acc, red, Sum());
        if (threadIdx.x == 0) { part[0] = acc[0]; part[1] = acc[1]; part[2] = acc[2]; part[3] = 0.0; }
    }
}

// joint masked median of plain value rows (the export tests and get_joint_pointcloud_depth use): one selection per row; a NaN counts as masked
template <bool VEC>
__global__ __launch_bounds__(NT) void raw_select_kernel(const float* __restrict__ v1, const float* __restrict__ v2, const uint8_t* __restrict__ m1,
                                                        const uint8_t* __restrict__ m2, int N, uint32_t* __restrict__ hist,
                                                        const uint32_t* __restrict__ sel, int digit) {
    __shared__ uint32_t lh[BINS];
    const int b = blockIdx.y, v = blockIdx.z;
    const float* vals = (v ? v2 : v1) + (size_t)b * N;
    const uint8_t* mk = v ? m2 : m1;
    for (int i = threadIdx.x; i < BINS; i += NT) lh[i] = 0u;
    const uint32_t prefix = digit == 0 ? 0u : sel[(size_t)b * MAXSEL * 2];
    const int shift = digit_shift(digit);
    const uint32_t hmask = digit_hmask(digit), bmask = digit_bins(digit) - 1u;
    __syncthreads();
    for (int p0 = (blockIdx.x * NT + threadIdx.x) * 4; p0 < N; p0 += gridDim.x * NT * 4) {
        const uint32_t m4 = mk ? load_mask4<VEC>(mk + (size_t)b * N, p0, N) : 0xFFFFFFFFu;
        float x[4];
        load_f4<VEC>(vals, p0, N, x);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (((m4 >> (8 * k)) & 0xFFu) && p0 + k < N && x[k] == x[k]) hist_add(lh, 0, key_of(x[k]), prefix, hmask, shift, bmask);
    }
    hist_flush(lh, hist + (size_t)b * MAXSEL * BINS, BINS);
}

// One workgroup per (selection, pair): find the digit that holds the wanted rank, narrow the prefix, clear the histogram for the next pass.
// digit 0 also fixes the rank: (n - 1) / 2 of the n keyed values, the element torch.nanmedian returns; n = 0 yields NaN. After the last digit
// the selected value goes to out[b * out_stride + slot_base + s]; fin: 1 = clipped below at 1e-8 (norm factor), 2 = x and y centres zeroed (z_only).
__global__ __launch_bounds__(256) void scan_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ sel, double* __restrict__ out, int digit,
                                                   int slot_base, int fin, int out_stride) {
    __shared__ uint32_t tsum[256];
    __shared__ uint32_t all;
    const int s = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    uint32_t* h = hist + ((size_t)b * MAXSEL + s) * BINS;
    uint32_t* state = sel + ((size_t)b * MAXSEL + s) * 2;
    uint32_t c[8], mine = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c[k] = h[t * 8 + k];
        mine += c[k];
        h[t * 8 + k] = 0u;
    }
    tsum[t] = mine;
    __syncthreads();
    if (t == 0) {               // exclusive prefix of the 256 thread counts
        uint32_t run = 0;
        for (int i = 0; i < 256; ++i) { const uint32_t x = tsum[i]; tsum[i] = run; run += x; }
        all = run;
    }
    __syncthreads();
    uint32_t prefix = digit == 0 ? 0u : state[0];
    uint32_t rank = digit == 0 ? (all == 0u ? EMPTY : (all - 1u) / 2u) : state[1];
    __syncthreads();            // every thread has read the state before one rewrites it
    if (rank == EMPTY) {
        if (t == 0) {
            state[0] = 0u; state[1] = EMPTY;
            if (digit == 2) out[(size_t)b * out_stride + slot_base + s] = (double)__uint_as_float(0x7FC00000u);
        }
        return;
    }
    const uint32_t before = tsum[t];
    if (rank >= before && rank < before + mine) {
        uint32_t run = before, lo = before;
        int bin = t * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (rank >= run) { bin = t * 8 + k; lo = run; }      // the last bin that starts at or below the rank and is not empty past it
            run += c[k];
        }
        rank -= lo;
        prefix |= (uint32_t)bin << digit_shift(digit);
        state[0] = prefix; state[1] = rank;
        if (digit == 2) {
            float val = val_of(prefix);
            if (fin == 1) val = val < 1e-8f ? 1e-8f : val;
            if (fin == 2 && (s % 3) != 2) val = 0.f;
            out[(size_t)b * out_stride + slot_base + s] = (double)val;
        }
    }
}

// partial[b][v][blk][k] added in workgroup order (8 threads: one per view and slot), then the pair's statistics
__global__ __launch_bounds__(64) void reduce_kernel(const double* __restrict__ partial, double* __restrict__ out, int gx, int nviews, int loss_pass,
                                                    int norm_mode, int norm_gt) {
    __shared__ double s[8];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < 8) {
        const int v = t >> 2, k = t & 3;
        double r = 0.0;
        if (v < nviews)
            for (int i = 0; i < gx; ++i) r += partial[(((size_t)b * 2 + v) * MAXGX + i) * 4 + k];
        s[t] = r;
    }
    __syncthreads();
    if (t != 0) return;
    double* o = out + (size_t)b * NSTAT;
    if (loss_pass) {
        o[D3R_CRIT_SUM_L1] = s[0]; o[D3R_CRIT_SUM_L2] = s[4]; o[D3R_CRIT_SUM_CONF1] = s[1]; o[D3R_CRIT_SUM_CONF2] = s[5];
        return;
    }
    for (int k = 0; k < NSTAT; ++k) o[k] = 0.0;
    const double n1 = s[2], n2 = s[6], n = n1 + n2;
    o[D3R_CRIT_N1] = n1; o[D3R_CRIT_N2] = n2;
    double fp = 1.0, fg = 1.0;
    if (norm_mode == D3R_NORM_AVG_DIS || norm_mode == D3R_NORM_AVG_LOG1P || norm_mode == D3R_NORM_AVG_WARP_LOG1P) {      // geometry.py:281, :300
        fp = fmax((s[0] + s[4]) / (n + 1e-8), 1e-8);
        fg = fmax((s[1] + s[5]) / (n + 1e-8), 1e-8);
    } else if (norm_mode == D3R_NORM_SQRT_DIS) {                                                                            // geometry.py:296
        const double a = (s[0] + s[4]) / n, g = (s[1] + s[5]) / n;
        fp = a * a; fg = g * g;
        fp = fp < 1e-8 ? 1e-8 : fp; fg = fg < 1e-8 ? 1e-8 : fg;      // NaN (n = 0) stays NaN, as torch.clip leaves it
    }
    o[D3R_CRIT_NORM_PR] = fp;
    o[D3R_CRIT_NORM_GT] = norm_gt ? fg : 1.0;
    o[D3R_CRIT_SCALE_PR] = 1.0; o[D3R_CRIT_SCALE_GT] = 1.0;
}

// median_dis leaves both factors in the slots; the ground truth's is dropped again when it keeps its own scale
__global__ void drop_gt_norm_kernel(double* out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) out[(size_t)b * NSTAT + D3R_CRIT_NORM_GT] = 1.0;
}

}  // namespace losses
}  // namespace d3r

using namespace d3r::losses;

struct LossWorkspace {
    uint32_t *hist, *sel;   // [B][MAXSEL][BINS], [B][MAXSEL][2]: zeroed at the start of a call, `clear` bytes from hist
    double* partial;        // [B][2][MAXGX][4]
    size_t clear, bytes;
};
static LossWorkspace loss_workspace(void* base, int B) {
    LossWorkspace w;
    d3r::Carver c(base);
    w.hist = c.take<uint32_t>((size_t)B * MAXSEL * BINS);
    w.sel = c.take<uint32_t>((size_t)B * MAXSEL * 2);
    w.clear = c.bytes;
    w.partial = c.take<double>((size_t)B * 2 * MAXGX * 4);
    w.bytes = c.bytes;
    return w;
}
static int grid_x(int N) { return (int)std::min<long long>(((long long)N + NT * 4 - 1) / (NT * 4), MAXGX); }
static bool aligned(const void* p, size_t a) { return ((size_t)p % a) == 0; }

extern "C" size_t d3r_pair_criterion_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return loss_workspace(nullptr, B).bytes;
}

extern "C" int d3r_pair_criterion_passes(const d3r_criterion_opts* o) {
    if (!o) return 0;
    int n = 1;
    if (o->norm_mode == D3R_NORM_MEDIAN_DIS) n += 3;
    if (o->stop_after == D3R_STAGE_NORM) return n;
    if (o->shift_inv) n += 3;
    if (o->stop_after == D3R_STAGE_SHIFT) return n;
    if (o->scale_inv) n += 6;
    if (o->stop_after == D3R_STAGE_SCALE) return n;
    return n + 1;
}

template <int MODE> static void launch_pass(const Args& a, int B, int nviews, bool vec, hipStream_t st) {
    const dim3 grid(grid_x(a.N), B, nviews);
    if (vec) hipLaunchKernelGGL((pass_kernel<MODE, true>), grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((pass_kernel<MODE, false>), grid, dim3(NT), 0, st, a);
}

template <int MODE> static void select3(Args& a, int B, int nviews, bool vec, int S, int slot_base, int fin, hipStream_t st) {
    for (int d = 0; d < 3; ++d) {
        a.digit = d;
        launch_pass<MODE>(a, B, nviews, vec, st);
        hipLaunchKernelGGL(scan_kernel, dim3(S, B), dim3(256), 0, st, a.hist, a.sel, a.out, d, slot_base, fin, NSTAT);
    }
}

extern "C" int d3r_pair_criterion(int B, int N, const float* gt_pts1, const float* gt_pts2, const float* inv_pose1, const uint8_t* valid1,
                                  const uint8_t* valid2, const float* pr_pts1, const float* pr_pts2, const float* conf1, const float* conf2,
                                  const d3r_criterion_opts* o, double* out, float* map1, float* map2, void* workspace, void* stream) {
    if (B <= 0 || B > 65535 || N <= 0 || N > (1 << 28) || !gt_pts1 || !inv_pose1 || !valid1 || !pr_pts1 || !o || !out || !workspace) return D3R_ERR_INVALID;
    const int nviews = gt_pts2 ? 2 : 1;
    if (nviews == 2 && (!valid2 || !pr_pts2)) return D3R_ERR_INVALID;
    if (o->norm_mode < D3R_NORM_NONE || o->norm_mode > D3R_NORM_SQRT_DIS || o->stop_after < D3R_STAGE_ALL || o->stop_after > D3R_STAGE_SCALE)
        return D3R_ERR_INVALID;
    if (o->use_conf && o->stop_after == D3R_STAGE_ALL && (!conf1 || (nviews == 2 && !conf2) || !(o->alpha > 0.f))) return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    Args a{};
    a.gt1 = gt_pts1; a.gt2 = gt_pts2; a.pr1 = pr_pts1; a.pr2 = pr_pts2; a.pose = inv_pose1; a.m1 = valid1; a.m2 = valid2;
    a.conf1 = o->use_conf ? conf1 : nullptr; a.conf2 = o->use_conf ? conf2 : nullptr;
    a.out = out;
    const LossWorkspace w = loss_workspace(workspace, B);
    a.hist = w.hist; a.sel = w.sel; a.partial = w.partial;
    a.map1 = map1; a.map2 = map2;
    a.N = N; a.norm_mode = o->norm_mode; a.has_clip = o->has_dist_clip; a.clip = o->dist_clip; a.alpha = o->use_conf ? o->alpha : 0.f;
    a.apply = 0u; a.digit = 0;
    // 16-byte loads: every pair's rows start on 16 bytes (masks: 4) when N % 4 == 0 and the tensors do
    bool vec = N % 4 == 0 && aligned(gt_pts1, 16) && aligned(pr_pts1, 16) && aligned(valid1, 4) && aligned(gt_pts2, 16) && aligned(pr_pts2, 16) &&
               aligned(valid2, 4) && aligned(conf1, 16) && aligned(conf2, 16) && aligned(map1, 16) && aligned(map2, 16);
    if (hipMemsetAsync(w.hist, 0, w.clear, st) != hipSuccess) return D3R_ERR_LAUNCH;
    const int gx = grid_x(N);
    const bool norm = o->norm_mode != D3R_NORM_NONE, norm_gt = norm && !o->gt_scale;

    launch_pass<M_PREP>(a, B, nviews, vec, st);
    hipLaunchKernelGGL(reduce_kernel, dim3(B), dim3(64), 0, st, a.partial, out, gx, nviews, 0, o->norm_mode, (int)norm_gt);
    if (o->norm_mode == D3R_NORM_MEDIAN_DIS) {                     // geometry.py:294
        select3<M_SEL_NORM>(a, B, nviews, vec, 2, D3R_CRIT_NORM_PR, 1, st);
        if (!norm_gt) hipLaunchKernelGGL(drop_gt_norm_kernel, dim3((B + 63) / 64), dim3(64), 0, st, out, B);
    }
    if (norm) a.apply |= A_NORM_PR | (norm_gt ? A_NORM_GT : 0u) | (o->norm_mode == D3R_NORM_AVG_WARP_LOG1P ? A_WARP : 0u);
    if (o->stop_after == D3R_STAGE_NORM) return rc_of(hipGetLastError());
    if (o->shift_inv) {                                            // losses.py:251-260
        select3<M_SEL_SHIFT>(a, B, nviews, vec, 2, D3R_CRIT_SHIFT_PR, 0, st);
        a.apply |= A_SHIFT;
    }
    if (o->stop_after == D3R_STAGE_SHIFT) return rc_of(hipGetLastError());
    if (o->scale_inv) {                                            // geometry.py:335-341, losses.py:276-291
        select3<M_SEL_CENTER>(a, B, nviews, vec, 6, D3R_CRIT_CENTER_PR, o->center_mode == D3R_CENTER_Z_ONLY ? 2 : 0, st);
        if (o->center_mode == D3R_CENTER_NONE) a.apply |= A_NO_CENTER;
        select3<M_SEL_SCALE>(a, B, nviews, vec, 2, D3R_CRIT_SCALE_PR, 0, st);
        a.apply |= o->gt_scale ? A_SCALE_MUL : A_SCALE_DIV;
    }
    if (o->stop_after == D3R_STAGE_SCALE) return rc_of(hipGetLastError());
    launch_pass<M_LOSS>(a, B, nviews, vec, st);
    hipLaunchKernelGGL(reduce_kernel, dim3(B), dim3(64), 0, st, a.partial, out, gx, nviews, 1, 0, 0);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_masked_median(int B, int N, const float* vals1, const float* vals2, const uint8_t* mask1, const uint8_t* mask2, double* out,
                                 void* workspace, void* stream) {
    if (B <= 0 || B > 65535 || N <= 0 || N > (1 << 28) || !vals1 || !out || !workspace) return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const LossWorkspace w = loss_workspace(workspace, B);
    uint32_t *hist = w.hist, *sel = w.sel;
    if (hipMemsetAsync(hist, 0, w.clear, st) != hipSuccess) return D3R_ERR_LAUNCH;
    const bool vec = N % 4 == 0 && aligned(vals1, 16) && aligned(vals2, 16) && aligned(mask1, 4) && aligned(mask2, 4);
    const dim3 grid(grid_x(N), B, vals2 ? 2 : 1);
    for (int d = 0; d < 3; ++d) {
        if (vec) hipLaunchKernelGGL(raw_select_kernel<true>, grid, dim3(NT), 0, st, vals1, vals2, mask1, mask2, N, hist, sel, d);
        else hipLaunchKernelGGL(raw_select_kernel<false>, grid, dim3(NT), 0, st, vals1, vals2, mask1, mask2, N, hist, sel, d);
        hipLaunchKernelGGL(scan_kernel, dim3(1, B), dim3(256), 0, st, hist, sel, out, d, 0, 0, 1);
    }
    return rc_of(hipGetLastError());
}
