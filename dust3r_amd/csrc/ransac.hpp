// dust3r_amd -- what the three RANSACs share (PnP in visloc.hip, Sim(3) over correspondences in cloud_features.hip, planes of a cloud in
// cloud_planes.hip): the counter-based sampler and the scoring of one round of hypotheses; the two over clouds also the selection of the winner
// and the loop that writes its mask. Each file keeps its solver, its inlier test (compiled with its own flags) and its loads.
#pragma once
#include "common.hpp"

namespace d3r {
namespace ransac {

// splitmix64 finaliser: a bijective 64-bit mix, the counter-based generator's only state is its argument
__host__ __device__ inline uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the c-th draw of hypothesis h of a job keyed by `seed`: uniform in [0, n) (multiply-high, bias < n / 2^32)
__host__ __device__ inline int draw_index(uint64_t seed, int h, int c, int n) {
    const uint64_t r = mix64(mix64(seed ^ (0xD1B54A32D192ED03ull * (uint64_t)(h + 1))) + (uint64_t)c);
    return (int)(((r >> 32) * (uint64_t)n) >> 32);
}

// K distinct indices in [0, n), n >= K: the first K distinct of at most 64 draws, in the order drawn, -1 behind them and false if 64 draws did
// not give K (never at the sizes RANSAC meets). Every index of idx[] is a constant after unrolling, so that nothing lands in scratch on the GPU.
template <int K> __host__ __device__ inline bool draw_distinct(uint64_t seed, int h, int n, int (&idx)[K]) {
#pragma unroll
    for (int s = 0; s < K; ++s) idx[s] = -1;
    for (int c = 0; c < 64 && idx[K - 1] < 0; ++c) {
        const int k = draw_index(seed, h, c, n);
        bool open = true;                                                 // not drawn before, not placed yet
#pragma unroll
        for (int s = 0; s < K; ++s) {
            if (open && idx[s] < 0) idx[s] = k;                           // the first free slot: every earlier one differs from k
            open = open && idx[s] != k;
        }
    }
    return idx[K - 1] >= 0;
}

// One round of RND hypotheses scored against the PPL points per lane that the calling workgroup of NT threads holds in registers. The round's
// fp32 rows [RND][12] and valid flags [RND] come from global memory, the slots from n_slots on do not exist (nothing is read). inlier(row, k): is
// the lane's point k an inlier of these 12 values (false for a lane without a point k). Rows and flags go to LDS; per valid hypothesis every wave
// counts by ballot and popcount, lane 0 adds to LDS, the non-zero counts go to counts[0, RND) by integer atomics (order-free). Once per kernel.
template <int NT, int PPL, int RND, class Inlier>
D3R_DEV void score_round(const float* __restrict__ round_rows, const int* __restrict__ round_valid, int n_slots, int* __restrict__ counts, Inlier inlier) {
    __shared__ float rows[RND][12];
    __shared__ int valid[RND];
    __shared__ int cnt[RND];
    for (int t = threadIdx.x; t < RND * 12; t += NT) rows[t / 12][t % 12] = t / 12 < n_slots ? round_rows[t] : 0.f;
    for (int t = threadIdx.x; t < RND; t += NT) {
        valid[t] = t < n_slots ? round_valid[t] : 0;
        cnt[t] = 0;
    }
    __syncthreads();
    for (int h = 0; h < RND; ++h) {
        if (!valid[h]) continue;                                          // the same for every lane
        int c = 0;
#pragma unroll
        for (int k = 0; k < PPL; ++k) c += __popcll(__ballot(inlier(rows[h], k)));
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&cnt[h], c);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < RND; t += NT)
        if (cnt[t]) atomicAdd(&counts[t], cnt[t]);
}

// ---- what the two RANSACs over clouds (Sim(3) in cloud_features.hip, planes in cloud_planes.hip) share behind the scoring -------------------
// (count, lowest h) as one key: the larger key wins
D3R_DEV uint64_t winner_key(int count, int h) { return ((uint64_t)(uint32_t)count << 32) | (uint32_t)(0x7FFFFFFF - h); }

struct Winner {
    int h, count, n_valid;              // h = -1 and count = 0 when no valid hypothesis has min_count inliers
};

// One workgroup of NT threads (a power of two) selects among n_hyp scored hypotheses: the valid one with the largest count, among equals
// the lowest h. A maximum over integer keys: the same whatever the order. Every thread gets the result. Once per kernel (it owns its LDS).
template <int NT> D3R_DEV Winner select_winner(int n_hyp, const int* __restrict__ valid, const int* __restrict__ counts, int min_count) {
    __shared__ uint64_t keys[NT];
    __shared__ int nv[NT];
    uint64_t key = 0;                                                     // below every valid hypothesis's key (h <= 0x7FFFFFFF - 1 there)
    int n_valid = 0;
    for (int h = threadIdx.x; h < n_hyp; h += NT) {
        if (!valid[h]) continue;
        n_valid += 1;
        const uint64_t kh = winner_key(counts[h], h);
        key = kh > key ? kh : key;
    }
    keys[threadIdx.x] = key;
    nv[threadIdx.x] = n_valid;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            keys[threadIdx.x] = keys[threadIdx.x + o] > keys[threadIdx.x] ? keys[threadIdx.x + o] : keys[threadIdx.x];
            nv[threadIdx.x] += nv[threadIdx.x + o];
        }
        __syncthreads();
    }
    const int count = (int)(keys[0] >> 32);
    const bool found = nv[0] > 0 && count >= min_count;
    Winner w;
    w.h = found ? 0x7FFFFFFF - (int)(uint32_t)keys[0] : -1;
    w.count = found ? count : 0;
    w.n_valid = nv[0];
    return w;
}

// the winner's mask over n rows, grid-stride with NT threads: out[i] = found && inlier(i)
template <int NT, class Inlier> D3R_DEV void write_mask(long long n, bool found, uint8_t* __restrict__ out, Inlier inlier) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) out[i] = found && inlier(i);
}

}  // namespace ransac
}  // namespace d3r
