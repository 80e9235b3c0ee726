// dust3r_amd -- the voxel grid that fuse.hip (scene.fuse()) and cloud_nn.hip (cloud-to-cloud nearest neighbours) share: stages 1-3 of
// d3r_fuse_voxels, moved here with the same arithmetic and launch sequence. What differs from the code as it stood in fuse.hip: valid_at
// takes a NULL mask; key_of is written on axis_q (one axis of the key, the same three operations), which the search kernel of cloud_knn.hip
// needs on its own; every kernel, the template included, is static, so each file that includes this header has and launches its OWN
// copies under its own host stubs -- nothing is merged across the two objects, whatever flags they are built with.
// Inputs are padded stacks (utils/padded.py): view v is elements [0, h w) of row v, flat index g = v row + e; a flat cloud of n points is
// one view of row = n with h w = n.
//   1. key and compact: fuse_flag_kernel<KEYS, false> counts the valid pixels of every tile, fuse_scan_kernel scans the tile counts,
//      fuse_flag_kernel<KEYS, true> places (key, g) of every valid pixel, view then raster order;
//      key = q_x | q_y << bits_x | q_z << (bits_x + bits_y), q_c = (int)floorf((p_c - lo_c) / voxel) in fp32
//   2. stable LSD radix sort by key, 4 bits per pass, over bits_x + bits_y + bits_z bits only. Per pass three launches: fuse_hist_kernel
//      (per tile of SUB x 1024 pairs the count of each digit, digit-major), fuse_scan_kernel over the 16 x tiles counts,
//      fuse_scatter_kernel (rank inside the tile from wave ballots, tiles in order)
//   3. segment heads: key[i] != key[i - 1], compacted with the pattern of stage 1 (fuse_flag_kernel<HEADS, ...>)
// No kernel waits on another workgroup: every scan over tiles is a launch of its own (ONE workgroup, chunks in order), there is no
// atomic, no look-back, no grid barrier. Integer placement only: the same bytes on every run. The workspace's carving and the grid
// arithmetic (tiles_of / blocks_of, capped at MAX_BLOCKS here) are reduce.hpp's.
#pragma once
#include <algorithm>
#include "common.hpp"
#include "scene_common.hpp"

namespace d3r {
namespace fuse {

using namespace d3r::scene;

constexpr int SUB = 4;                  // sub-tiles of NT pairs per sort tile: a quarter of the histogram rows to scan
constexpr int DIGIT_BITS = 4, DIGITS = 16;
constexpr int WAVES = NT / 64;
constexpr int MAX_BLOCKS = 2048;        // grid cap of the tile kernels (grid-stride beyond)

D3R_DEV bool finite_f(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7F800000u) != 0x7F800000u; }

// ---- the fp32 3-vector arithmetic of the cloud kernels, each operation rounded on its own whatever the including file's flags: a point has
// three finite coordinates, a usable normal is finite and not zero
D3R_DEV bool finite3(float x, float y, float z) { return finite_f(x) && finite_f(y) && finite_f(z); }
D3R_DEV bool finite3(const float* p) { return finite_f(p[0]) && finite_f(p[1]) && finite_f(p[2]); }      // reads p[1], p[2] only as far as needed
D3R_DEV bool normal_ok(float x, float y, float z) { return finite3(x, y, z) && (x != 0.f || y != 0.f || z != 0.f); }
// ((a0 x + a1 y) + a2 z); a row [a0 a1 a2 t] of an affine map adds t last
D3R_DEV float row3(float a0, float a1, float a2, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fmul_rn(a0, x), __fmul_rn(a1, y)), __fmul_rn(a2, z));
}
D3R_DEV float row3(const float* a, float x, float y, float z) { return row3(a[0], a[1], a[2], x, y, z); }
D3R_DEV float affine_row(const float* m, float x, float y, float z) { return __fadd_rn(row3(m, x, y, z), m[3]); }
// the squared length (dx dx + dy dy) + dz dz of a difference
D3R_DEV float dist2(float dx, float dy, float dz) { return row3(dx, dy, dz, dx, dy, dz); }

// mask == nullptr: every element passes it (a flat cloud)
D3R_DEV bool valid_at(const float* pts, const uint8_t* mask, const float* weight, size_t g) {
    if (mask && !mask[g]) return false;
    if (!finite3(pts + 3 * g)) return false;
    if (!weight) return true;
    const float w = weight[g];
    return finite_f(w) && w > 0.f;
}

// the number of pairs / voxels a kernel of stage 2-4 works on: what an earlier stage left on the device, never above the buffers' capacity
D3R_DEV int count_of(const int* n_dev, int cap) { return min(max(*n_dev, 0), cap); }

struct KeyParams {
    float lo[3], voxel;
    int shift[3], qmax[3];              // shift of each axis inside the key; 2^bits - 1
};

// one axis of the key: q clamped to its bits. Monotone in x (fp32 subtraction, IEEE division, floor and the clamp all are)
D3R_DEV int axis_q(float x, const KeyParams& k, int c) {
    const float f = floorf(__fdiv_rn(__fsub_rn(x, k.lo[c]), k.voxel));
    return (int)fminf(fmaxf(f, 0.f), (float)k.qmax[c]);
}

// q clamped to its bits: inside the contract (lo = the bounds' minimum, bits from their extent) the clamp never acts
D3R_DEV uint64_t key_of(const float* p, const KeyParams& k) {
    uint64_t key = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) key |= (uint64_t)axis_q(p[c], k, c) << k.shift[c];
    return key;
}

// exclusive scan of a[0, L) in place by ONE workgroup, chunks of NT in order; the sum -> *total_out (when given)
static __global__ __launch_bounds__(NT) void fuse_scan_kernel(int* __restrict__ a, int L, int* __restrict__ total_out) {
    __shared__ int wave_sums[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int run = 0;
    for (int base = 0; base < L; base += NT) {
        const int i = base + threadIdx.x;
        const int x = i < L ? a[i] : 0;
        // reduce.hpp's wave_scan_inclusive, written out: through the call the compiler orders the same instructions differently, and every
        // grid build and d3r_fuse_voxels measured 0.5 % slower (this kernel runs once per sort pass)
        int inc = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wave_sums[wave] = inc;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < WAVES; ++w) {
            const int s = wave_sums[w];
            before += w < wave ? s : 0;
            all += s;
        }
        __syncthreads();
        if (i < L) a[i] = run + before + inc - x;
        run += all;
    }
    if (threadIdx.x == 0 && total_out) *total_out = run;
}

// Stages 1 and 3, one compaction pattern. Tile T of NT elements; its flag counts -> tile_cnt[T] (PLACE = false), or, with tile_cnt scanned,
// the flagged elements placed in order (PLACE = true).
//   KEYS:  element = pixel e = t NT + thread of view v, T = v tiles_per_view + t; flag = valid; places (key, g) into keys / idx
//   HEADS: element = sorted pair i = T NT + thread; flag = i < N and (i == 0 or key[i] != key[i - 1]); places i into idx
//   ROOTS: element = point i = T NT + thread; flag = i < cap and root[i] >= 0; places (root[i], i) into keys / idx (cloud_cluster.hip)
enum { KEYS = 0, HEADS = 1, ROOTS = 2 };
struct FlagArgs {
    const float* pts;
    const uint8_t* mask;
    const float* weight;
    const int *img_h, *img_w;
    int row, tiles_per_view;
    KeyParams key;
    const uint64_t* sorted;             // HEADS: the sorted keys
    const int* n_dev;
    int cap;
    const int* root;                    // ROOTS: the cluster root of every point, -1 for none. Last: the fields above keep their offsets
};

template <int WHAT, bool PLACE>
static __global__ __launch_bounds__(NT) void fuse_flag_kernel(const FlagArgs a, long long n_tiles, int* __restrict__ tile_cnt, uint64_t* __restrict__ keys,
                                                      int* __restrict__ idx) {
    __shared__ int wave_sums[WAVES];
    const int N = WHAT == HEADS ? count_of(a.n_dev, a.cap) : 0;
    for (long long T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        bool flag;
        size_t g = 0;
        long long i = 0;
        if (WHAT == KEYS) {
            const int v = (int)(T / a.tiles_per_view);
            const long long e = (T - (long long)v * a.tiles_per_view) * NT + threadIdx.x;
            g = (size_t)v * a.row + e;
            flag = e < area_of(a.img_h[v], a.img_w[v], a.row) && valid_at(a.pts, a.mask, a.weight, g);
        } else {
            i = T * NT + threadIdx.x;
            flag = WHAT == HEADS ? i < N && (i == 0 || a.sorted[i] != a.sorted[i - 1]) : i < a.cap && a.root[i] >= 0;
        }
        int total;
        const int pos = block_scan_1024(flag, wave_sums, &total);
        if (!PLACE) {
            if (threadIdx.x == 0) tile_cnt[T] = total;
        } else if (flag) {
            const long long o = (long long)tile_cnt[T] + pos;
            if (o < a.cap) {
                if (WHAT == KEYS) {
                    keys[o] = key_of(a.pts + 3 * g, a.key);
                    idx[o] = (int)g;
                } else {
                    if (WHAT == ROOTS) keys[o] = (uint64_t)a.root[i];
                    idx[o] = (int)i;
                }
            }
        }
    }
}

// the 16 digit masks of a wave from four ballots: lane l < 16 gets the lanes whose digit is l
D3R_DEV unsigned long long digit_mask(int digit, unsigned long long ok, const unsigned long long (&bit)[DIGIT_BITS]) {
    unsigned long long m = ok;
#pragma unroll
    for (int b = 0; b < DIGIT_BITS; ++b) m &= ((digit >> b) & 1) ? bit[b] : ~bit[b];
    return m;
}

// hist[d][T] = the pairs of sort tile T (SUB x NT consecutive pairs) whose digit (key >> shift) & 15 is d
static __global__ __launch_bounds__(NT) void fuse_hist_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ n_dev, int cap, int shift,
                                                             int n_tiles, int* __restrict__ hist) {
    __shared__ int cnt[WAVES][DIGITS];
    const int N = count_of(n_dev, cap);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        int mine = 0;                                    // thread d < 16: the tile's count of digit d
        for (int s = 0; s < SUB; ++s) {
            const long long i = ((long long)T * SUB + s) * NT + threadIdx.x;
            const bool ok = i < N;
            const int d = ok ? (int)((keys[i] >> shift) & (DIGITS - 1)) : 0;
            unsigned long long bit[DIGIT_BITS];
#pragma unroll
            for (int b = 0; b < DIGIT_BITS; ++b) bit[b] = __ballot(ok && ((d >> b) & 1));
            const unsigned long long okm = __ballot(ok);
            if (lane < DIGITS) cnt[wave][lane] = __popcll(digit_mask(lane, okm, bit));
            __syncthreads();
            if (threadIdx.x < DIGITS) {
                for (int w = 0; w < WAVES; ++w) mine += cnt[w][threadIdx.x];
            }
            __syncthreads();
        }
        if (threadIdx.x < DIGITS) hist[(size_t)threadIdx.x * n_tiles + T] = mine;
    }
}

// off[d][T] (the scanned hist) = where the first pair of tile T with digit d goes; pairs of one digit keep their order: sub-tile, wave, lane
static __global__ __launch_bounds__(NT) void fuse_scatter_kernel(const uint64_t* __restrict__ keys_in, const int* __restrict__ idx_in,
                                                                const int* __restrict__ n_dev, int cap, int shift, int n_tiles,
                                                                const int* __restrict__ off, uint64_t* __restrict__ keys_out, int* __restrict__ idx_out) {
    __shared__ int cnt[WAVES][DIGITS];
    __shared__ int base[DIGITS];
    const int N = count_of(n_dev, cap);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        if (threadIdx.x < DIGITS) base[threadIdx.x] = off[(size_t)threadIdx.x * n_tiles + T];        // published by the first barrier below
        for (int s = 0; s < SUB; ++s) {
            const long long i = ((long long)T * SUB + s) * NT + threadIdx.x;
            const bool ok = i < N;
            const uint64_t key = ok ? keys_in[i] : 0;
            const int id = ok ? idx_in[i] : 0;
            const int d = (int)((key >> shift) & (DIGITS - 1));
            unsigned long long bit[DIGIT_BITS];
#pragma unroll
            for (int b = 0; b < DIGIT_BITS; ++b) bit[b] = __ballot(ok && ((d >> b) & 1));
            const unsigned long long okm = __ballot(ok);
            if (lane < DIGITS) cnt[wave][lane] = __popcll(digit_mask(lane, okm, bit));
            const int in_wave = __popcll(digit_mask(d, okm, bit) & ((1ull << lane) - 1ull));
            __syncthreads();
            if (ok) {
                int before = 0;
                for (int w = 0; w < wave; ++w) before += cnt[w][d];
                const long long o = (long long)base[d] + before + in_wave;
                if (o < cap) {
                    keys_out[o] = key;
                    idx_out[o] = id;
                }
            }
            __syncthreads();
            if (threadIdx.x < DIGITS) {
                int tot = 0;
                for (int w = 0; w < WAVES; ++w) tot += cnt[w][threadIdx.x];
                base[threadIdx.x] += tot;
            }
            __syncthreads();
        }
    }
}


struct FuseWorkspace {
    int* tile_cnt;          // [max(n tiles_per_view, ceil(cap / NT))]: the tile counts of stage 1, then of stage 3
    int* hist;              // [16][ceil(cap / (SUB NT))]
    int* n_dev;             // [2]: the pairs N, the voxels M
    uint64_t* keys[2];      // [cap] each: ping-pong
    int* idx[2];            // [cap] each; the one the sort does not end in holds the voxel starts
    size_t bytes;
};

static inline FuseWorkspace fuse_workspace(void* base, int n_views, int row, int cap) {
    FuseWorkspace w;
    Carver c(base);
    const long long t1 = (long long)n_views * tiles_of(row, NT), t3 = tiles_of(cap, NT), ts = tiles_of(cap, SUB * NT);
    w.tile_cnt = c.take<int>((size_t)std::max(t1, t3));
    w.hist = c.take<int>((size_t)ts * DIGITS);
    w.n_dev = c.take<int>(2);
    w.keys[0] = c.take<uint64_t>(cap);
    w.keys[1] = c.take<uint64_t>(cap);
    w.idx[0] = c.take<int>(cap);
    w.idx[1] = c.take<int>(cap);
    w.bytes = c.bytes;
    return w;
}

static inline bool fuse_shape_ok(int n_views, int row, int capacity) {
    return n_views > 0 && n_views <= 65535 && row > 0 && (long long)n_views * row <= 2147483647LL && capacity > 0 &&
           (long long)n_views * tiles_of(row, NT) <= 2147483647LL / DIGITS;
}

// lo, voxel and bits into the key's parameters; false when a bit count is outside [1, 21] or lo is not finite. *total_bits: their sum
static inline bool fuse_key_params(const float* lo, float voxel, const int* bits, KeyParams* key, int* total_bits) {
    *total_bits = 0;
    for (int c = 0; c < 3; ++c) {
        if (bits[c] < 1 || bits[c] > 21 || !(lo[c] >= -3.4e38f && lo[c] <= 3.4e38f)) return false;
        key->lo[c] = lo[c];
        key->shift[c] = *total_bits;
        key->qmax[c] = (1 << bits[c]) - 1;
        *total_bits += bits[c];
    }
    key->voxel = voxel;
    return true;
}

// the bits of x: what a sort by an index below n needs, bit_length(n - 1)
static inline int bit_length(unsigned x) {
    int b = 0;
    for (; x; x >>= 1) ++b;
    return b;
}

// Stage 2 on the stream, on buffers of the caller's (tracks.hip sorts its observations by view with it): the *n_dev (at most capacity)
// pairs of keys[cur] / idx[cur] sorted stably by bits [0, total_bits) of the key, pass k by bits [4 k, 4 k + 4), ping-pong between the two
// buffers; hist: [16][ceil(capacity / (SUB NT))]. Returns the buffer the sort ends in (cur itself for total_bits <= 0).
static inline int fuse_sort_pairs(uint64_t* const (&keys)[2], int* const (&idx)[2], int* hist, const int* n_dev, int capacity, int total_bits, int cur,
                                  hipStream_t st) {
    const int ts = (int)tiles_of(capacity, SUB * NT);
    for (int shift = 0; shift < total_bits; shift += DIGIT_BITS, cur ^= 1) {
        hipLaunchKernelGGL(fuse_hist_kernel, dim3(blocks_of(ts, MAX_BLOCKS)), dim3(NT), 0, st, keys[cur], n_dev, capacity, shift, ts, hist);
        hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(NT), 0, st, hist, ts * DIGITS, (int*)nullptr);
        hipLaunchKernelGGL(fuse_scatter_kernel, dim3(blocks_of(ts, MAX_BLOCKS)), dim3(NT), 0, st, keys[cur], idx[cur], n_dev, capacity, shift, ts, hist, keys[cur ^ 1],
                           idx[cur ^ 1]);
    }
    return cur;
}

// Stages 1 and 2 on the stream: a (pts, mask, weight, img_h, img_w, row, key set by the caller) keyed and compacted into w, then sorted.
// Returns the buffer the sort ends in: w.keys[cur] / w.idx[cur] hold the w.n_dev[0] sorted pairs.
static inline int fuse_key_and_sort(FlagArgs& a, const FuseWorkspace& w, int n_views, int capacity, int total_bits, hipStream_t st) {
    const int tpv = (int)tiles_of(a.row, NT);
    const long long t1 = (long long)n_views * tpv;
    a.tiles_per_view = tpv; a.sorted = nullptr; a.n_dev = w.n_dev; a.cap = capacity;
    // 1. key and compact
    hipLaunchKernelGGL((fuse_flag_kernel<KEYS, false>), dim3(blocks_of(t1, MAX_BLOCKS)), dim3(NT), 0, st, a, t1, w.tile_cnt, w.keys[0], w.idx[0]);
    hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(NT), 0, st, w.tile_cnt, (int)t1, w.n_dev);
    hipLaunchKernelGGL((fuse_flag_kernel<KEYS, true>), dim3(blocks_of(t1, MAX_BLOCKS)), dim3(NT), 0, st, a, t1, w.tile_cnt, w.keys[0], w.idx[0]);
    // 2. the sort: pass k orders by bits [4 k, 4 k + 4) of the key
    return fuse_sort_pairs(w.keys, w.idx, w.hist, w.n_dev, capacity, total_bits, 0, st);
}

// Stage 3 on the stream: the segment heads of the sorted keys w.keys[cur], into the index buffer the sort left free (returned); their
// number -> w.n_dev[1]
static inline int* fuse_segment_heads(FlagArgs& a, const FuseWorkspace& w, int cur, int capacity, hipStream_t st) {
    const long long t3 = tiles_of(capacity, NT);
    int* starts = w.idx[cur ^ 1];
    a.sorted = w.keys[cur];
    hipLaunchKernelGGL((fuse_flag_kernel<HEADS, false>), dim3(blocks_of(t3, MAX_BLOCKS)), dim3(NT), 0, st, a, t3, w.tile_cnt, (uint64_t*)nullptr, starts);
    hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(NT), 0, st, w.tile_cnt, (int)t3, w.n_dev + 1);
    hipLaunchKernelGGL((fuse_flag_kernel<HEADS, true>), dim3(blocks_of(t3, MAX_BLOCKS)), dim3(NT), 0, st, a, t3, w.tile_cnt, (uint64_t*)nullptr, starts);
    return starts;
}

}  // namespace fuse
}  // namespace d3r
