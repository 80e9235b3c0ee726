// dust3r_amd -- scene.fuse(): the per-view pointmaps of a scene merged into ONE voxel-fused, confidence-weighted cloud (new; the reference
// exports every masked pixel of every view). Inputs are the scene's padded stacks, as for d3r_scene_mesh (utils/padded.py): view v is
// elements [0, h w) of row v, flat index g = v row + e; what lies behind h w is never read.
//
// A pixel is VALID when its mask is nonzero, its three coordinates are finite and its weight is finite and > 0 (no weights: 1).
//   d3r_fuse_bounds   fuse_bounds_kernel        per workgroup, the bounds and the count of the valid points of its pixels
//                     fuse_bounds_final_kernel  one workgroup over the partials in index order
//   d3r_fuse_voxels   1. key and compact: fuse_flag_kernel<KEYS, false> counts the valid pixels of every tile, fuse_scan_kernel scans the tile
//                        counts, fuse_flag_kernel<KEYS, true> places (key, g) of every valid pixel, view then raster order;
//                        key = q_x | q_y << bits_x | q_z << (bits_x + bits_y), q_c = (int)floorf((p_c - lo_c) / voxel) in fp32
//                     2. stable LSD radix sort by key, 4 bits per pass, over bits_x + bits_y + bits_z bits only. Per pass three launches:
//                        fuse_hist_kernel (per tile of SUB x 1024 pairs the count of each digit, digit-major), fuse_scan_kernel over the
//                        16 x tiles counts, fuse_scatter_kernel (rank inside the tile from wave ballots, tiles in order)
//                     3. segment heads: key[i] != key[i - 1], compacted with the pattern of stage 1 (fuse_flag_kernel<HEADS, ...>)
//                     4. fuse_reduce_kernel: one thread per voxel walks its points in sorted order (= view, then raster: the sort is
//                        stable) and sums in fp64
// No kernel waits on another workgroup: every scan over tiles is a launch of its own (ONE workgroup, chunks in order), there is no
// atomic, no look-back, no grid barrier. Integer placement and fixed-order fp64 sums: the same bytes on every run, and the bytes of the
// numpy restatement (tests/test_fuse_cpu.py). A voxel as large as the scene makes one thread walk every point: slow but finite, not a target.
#include "../../include/dust3r_hip.h"
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

D3R_DEV bool valid_at(const float* pts, const uint8_t* mask, const float* weight, size_t g) {
    if (!mask[g]) return false;
    const float* p = pts + 3 * g;
    if (!(finite_f(p[0]) && finite_f(p[1]) && finite_f(p[2]))) return false;
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

// q clamped to its bits: inside the contract (lo = the bounds' minimum, bits from their extent) the clamp never acts
D3R_DEV uint64_t key_of(const float* p, const KeyParams& k) {
    uint64_t key = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float f = floorf(__fdiv_rn(__fsub_rn(p[c], k.lo[c]), k.voxel));
        const int q = (int)fminf(fmaxf(f, 0.f), (float)k.qmax[c]);
        key |= (uint64_t)q << k.shift[c];
    }
    return key;
}

__global__ __launch_bounds__(NT) void fuse_bounds_kernel(const float* __restrict__ pts, const uint8_t* __restrict__ mask, const float* __restrict__ weight,
                                                        const int* __restrict__ img_h, const int* __restrict__ img_w, int row,
                                                        float* __restrict__ partials, int* __restrict__ part_cnt) {
    __shared__ float lds_b[WAVES * 6];
    __shared__ int wave_cnt[WAVES];
    const int v = blockIdx.y;
    const long long area = area_of(img_h[v], img_w[v], row);
    const size_t base = (size_t)v * row;
    float b[6];
    bounds_init(b);
    int cnt = 0;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < area; e += (long long)gridDim.x * NT) {
        if (valid_at(pts, mask, weight, base + e)) {
            bounds_add(b, pts + 3 * (base + e));
            ++cnt;
        }
    }
    const size_t part = (size_t)v * gridDim.x + blockIdx.x;
    block_bounds(b, lds_b, partials + part * 6);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < WAVES; ++w) s += wave_cnt[w];
        part_cnt[part] = s;
    }
}

__global__ __launch_bounds__(256) void fuse_bounds_final_kernel(int n_parts, const float* __restrict__ partials, const int* __restrict__ part_cnt,
                                                               float* __restrict__ bounds_out, long long* __restrict__ count_out) {
    __shared__ float lds[4][6];
    __shared__ long long lds_n[4];
    float b[6];
    bounds_init(b);
    long long n = 0;
    for (int i = threadIdx.x; i < n_parts; i += 256) {
        const float* p = partials + (size_t)i * 6;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            b[c] = fminf(b[c], p[c]);
            b[3 + c] = fmaxf(b[3 + c], p[3 + c]);
        }
        n += part_cnt[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float t = __shfl_xor(b[c], o);
            b[c] = c < 3 ? fminf(b[c], t) : fmaxf(b[c], t);
        }
        n += __shfl_xor(n, o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) lds[threadIdx.x >> 6][c] = b[c];
        lds_n[threadIdx.x >> 6] = n;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        float r = lds[0][c];
        for (int w = 1; w < 4; ++w) r = c < 3 ? fminf(r, lds[w][c]) : fmaxf(r, lds[w][c]);
        bounds_out[c] = r;
    }
    if (threadIdx.x == 6) *count_out = lds_n[0] + lds_n[1] + lds_n[2] + lds_n[3];
}

// exclusive scan of a[0, L) in place by ONE workgroup, chunks of NT in order; the sum -> *total_out (when given)
__global__ __launch_bounds__(NT) void fuse_scan_kernel(int* __restrict__ a, int L, int* __restrict__ total_out) {
    __shared__ int wave_sums[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int run = 0;
    for (int base = 0; base < L; base += NT) {
        const int i = base + threadIdx.x;
        const int x = i < L ? a[i] : 0;
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
enum { KEYS = 0, HEADS = 1 };
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
};

template <int WHAT, bool PLACE>
__global__ __launch_bounds__(NT) void fuse_flag_kernel(const FlagArgs a, long long n_tiles, int* __restrict__ tile_cnt, uint64_t* __restrict__ keys,
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
            flag = i < N && (i == 0 || a.sorted[i] != a.sorted[i - 1]);
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
__global__ __launch_bounds__(NT) void fuse_hist_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ n_dev, int cap, int shift, int n_tiles,
                                                      int* __restrict__ hist) {
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
__global__ __launch_bounds__(NT) void fuse_scatter_kernel(const uint64_t* __restrict__ keys_in, const int* __restrict__ idx_in, const int* __restrict__ n_dev,
                                                         int cap, int shift, int n_tiles, const int* __restrict__ off, uint64_t* __restrict__ keys_out,
                                                         int* __restrict__ idx_out) {
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

// voxel j = the sorted pairs [starts[j], starts[j + 1]) (the last: up to N), walked in order
__global__ __launch_bounds__(256) void fuse_reduce_kernel(const int* __restrict__ idx, const int* __restrict__ starts, const int* __restrict__ n_dev,
                                                         const int* __restrict__ m_dev, int cap, const float* __restrict__ pts,
                                                         const float* __restrict__ weight, const void* __restrict__ rgb, int is_u8,
                                                         float* __restrict__ positions, uint32_t* __restrict__ colors, float* __restrict__ weight_out,
                                                         int* __restrict__ count_out, long long* __restrict__ totals_out) {
    const int N = count_of(n_dev, cap), M = count_of(m_dev, cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        totals_out[0] = N;
        totals_out[1] = M;
    }
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < M; j += (long long)gridDim.x * 256) {
        const int s = starts[j], e = j + 1 < M ? starts[j + 1] : N;
        double W = 0.0, S[3] = {0.0, 0.0, 0.0}, C[3] = {0.0, 0.0, 0.0};
        for (int i = s; i < e; ++i) {
            const size_t g = (size_t)idx[i];
            const double w = weight ? (double)weight[g] : 1.0;
            const float* p = pts + 3 * g;
            const uint32_t q = pixel_q(rgb, is_u8, g);
            W += w;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                S[c] += w * (double)p[c];                               // exact products (24 + 24 bits), one rounding per sum
                C[c] += w * (double)((q >> (8 * c)) & 0xFFu);
            }
        }
        uint32_t rgba = 0xFF000000u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            positions[3 * j + c] = (float)(S[c] / W);
            rgba |= (uint32_t)fmin(fmax(floor(C[c] / W + 0.5), 0.0), 255.0) << (8 * c);
        }
        colors[j] = rgba;
        weight_out[j] = (float)W;
        count_out[j] = e - s;
    }
}

}  // namespace fuse
}  // namespace d3r

using namespace d3r::fuse;

static long long fuse_tiles(long long n, int per) { return (n + per - 1) / per; }
static int fuse_blocks(long long tiles) { return (int)std::max(1LL, std::min(tiles, (long long)MAX_BLOCKS)); }

extern "C" size_t d3r_fuse_bounds_workspace_bytes(int n_views, int row) {
    if (n_views <= 0 || row <= 0) return 0;
    const size_t parts = (size_t)n_views * fuse_blocks(fuse_tiles(row, NT));
    return align256(parts * 6 * sizeof(float)) + align256(parts * sizeof(int));
}

extern "C" int d3r_fuse_bounds(int n_views, const float* pts, const uint8_t* mask, const float* weight, const int* img_h_dev, const int* img_w_dev, int row,
                               float* bounds_out, long long* count_out, void* workspace, void* stream) {
    if (n_views <= 0 || n_views > 65535 || !pts || !mask || !img_h_dev || !img_w_dev || row <= 0 || (long long)n_views * row > 2147483647LL ||
        !bounds_out || !count_out || !workspace)
        return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int bx = fuse_blocks(fuse_tiles(row, NT));
    const size_t parts = (size_t)n_views * bx;
    float* partials = (float*)workspace;
    int* part_cnt = (int*)((char*)workspace + align256(parts * 6 * sizeof(float)));
    hipLaunchKernelGGL(fuse_bounds_kernel, dim3(bx, n_views), dim3(NT), 0, st, pts, mask, weight, img_h_dev, img_w_dev, row, partials, part_cnt);
    hipLaunchKernelGGL(fuse_bounds_final_kernel, dim3(1), dim3(256), 0, st, (int)parts, partials, part_cnt, bounds_out, count_out);
    return rc_of(hipGetLastError());
}

struct FuseWorkspace {
    int* tile_cnt;          // [max(n tiles_per_view, ceil(cap / NT))]: the tile counts of stage 1, then of stage 3
    int* hist;              // [16][ceil(cap / (SUB NT))]
    int* n_dev;             // [2]: the pairs N, the voxels M
    uint64_t* keys[2];      // [cap] each: ping-pong
    int* idx[2];            // [cap] each; the one the sort does not end in holds the voxel starts
    size_t bytes;
};

static FuseWorkspace fuse_workspace(void* base, int n_views, int row, int cap) {
    FuseWorkspace w;
    char* p = (char*)base;
    const long long t1 = (long long)n_views * fuse_tiles(row, NT), t3 = fuse_tiles(cap, NT), ts = fuse_tiles(cap, SUB * NT);
    const size_t sizes[7] = {(size_t)std::max(t1, t3) * sizeof(int), (size_t)ts * DIGITS * sizeof(int), 2 * sizeof(int), (size_t)cap * sizeof(uint64_t),
                             (size_t)cap * sizeof(uint64_t), (size_t)cap * sizeof(int), (size_t)cap * sizeof(int)};
    void* ptrs[7];
    size_t off = 0;
    for (int i = 0; i < 7; ++i) {
        ptrs[i] = p ? p + off : nullptr;
        off += align256(sizes[i]);
    }
    w.tile_cnt = (int*)ptrs[0];
    w.hist = (int*)ptrs[1];
    w.n_dev = (int*)ptrs[2];
    w.keys[0] = (uint64_t*)ptrs[3];
    w.keys[1] = (uint64_t*)ptrs[4];
    w.idx[0] = (int*)ptrs[5];
    w.idx[1] = (int*)ptrs[6];
    w.bytes = off;
    return w;
}

static bool fuse_shape_ok(int n_views, int row, int capacity) {
    return n_views > 0 && n_views <= 65535 && row > 0 && (long long)n_views * row <= 2147483647LL && capacity > 0 &&
           (long long)n_views * fuse_tiles(row, NT) <= 2147483647LL / DIGITS;
}

extern "C" size_t d3r_fuse_voxels_workspace_bytes(int n_views, int row, int capacity) {
    if (!fuse_shape_ok(n_views, row, capacity)) return 0;
    return fuse_workspace(nullptr, n_views, row, capacity).bytes;
}

extern "C" int d3r_fuse_voxels(int n_views, const float* pts, const uint8_t* mask, const float* weight, const void* rgb, int rgb_is_u8, const int* img_h_dev,
                               const int* img_w_dev, int row, const float* lo, float voxel, const int* bits, int capacity, float* positions_out,
                               uint32_t* colors_out, float* weight_out, int* count_out, long long* totals_out, void* workspace, void* stream) {
    if (!fuse_shape_ok(n_views, row, capacity) || !pts || !mask || !rgb || !img_h_dev || !img_w_dev || !lo || !bits || !positions_out || !colors_out ||
        !weight_out || !count_out || !totals_out || !workspace || !(voxel > 0.f) || !(voxel <= 3.0e38f))
        return D3R_ERR_INVALID;
    FlagArgs a;
    int total_bits = 0;
    for (int c = 0; c < 3; ++c) {
        if (bits[c] < 1 || bits[c] > 21 || !(lo[c] >= -3.4e38f && lo[c] <= 3.4e38f)) return D3R_ERR_INVALID;
        a.key.lo[c] = lo[c];
        a.key.shift[c] = total_bits;
        a.key.qmax[c] = (1 << bits[c]) - 1;
        total_bits += bits[c];
    }
    a.key.voxel = voxel;
    hipStream_t st = (hipStream_t)stream;
    const FuseWorkspace w = fuse_workspace(workspace, n_views, row, capacity);
    const int tpv = (int)fuse_tiles(row, NT);
    const long long t1 = (long long)n_views * tpv, t3 = fuse_tiles(capacity, NT);
    const int ts = (int)fuse_tiles(capacity, SUB * NT);
    a.pts = pts; a.mask = mask; a.weight = weight; a.img_h = img_h_dev; a.img_w = img_w_dev;
    a.row = row; a.tiles_per_view = tpv; a.sorted = nullptr; a.n_dev = w.n_dev; a.cap = capacity;
    // 1. key and compact
    hipLaunchKernelGGL((fuse_flag_kernel<KEYS, false>), dim3(fuse_blocks(t1)), dim3(NT), 0, st, a, t1, w.tile_cnt, w.keys[0], w.idx[0]);
    hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(NT), 0, st, w.tile_cnt, (int)t1, w.n_dev);
    hipLaunchKernelGGL((fuse_flag_kernel<KEYS, true>), dim3(fuse_blocks(t1)), dim3(NT), 0, st, a, t1, w.tile_cnt, w.keys[0], w.idx[0]);
    // 2. the sort: pass k orders by bits [4 k, 4 k + 4) of the key
    int cur = 0;
    for (int shift = 0; shift < total_bits; shift += DIGIT_BITS, cur ^= 1) {
        hipLaunchKernelGGL(fuse_hist_kernel, dim3(fuse_blocks(ts)), dim3(NT), 0, st, w.keys[cur], w.n_dev, capacity, shift, ts, w.hist);
        hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(NT), 0, st, w.hist, ts * DIGITS, (int*)nullptr);
        hipLaunchKernelGGL(fuse_scatter_kernel, dim3(fuse_blocks(ts)), dim3(NT), 0, st, w.keys[cur], w.idx[cur], w.n_dev, capacity, shift, ts, w.hist,
                           w.keys[cur ^ 1], w.idx[cur ^ 1]);
    }
    // 3. segment heads, into the index buffer the sort left free
    int* starts = w.idx[cur ^ 1];
    a.sorted = w.keys[cur];
    hipLaunchKernelGGL((fuse_flag_kernel<HEADS, false>), dim3(fuse_blocks(t3)), dim3(NT), 0, st, a, t3, w.tile_cnt, (uint64_t*)nullptr, starts);
    hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(NT), 0, st, w.tile_cnt, (int)t3, w.n_dev + 1);
    hipLaunchKernelGGL((fuse_flag_kernel<HEADS, true>), dim3(fuse_blocks(t3)), dim3(NT), 0, st, a, t3, w.tile_cnt, (uint64_t*)nullptr, starts);
    // 4. reduce
    hipLaunchKernelGGL(fuse_reduce_kernel, dim3(fuse_blocks(fuse_tiles(capacity, 256))), dim3(256), 0, st, w.idx[cur], starts, w.n_dev, w.n_dev + 1, capacity,
                       pts, weight, rgb, rgb_is_u8, positions_out, colors_out, weight_out, count_out, totals_out);
    return rc_of(hipGetLastError());
}
