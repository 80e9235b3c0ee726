// dust3r_amd -- 2-D tracks of a cloud in the views of a scene (new; FusedCloud.build_tracks, the POINTS2D and tracks of the COLMAP export):
// which pixel of which view observes point j, by PROJECTION, and how far the projection lands from that pixel. Inputs are the scene's padded
// stacks, as for fuse.hip (view v is elements [0, h w) of row v, flat index g = v row + e; what lies behind h w is never read), the cloud's
// fp32 positions and per view 16 doubles: the world-to-camera rows R (9, row-major), t (3), then fx, fy, cx, cy.
//
// THE RULE for point c and view v, every fp64 and fp32 operation rounded on its own (built with -ffp-contract=off), in the order written:
//   1. X_r = ((R[r][0] x + R[r][1] y) + R[r][2] z) + t[r] in fp64; rejected unless X_2 > 0 (NaN too)
//   2. u = fx (X_0 / X_2) + cx, w = fy (X_1 / X_2) + cy; iu = floor(u + 0.5), iw = floor(w + 0.5); rejected unless 0 <= iu < W and
//      0 <= iw < H, compared in fp64 before any conversion to int
//   3. the candidates are the pixels (iu + a, iw + b), a, b in {-1, 0, 1}, inside the image, valid by valid_at (fuse_grid.hpp), with
//      fp32 d2 = (dx dx + dy dy) + dz dz to c at most r2
//   4. the least d2 wins, on a tie the lowest pixel index e = y W + x
//   5. the observation (v, e) carries e2 = (u - x) (u - x) + (w - y) (w - y) in fp64; with a threshold it is dropped when e2 > thr2
//
//   d3r_cloud_tracks_count  tracks_walk_kernel<false>  one thread per point walks the views, counts its observations and keeps one bit per
//                                                      view (seen [M][ceil(n / 32)]): which views observe it
//                           tracks_total_kernel        their sum in 64 bits (one workgroup), so that a total past 2^31 - 1 is seen
//                           fuse_scan_kernel           point_off [M + 1]
//   d3r_cloud_tracks_fill   tracks_walk_kernel<true>   the same walk over the views whose bit is set writes view / pixel / e2 of observation
//                                                      k = point_off[j] + i, and (view, k) as the pairs of the sort
//                           fuse_sort_pairs            stable LSD radix sort by view over bit_length(n - 1) bits (fuse_grid.hpp): image_obs
//                           tracks_image_off_kernel    image_off [n + 1] from the sorted views: the thread of the first observation of a
//                                                      view writes the offsets of that view and of the empty views before it
//                           tracks_point2d_kernel      point2d[image_obs[k']] = k' - image_off[view]
// A track is in ascending view order (the walk's), an image's list in ascending point order (the sort is stable and k ascends with the
// point). Every output slot has one writer: no atomics, no waiting between workgroups. The camera rows are read at a wave-uniform address
// (the view loop is the same for every lane), which the compiler turns into scalar loads; the pointmaps are gathered, nine pixels per pair
// that projects into the image. Integer results and fp64 + * / floor only: the bytes of the numpy restatement (tests/test_tracks_cpu.py).
#include <cmath>
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "scene_common.hpp"
#include "fuse_grid.hpp"

namespace d3r {
namespace tracks {

using namespace d3r::fuse;

constexpr int WALK_NT = 256;
constexpr int CAM_DOUBLES = 16;

struct WalkArgs {
    const float* pts;
    const uint8_t* mask;
    const float* weight;
    const int *img_h, *img_w;
    int row, n_views, n_points;
    const float* positions;
    const double* cams;
    float r2;
    int has_thr;
    double thr2;
};

// FILL = false: cnt[j] = the observations of point j, cnt[M] = 0, and bit v & 31 of seen[j][v >> 5] says whether view v observes it.
// FILL = true: cnt is point_off, observation k = point_off[j] + i; only the views whose bit is set are walked again (their projection
// and their nine candidates are recomputed: the same arithmetic on the same inputs, so the same observation).
template <bool FILL>
__global__ __launch_bounds__(WALK_NT) void tracks_walk_kernel(const WalkArgs a, int* __restrict__ cnt, uint32_t* __restrict__ seen, int capacity, int* __restrict__ view_out,
                                                              int* __restrict__ pixel_out, double* __restrict__ e2_out, uint64_t* __restrict__ keys,
                                                              int* __restrict__ idx) {
    if (!FILL && blockIdx.x == 0 && threadIdx.x == 0) cnt[a.n_points] = 0;
    for (long long j = (long long)blockIdx.x * WALK_NT + threadIdx.x; j < a.n_points; j += (long long)gridDim.x * WALK_NT) {
        const float cx32 = a.positions[3 * j], cy32 = a.positions[3 * j + 1], cz32 = a.positions[3 * j + 2];
        const double x = (double)cx32, y = (double)cy32, z = (double)cz32;
        long long k = FILL ? (long long)cnt[j] : 0;
        int found = 0;
        const int words = (a.n_views + 31) >> 5;
        uint32_t* __restrict__ bits = seen + (size_t)j * words;
        uint32_t word = 0;
        for (int v = 0; v < a.n_views; ++v) {
            if (FILL) {
                if ((v & 31) == 0) word = bits[v >> 5];
                const uint32_t rest = word >> (v & 31);                 // the bits of views v ... of this word
                if (rest == 0) {
                    v |= 31;                                            // on to the next word
                    continue;
                }
                v += __builtin_ctz(rest);
                if (v >= a.n_views) break;                              // (a bit the count pass cannot have set)
            } else if ((v & 31) == 0 && v > 0) {
                bits[(v >> 5) - 1] = word;
                word = 0;
            }
            const double* __restrict__ cam = a.cams + (size_t)v * CAM_DOUBLES;
            const double X2 = ((cam[6] * x + cam[7] * y) + cam[8] * z) + cam[11];
            if (!(X2 > 0.0)) continue;
            const double X0 = ((cam[0] * x + cam[1] * y) + cam[2] * z) + cam[9];
            const double X1 = ((cam[3] * x + cam[4] * y) + cam[5] * z) + cam[10];
            const double u = cam[12] * (X0 / X2) + cam[14];
            const double w = cam[13] * (X1 / X2) + cam[15];
            const double iu = floor(u + 0.5), iw = floor(w + 0.5);
            const int H = a.img_h[v], W = a.img_w[v];
            if (area_of(H, W, a.row) == 0) continue;
            if (!(iu >= 0.0 && iu < (double)W && iw >= 0.0 && iw < (double)H)) continue;
            const int px = (int)iu, py = (int)iw;
            const size_t base = (size_t)v * a.row;
            float best = 0.f;
            int best_e = -1;
            for (int b = -1; b <= 1; ++b) {
                const int yy = py + b;
                if (yy < 0 || yy >= H) continue;
                for (int c = -1; c <= 1; ++c) {
                    const int xx = px + c;
                    if (xx < 0 || xx >= W) continue;
                    const int e = yy * W + xx;
                    const size_t g = base + e;
                    if (!valid_at(a.pts, a.mask, a.weight, g)) continue;
                    const float* p = a.pts + 3 * g;
                    const float dx = p[0] - cx32, dy = p[1] - cy32, dz = p[2] - cz32;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 <= a.r2 && (best_e < 0 || d2 < best)) {       // ascending e: the first of equal d2 stays
                        best = d2;
                        best_e = e;
                    }
                }
            }
            if (best_e < 0) continue;
            const double ex = u - (double)(best_e % W), ey = w - (double)(best_e / W);
            const double e2 = ex * ex + ey * ey;
            if (a.has_thr && e2 > a.thr2) continue;
            if (FILL) {
                if (k < capacity) {
                    view_out[k] = v;
                    pixel_out[k] = best_e;
                    e2_out[k] = e2;
                    keys[k] = (uint64_t)v;
                    idx[k] = (int)k;
                }
                ++k;
            } else {
                ++found;
                word |= 1u << (v & 31);
            }
        }
        if (!FILL) {
            bits[words - 1] = word;
            cnt[j] = found;
        }
    }
}

// *total_out = the sum of cnt[0, L) in 64 bits, one workgroup, a fixed order (integers: any order gives the same)
__global__ __launch_bounds__(NT) void tracks_total_kernel(const int* __restrict__ cnt, int L, long long* __restrict__ total_out) {
    __shared__ long long wave_sums[WAVES];
    long long s[1] = {0};
    for (long long i = threadIdx.x; i < L; i += NT) s[0] += cnt[i];
    block_reduce_gather<NT, false>(s, wave_sums, Sum());
    if (threadIdx.x == 0) *total_out = s[0];
}

// sorted [T]: the views of the observations in image order. Thread k' <= T: the views (sorted[k' - 1], sorted[k']] start at k' (k' = T: the
// views after the last observation's, and image_off[n] = T): every slot of image_off [n + 1] has one writer
__global__ __launch_bounds__(WALK_NT) void tracks_image_off_kernel(const uint64_t* __restrict__ sorted, const int* __restrict__ n_dev, int capacity, int n_views,
                                                                   int* __restrict__ image_off) {
    const int T = count_of(n_dev, capacity);
    for (long long k = (long long)blockIdx.x * WALK_NT + threadIdx.x; k <= T; k += (long long)gridDim.x * WALK_NT) {
        const int prev = k > 0 ? (int)sorted[k - 1] : -1;
        const int cur = k < T ? min((int)sorted[k], n_views - 1) : n_views;
        for (int v = prev + 1; v <= cur; ++v) image_off[v] = (int)k;
    }
}

__global__ __launch_bounds__(WALK_NT) void tracks_point2d_kernel(const uint64_t* __restrict__ sorted, const int* __restrict__ image_obs,
                                                                 const int* __restrict__ n_dev, int capacity, int n_views, const int* __restrict__ image_off,
                                                                 int* __restrict__ point2d) {
    const int T = count_of(n_dev, capacity);
    for (long long k = (long long)blockIdx.x * WALK_NT + threadIdx.x; k < T; k += (long long)gridDim.x * WALK_NT) {
        const int v = min((int)sorted[k], n_views - 1), o = image_obs[k];
        if (o >= 0 && o < T) point2d[o] = (int)k - image_off[v];
    }
}

struct TracksWorkspace {
    uint64_t* keys[2];      // [cap] each: the views, ping-pong
    int* idx;               // [cap]: the index buffer beside image_obs_out
    int* hist;              // [16][ceil(cap / (SUB NT))]
    size_t bytes;
};

static inline TracksWorkspace tracks_workspace(void* base, int cap) {
    TracksWorkspace w;
    Carver c(base);
    w.keys[0] = c.take<uint64_t>(cap);
    w.keys[1] = c.take<uint64_t>(cap);
    w.idx = c.take<int>(cap);
    w.hist = c.take<int>((size_t)tiles_of(cap, SUB * NT) * DIGITS);
    w.bytes = c.bytes;
    return w;
}

static inline bool tracks_shape_ok(int n_views, int row, int n_points) {
    return n_views >= 1 && n_views <= 65535 && row > 0 && (long long)n_views * row <= 2147483647LL && n_points > 0 && n_points < 2147483647;
}

static inline bool tracks_walk_args(WalkArgs* a, int n_views, const float* pts, const uint8_t* mask, const float* weight, const int* img_h, const int* img_w, int row,
                                    int n_points, const float* positions, const double* cams, float r2, int has_thr, double thr2) {
    if (!tracks_shape_ok(n_views, row, n_points) || !pts || !mask || !img_h || !img_w || !positions || !cams) return false;
    if (!(r2 >= 0.f && r2 <= 3.4028234663852886e38f)) return false;
    if (has_thr && !(thr2 >= 0.0)) return false;
    a->pts = pts; a->mask = mask; a->weight = weight; a->img_h = img_h; a->img_w = img_w;
    a->row = row; a->n_views = n_views; a->n_points = n_points;
    a->positions = positions; a->cams = cams;
    a->r2 = r2; a->has_thr = has_thr ? 1 : 0; a->thr2 = has_thr ? thr2 : 0.0;
    return true;
}

}  // namespace tracks
}  // namespace d3r

using namespace d3r;
using namespace d3r::tracks;

extern "C" size_t d3r_cloud_tracks_workspace_bytes(int capacity) {
    if (capacity <= 0) return 0;
    return tracks_workspace(nullptr, capacity).bytes;
}

extern "C" int d3r_cloud_tracks_count(int n_views, const float* pts, const uint8_t* mask, const float* weight, const int* img_h_dev, const int* img_w_dev, int row,
                                      int n_points, const float* positions, const double* cams_dev, float r2, int has_thr, double thr2, int* point_off_out,
                                      uint32_t* seen_out, long long* total_out, void* stream) {
    WalkArgs a;
    if (!tracks_walk_args(&a, n_views, pts, mask, weight, img_h_dev, img_w_dev, row, n_points, positions, cams_dev, r2, has_thr, thr2) || !point_off_out ||
        !seen_out || !total_out)
        return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((tracks_walk_kernel<false>), dim3(blocks_of(tiles_of(n_points, WALK_NT), MAX_BLOCKS)), dim3(WALK_NT), 0, st, a, point_off_out, seen_out, 0,
                       (int*)nullptr, (int*)nullptr, (double*)nullptr, (uint64_t*)nullptr, (int*)nullptr);
    hipLaunchKernelGGL(tracks_total_kernel, dim3(1), dim3(NT), 0, st, point_off_out, n_points, total_out);
    hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(NT), 0, st, point_off_out, n_points + 1, (int*)nullptr);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_cloud_tracks_fill(int n_views, const float* pts, const uint8_t* mask, const float* weight, const int* img_h_dev, const int* img_w_dev, int row,
                                     int n_points, const float* positions, const double* cams_dev, float r2, int has_thr, double thr2, const int* point_off,
                                     const uint32_t* seen, long long total, int capacity, int* view_out, int* pixel_out, double* err2_out, int* point2d_out, int* image_off_out,
                                     int* image_obs_out, void* workspace, void* stream) {
    WalkArgs a;
    if (!tracks_walk_args(&a, n_views, pts, mask, weight, img_h_dev, img_w_dev, row, n_points, positions, cams_dev, r2, has_thr, thr2) || !point_off || !seen || !view_out ||
        !pixel_out || !err2_out || !point2d_out || !image_off_out || !image_obs_out || !workspace || capacity <= 0 || total < 0 || total > capacity ||
        total > 2147483647LL)
        return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const TracksWorkspace w = tracks_workspace(workspace, capacity);
    const int bits = bit_length((unsigned)(n_views - 1));
    const int passes = (bits + DIGIT_BITS - 1) / DIGIT_BITS;
    // the sort ends in image_obs_out: an even number of passes starts there, an odd one in the workspace's buffer
    uint64_t* const keys[2] = {w.keys[0], w.keys[1]};
    int* const idx[2] = {image_obs_out, w.idx};
    const int start = passes & 1;
    const int* n_dev = point_off + n_points;                           // T, as the count pass left it
    hipLaunchKernelGGL((tracks_walk_kernel<true>), dim3(blocks_of(tiles_of(n_points, WALK_NT), MAX_BLOCKS)), dim3(WALK_NT), 0, st, a, (int*)point_off, (uint32_t*)seen, capacity, view_out,
                       pixel_out, err2_out, keys[start], idx[start]);
    const int cur = fuse_sort_pairs(keys, idx, w.hist, n_dev, capacity, bits, start, st);      // cur == 0
    const int blocks = blocks_of(tiles_of((long long)capacity + 1, WALK_NT), MAX_BLOCKS);
    hipLaunchKernelGGL(tracks_image_off_kernel, dim3(blocks), dim3(WALK_NT), 0, st, keys[cur], n_dev, capacity, n_views, image_off_out);
    hipLaunchKernelGGL(tracks_point2d_kernel, dim3(blocks), dim3(WALK_NT), 0, st, keys[cur], idx[cur], n_dev, capacity, n_views, image_off_out, point2d_out);
    return rc_of(hipGetLastError());
}
