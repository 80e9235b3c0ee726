// dust3r_amd -- sky segmentation of a scene's images (the reference's dust3r/viz.py:345-381 `segment_sky`, called by
// BasePCOptimizer.mask_sky, dust3r/cloud_opt/base_opt.py:290-295), batched over all images of a scene in one call.
//
// Per image: 8-bit HSV of the RGB picture (OpenCV's COLOR_BGR2HSV fixed-point path applied to RGB data, as the reference does),
// a colour threshold, a binary opening with a 5x5 square, the 8-connected components of the opened mask, and the selection of
// every component whose area is more than half the largest one. Everything is integer arithmetic: the output is bit-exact and
// does not depend on the order in which atomics land.
//
// Layout: images are rows of one [n][max_area] array (row-major H x W inside a row, RGB interleaved), sizes in device arrays,
// like d3r_clean_pointcloud. Kernels (all grid-stride over 32 x 32 tiles or over pixels, so the host needs no image size):
//   sky_open_label_kernel  colour mask of the tile + a 4-pixel halo, erosion and dilation in LDS, union-find of the tile in LDS;
//                          writes a parent label per pixel (image-linear index of the tile-local root; -1 = background) and
//                          the pixel count of each tile-local component at its root
//   sky_merge_kernel       the tiles' left column and top row link to their 8-neighbours in other tiles: a concurrent union-find on
//                          the global labels. Another workgroup (on another XCD) may relink any root at any time, so every parent
//                          read or written here is an agent-scope atomic: plain loads could return stale L1/L2 lines.
//   sky_flatten_kernel     root of every pixel (written back as its label); the tile-local counts are added up at the roots
//   sky_amax_kernel        atomicMax of the root areas: the largest component of each image
//   sky_select_kernel      mask = foreground && 2 * area(root) > a_max
// Kernel boundaries give the visibility between phases.
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "scene_common.hpp"

namespace d3r {
namespace sky {

constexpr int T = 32;        // tile edge (output pixels)
constexpr int HALO = 4;      // 2 for the erosion + 2 for the dilation
constexpr int M = T + 2 * HALO;
constexpr int NT = 256;      // threads per tile workgroup

// OpenCV RGB2HSV_b (hsv_shift = 12, hrange 180). cvRound of (255 << 12) / v and (180 << 12) / (6 d) never meets a tie for
// v, d < 256, so round-half-up in integers is exact: floor(x / y + 1/2) = (2 x + y) / (2 y).
D3R_DEV int sdiv(int v) { return v == 0 ? 0 : (2 * (255 << 12) + v) / (2 * v); }
D3R_DEV int hdiv180(int d) { return d == 0 ? 0 : (2 * (180 << 12) + 6 * d) / (12 * d); }

// steps 2-3 of the reference on one pixel of an RGB picture: cv2 reads the R channel as "b" and the B channel as "r"
D3R_DEV bool sky_color(int R, int G, int B) {
    const int b = R, g = G, r = B;
    const int v = max(max(b, g), r), vmin = min(min(b, g), r);
    const int diff = v - vmin;
    const int s = (diff * sdiv(v) + (1 << 11)) >> 12;
    int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (h * hdiv180(diff) + (1 << 11)) >> 12;
    h += h < 0 ? 180 : 0;
    h = min(max(h, 0), 255);
    return (h <= 30 && v >= 100) || (s < 10 && v > 150) || (s < 30 && v > 180) || (s < 50 && v > 220);
}

// step 1: np.uint8(255 * x.clip(0, 1)) -- one fp32 multiply, then truncation (a NaN clips to 0)
D3R_DEV int to_u8(float x) { return (int)__fmul_rn(255.f, fminf(fmaxf(x, 0.f), 1.f)); }

D3R_DEV bool pixel_color(const void* rgb, int is_u8, size_t p) {
    if (is_u8) {
        const uint8_t* q = (const uint8_t*)rgb + 3 * p;
        return sky_color(q[0], q[1], q[2]);
    }
    const float* q = (const float*)rgb + 3 * p;
    return sky_color(to_u8(q[0]), to_u8(q[1]), to_u8(q[2]));
}

using scene::area_of;        // an image's pixel count, 0 when its size is negative or does not fit its row: shared with mesh.hip and fuse.hip

__global__ __launch_bounds__(256) void sky_color_kernel(const void* __restrict__ rgb, int is_u8, const int* __restrict__ img_h,
                                                        const int* __restrict__ img_w, int max_area, uint8_t* __restrict__ out) {
    const int img = blockIdx.y;
    const int area = area_of(img_h[img], img_w[img], max_area);
    for (int p = blockIdx.x * 256 + threadIdx.x; p < max_area; p += gridDim.x * 256) {
        const size_t g = (size_t)img * max_area + p;
        out[g] = p < area ? pixel_color(rgb, is_u8, g) : 0;
    }
}

// LDS union-find of one tile: parents point to smaller indices, a link is a CAS on a root
D3R_DEV int lfind(int* L, int p) {
    int q = __hip_atomic_load(L + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (q != p) {
        p = q;
        q = __hip_atomic_load(L + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return p;
}

D3R_DEV void lunion(int* L, int a, int b) {
    while (true) {
        a = lfind(L, a);
        b = lfind(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        int expected = b;
        if (__hip_atomic_compare_exchange_strong(L + b, &expected, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;
    }
}

D3R_DEV int tiles_of(int H, int W, int max_area) { return area_of(H, W, max_area) ? ((H + T - 1) / T) * ((W + T - 1) / T) : 0; }

__global__ __launch_bounds__(NT) void sky_open_label_kernel(const void* __restrict__ rgb, int is_u8, const int* __restrict__ img_h,
                                                             const int* __restrict__ img_w, int max_area, int* __restrict__ labels,
                                                             int* __restrict__ areas) {
    __shared__ uint8_t cm[M][M];              // colour mask, 0 outside the image (scipy's border_value = 0)
    __shared__ uint8_t er[M][M - 4];          // row erosion
    __shared__ uint8_t ero[M - 4][M - 4];     // erosion, centred at tile coordinates -2 .. T+1
    __shared__ uint8_t dr[M - 4][T];          // row dilation
    __shared__ int lab[T * T];
    __shared__ int cnt[T * T];                // pixel count of each tile-local component, at its root
    const int img = blockIdx.y;
    const int H = img_h[img], W = img_w[img];
    const int tx_n = (W + T - 1) / T, n_tiles = tiles_of(H, W, max_area);
    const size_t base = (size_t)img * max_area;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int X0 = (tile % tx_n) * T, Y0 = (tile / tx_n) * T;
        __syncthreads();                      // the LDS of the previous tile is no longer read
        for (int k = threadIdx.x; k < M * M; k += NT) {
            const int my = k / M, mx = k % M, y = Y0 - HALO + my, x = X0 - HALO + mx;
            cm[my][mx] = (y >= 0 && y < H && x >= 0 && x < W) ? pixel_color(rgb, is_u8, base + (size_t)y * W + x) : 0;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < M * (M - 4); k += NT) {
            const int y = k / (M - 4), x = k % (M - 4);
            er[y][x] = cm[y][x] & cm[y][x + 1] & cm[y][x + 2] & cm[y][x + 3] & cm[y][x + 4];
        }
        __syncthreads();
        for (int k = threadIdx.x; k < (M - 4) * (M - 4); k += NT) {
            const int y = k / (M - 4), x = k % (M - 4);
            ero[y][x] = er[y][x] & er[y + 1][x] & er[y + 2][x] & er[y + 3][x] & er[y + 4][x];
        }
        __syncthreads();
        for (int k = threadIdx.x; k < (M - 4) * T; k += NT) {
            const int y = k / T, x = k % T;
            dr[y][x] = ero[y][x] | ero[y][x + 1] | ero[y][x + 2] | ero[y][x + 3] | ero[y][x + 4];
        }
        __syncthreads();
        for (int k = threadIdx.x; k < T * T; k += NT) {
            const int y = k / T, x = k % T;
            const bool fg = (dr[y][x] | dr[y + 1][x] | dr[y + 2][x] | dr[y + 3][x] | dr[y + 4][x]) && Y0 + y < H && X0 + x < W;
            lab[k] = fg ? k : -1;
            cnt[k] = 0;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < T * T; k += NT) {
            if (lab[k] < 0) continue;
            const int y = k / T, x = k % T;
            if (x > 0 && lab[k - 1] >= 0) lunion(lab, k, k - 1);
            if (y > 0) {
                if (x > 0 && lab[k - T - 1] >= 0) lunion(lab, k, k - T - 1);
                if (lab[k - T] >= 0) lunion(lab, k, k - T);
                if (x < T - 1 && lab[k - T + 1] >= 0) lunion(lab, k, k - T + 1);
            }
        }
        __syncthreads();
        for (int k = threadIdx.x; k < T * T; k += NT) {
            const int y = k / T, x = k % T;
            if (Y0 + y >= H || X0 + x >= W) continue;
            int out = -1;
            if (lab[k] >= 0) {
                const int r = lfind(lab, k);
                atomicAdd(cnt + r, 1);
                out = (Y0 + r / T) * W + X0 + r % T;      // tile order = image order: the root keeps the smallest index
            }
            labels[base + (size_t)(Y0 + y) * W + X0 + x] = out;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < T * T; k += NT)     // every local root is its own pixel: plain stores into the zeroed plane
            if (cnt[k]) areas[base + (size_t)(Y0 + k / T) * W + X0 + k % T] = cnt[k];
    }
}

// global union-find over one image's labels (L = the image's row), merge kernel only: path halving keeps the chains short. It is safe
// there because a halving store only replaces a non-root's parent by one of its ancestors, and links only ever rewrite roots.
D3R_DEV int gload(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

D3R_DEV int gfind(int* L, int p) {
    while (true) {
        const int q = gload(L + p);
        if (q == p) return p;
        const int g = gload(L + q);
        if (g != q) __hip_atomic_store(L + p, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // g is an ancestor of p: still a valid parent
        p = g;
    }
}

D3R_DEV void gunion(int* L, int a, int b) {
    while (true) {
        a = gfind(L, a);
        b = gfind(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        int expected = b;
        if (__hip_atomic_compare_exchange_strong(L + b, &expected, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

// one 64-lane wave per tile: lanes 0-31 walk the left column, lanes 32-63 the top row, and each links its pixel to every
// 8-neighbour that lies in another tile (every cross-tile pair has one end on a left column or a top row)
__global__ __launch_bounds__(64) void sky_merge_kernel(const int* __restrict__ img_h, const int* __restrict__ img_w, int max_area, int* labels) {
    const int img = blockIdx.y;
    const int H = img_h[img], W = img_w[img];
    const int tx_n = (W + T - 1) / T, n_tiles = tiles_of(H, W, max_area);
    int* L = labels + (size_t)img * max_area;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int X0 = (tile % tx_n) * T, Y0 = (tile / tx_n) * T;
        const int t = threadIdx.x & 31;
        const int x = threadIdx.x < 32 ? X0 : X0 + t, y = threadIdx.x < 32 ? Y0 + t : Y0;
        if (x >= W || y >= H) continue;
        if ((threadIdx.x < 32 && X0 == 0) || (threadIdx.x >= 32 && Y0 == 0)) continue;      // image border: nothing beyond
        const int p = y * W + x;
        if (gload(L + p) < 0) continue;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int yy = y + dy, xx = x + dx;
                if ((dx == 0 && dy == 0) || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                if (yy >= Y0 && yy < Y0 + T && xx >= X0 && xx < X0 + T) continue;           // same tile: linked already
                const int q = yy * W + xx;
                if (gload(L + q) >= 0) gunion(L, p, q);
            }
    }
}

// Roots are final once the merge kernel has ended. The root chase here is read-only, and the one store to L[p] is p's own root, made by
// p's thread: other threads chasing through p read either its old parent or its root, both valid, and L[p] ends as the root whatever
// the order. (Path halving here would let a thread store a stale grandparent over a root that p's thread has already written.)
// areas[p] holds the tile-local count at every tile-local root p and 0 elsewhere. A local root that is not a global root moves its count
// to its root; global roots are local roots that were never linked, so only they receive counts, and the exchange-then-add keeps every
// count whatever the order.
D3R_DEV int groot(const int* L, int p) {
    int q = gload(L + p);
    while (q != p) {
        p = q;
        q = gload(L + p);
    }
    return p;
}

__global__ __launch_bounds__(256) void sky_flatten_kernel(const int* __restrict__ img_h, const int* __restrict__ img_w, int max_area, int* labels,
                                                          int* areas) {
    const int img = blockIdx.y;
    const int area = area_of(img_h[img], img_w[img], max_area);
    int* L = labels + (size_t)img * max_area;
    int* A = areas + (size_t)img * max_area;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < area; p += gridDim.x * 256) {
        if (gload(L + p) < 0) continue;
        const int r = groot(L, p);
        if (r != p && gload(A + p) != 0) {
            const int c = __hip_atomic_exchange(A + p, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c) __hip_atomic_fetch_add(A + r, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void sky_amax_kernel(const int* __restrict__ img_h, const int* __restrict__ img_w, int max_area, const int* __restrict__ labels,
                                                       const int* __restrict__ areas, int* __restrict__ amax) {
    const int img = blockIdx.y;
    const int area = area_of(img_h[img], img_w[img], max_area);
    const size_t base = (size_t)img * max_area;
    int best = 0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < area; p += gridDim.x * 256)
        if (labels[base + p] == p) best = max(best, areas[base + p]);
    best = wave_reduce(best, [](int a, int b) { return max(a, b); });
    if ((threadIdx.x & 63) == 0 && best > 0) atomicMax(amax + img, best);
}

__global__ __launch_bounds__(256) void sky_select_kernel(const int* __restrict__ img_h, const int* __restrict__ img_w, int max_area, const int* __restrict__ labels,
                                                         const int* __restrict__ areas, const int* __restrict__ amax, uint8_t* __restrict__ out) {
    const int img = blockIdx.y;
    const int area = area_of(img_h[img], img_w[img], max_area);
    const size_t base = (size_t)img * max_area;
    const int a_max = amax[img];
    for (int p = blockIdx.x * 256 + threadIdx.x; p < max_area; p += gridDim.x * 256) {
        const int r = p < area ? labels[base + p] : -1;
        out[base + p] = r >= 0 && 2 * areas[base + r] > a_max;
    }
}

}  // namespace sky
}  // namespace d3r

using namespace d3r::sky;

extern "C" size_t d3r_segment_sky_workspace_bytes(int n_imgs, int max_area) {
    if (n_imgs <= 0 || max_area <= 0) return 0;
    return 2 * align256((size_t)n_imgs * max_area * sizeof(int)) + align256((size_t)n_imgs * sizeof(int));
}

// grid.x of the pixel kernels: enough workgroups for a 512 x 384 image at 4 pixels per thread, grid-stride beyond
static int pixel_blocks(int max_area) { return d3r::blocks_of(d3r::tiles_of(max_area, 1024), 1024); }

extern "C" int d3r_sky_color_mask(int n_imgs, const void* rgb, int rgb_is_u8, const int* img_h_dev, const int* img_w_dev, int max_area,
                                  uint8_t* mask_out, void* stream) {
    if (n_imgs <= 0 || n_imgs > 65535 || !rgb || !img_h_dev || !img_w_dev || max_area <= 0 || !mask_out) return D3R_ERR_INVALID;
    hipLaunchKernelGGL(sky_color_kernel, dim3(pixel_blocks(max_area), n_imgs), dim3(256), 0, (hipStream_t)stream, rgb, rgb_is_u8, img_h_dev, img_w_dev,
                       max_area, mask_out);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_segment_sky(int n_imgs, const void* rgb, int rgb_is_u8, const int* img_h_dev, const int* img_w_dev, int max_area, uint8_t* mask_out,
                               void* workspace, void* stream) {
    if (n_imgs <= 0 || n_imgs > 65535 || !rgb || !img_h_dev || !img_w_dev || max_area <= 0 || !mask_out || !workspace) return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const size_t plane = align256((size_t)n_imgs * max_area * sizeof(int));
    int* labels = (int*)workspace;
    int* areas = (int*)((char*)workspace + plane);
    int* amax = (int*)((char*)workspace + 2 * plane);
    if (hipMemsetAsync(areas, 0, plane + n_imgs * sizeof(int), st) != hipSuccess) return D3R_ERR_LAUNCH;
    // tile grids: a 512 x 384 image has 192 tiles; other sizes of the same area have about as many, the rest is grid-stride
    const int tile_blocks = (int)std::min<long long>(((long long)max_area + T * T - 1) / (T * T) + 16, 4096);
    const int pix = pixel_blocks(max_area);
    hipLaunchKernelGGL(sky_open_label_kernel, dim3(tile_blocks, n_imgs), dim3(NT), 0, st, rgb, rgb_is_u8, img_h_dev, img_w_dev, max_area, labels, areas);
    hipLaunchKernelGGL(sky_merge_kernel, dim3(tile_blocks, n_imgs), dim3(64), 0, st, img_h_dev, img_w_dev, max_area, labels);
    hipLaunchKernelGGL(sky_flatten_kernel, dim3(pix, n_imgs), dim3(256), 0, st, img_h_dev, img_w_dev, max_area, labels, areas);
    hipLaunchKernelGGL(sky_amax_kernel, dim3(pix, n_imgs), dim3(256), 0, st, img_h_dev, img_w_dev, max_area, labels, areas, amax);
    hipLaunchKernelGGL(sky_select_kernel, dim3(pix, n_imgs), dim3(256), 0, st, img_h_dev, img_w_dev, max_area, labels, areas, amax, mask_out);
    return rc_of(hipGetLastError());
}
