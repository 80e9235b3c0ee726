// dust3r_amd -- the geometry of the demo's GLB export (the reference's dust3r/demo.py:66-107 _convert_scene_output_to_glb: pts3d_to_trimesh
// per view + cat_meshes, dust3r/viz.py:38-87, or the masked point cloud), batched over all views of a scene in one call.
//
// Layout: views are rows of [n][max_area] arrays (row-major H x W inside a row), sizes in device arrays, like d3r_segment_sky. An
// ELEMENT is a quad (y, x) of the pixel grid in mesh mode -- (H - 1)(W - 1) per view, raster order -- or a pixel in point-cloud mode.
// A TILE is NT consecutive elements of one view. The compaction is stable and atomic-free:
//   mesh_count_kernel       per tile, the number of valid upper / lower triangles (mesh) or valid pixels (point cloud): ballot counts
//   mesh_scan_tiles_kernel  one wave per view: exclusive scan of its tile counts (in place) and the view's totals
//   mesh_scan_views_kernel  one wave: exclusive scans over the views of the face (or point) counts and of the vertex counts (h w each,
//                           valid or not: the reference keeps every vertex); the per-view counts for the host
//   mesh_scatter_kernel     recomputes the flags of each tile and places its elements with the block-wide ballot / popcount scan
//                           (block_scan_1024): faces of view v in the reference's four segments -- valid upper triangles in raster order,
//                           the same reversed, valid lower triangles, the same reversed --, or the masked points and their colours
//   mesh_color_kernel       (mesh) per vertex, a 3 x 3 stencil over the mask and the image: the integer mean of the colours of the valid
//                           faces that use it (upper triangle: its top-left pixel, lower: its bottom-right pixel), its own colour when no
//                           face uses it; the POSITION bounds over the vertices that a face uses
//   mesh_bounds_kernel      the per-workgroup bounds reduced in a fixed order
// Every kernel is grid-stride over tiles or pixels, so the host sizes no grid by image size. Integer arithmetic and fixed-order
// reductions: the same bytes on every run.
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "scene_common.hpp"

namespace d3r {
namespace mesh {

using namespace d3r::scene;      // NT, area_of, pixel_q, the bounds helpers: shared with fuse.hip

template <bool PC> D3R_DEV int elems_of(int H, int W, int max_area) {
    const int a = area_of(H, W, max_area);
    if (PC) return a;
    return a > 0 && H > 1 && W > 1 ? (H - 1) * (W - 1) : 0;
}

// flags of element e: upper / lower triangle of quad e (mesh), or the pixel's mask (point cloud, in `up`). A triangle is valid when its
// three pixels are: upper (p, p + 1, p + W), lower (p + 1, p + W, p + W + 1), p = the quad's top-left pixel.
template <bool PC> D3R_DEV void flags_of(const uint8_t* m, int W, int n, int e, bool& up, bool& lo) {
    up = lo = false;
    if (e >= n) return;
    if (PC) {
        up = m[e] != 0;
        return;
    }
    const int y = e / (W - 1), p = e + y;          // p = y W + x with x = e - y (W - 1)
    const bool b = m[p + 1] != 0, c = m[p + W] != 0;
    up = b && c && m[p] != 0;
    lo = b && c && m[p + W + 1] != 0;
}

template <bool PC>
__global__ __launch_bounds__(NT) void mesh_count_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ img_h, const int* __restrict__ img_w,
                                                       int max_area, int max_tiles, int* __restrict__ tile_cnt) {
    __shared__ int wave_sums[NT / 64];
    const int v = blockIdx.y;
    const int W = img_w[v], n = elems_of<PC>(img_h[v], W, max_area);
    const int tiles = (n + NT - 1) / NT;
    const uint8_t* m = mask + (size_t)v * max_area;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        bool up, lo;
        flags_of<PC>(m, W, n, t * NT + threadIdx.x, up, lo);
        int tu, tl = 0;
        block_scan_1024(up, wave_sums, &tu);
        if (!PC) block_scan_1024(lo, wave_sums, &tl);
        if (threadIdx.x == 0) {
            tile_cnt[((size_t)v * max_tiles + t) * 2] = tu;
            tile_cnt[((size_t)v * max_tiles + t) * 2 + 1] = tl;
        }
    }
}

template <bool PC>
__global__ __launch_bounds__(64) void mesh_scan_tiles_kernel(const int* __restrict__ img_h, const int* __restrict__ img_w, int max_area, int max_tiles,
                                                             int* __restrict__ tile_cnt, int* __restrict__ view_tot) {
    const int v = blockIdx.x, lane = threadIdx.x;
    const int tiles = (elems_of<PC>(img_h[v], img_w[v], max_area) + NT - 1) / NT;
    int* c = tile_cnt + (size_t)v * max_tiles * 2;
    int run_u = 0, run_l = 0;
    for (int t0 = 0; t0 < tiles; t0 += 64) {
        const int t = t0 + lane;
        const int u = t < tiles ? c[2 * t] : 0, l = t < tiles ? c[2 * t + 1] : 0;
        const int iu = wave_scan_inclusive(u, lane), il = wave_scan_inclusive(l, lane);
        if (t < tiles) {
            c[2 * t] = run_u + iu - u;
            c[2 * t + 1] = run_l + il - l;
        }
        run_u += __shfl(iu, 63);
        run_l += __shfl(il, 63);
    }
    if (lane == 0) {
        view_tot[2 * v] = run_u;
        view_tot[2 * v + 1] = run_l;
    }
}

template <bool PC>
__global__ __launch_bounds__(64) void mesh_scan_views_kernel(int n_views, const int* __restrict__ img_h, const int* __restrict__ img_w, int max_area,
                                                             const int* __restrict__ view_tot, long long* __restrict__ view_off,
                                                             long long* __restrict__ vert_off, long long* __restrict__ counts_out) {
    const int lane = threadIdx.x;
    long long run_f = 0, run_v = 0;
    for (int v0 = 0; v0 < n_views; v0 += 64) {
        const int v = v0 + lane;
        long long f = 0, a = 0;
        if (v < n_views) {
            f = PC ? (long long)view_tot[2 * v] : 2 * ((long long)view_tot[2 * v] + view_tot[2 * v + 1]);
            a = area_of(img_h[v], img_w[v], max_area);
        }
        const long long fi = wave_scan_inclusive(f, lane), ai = wave_scan_inclusive(a, lane);
        if (v < n_views) {
            view_off[v] = run_f + fi - f;
            vert_off[v] = run_v + ai - a;
            counts_out[v] = f;
        }
        run_f += __shfl(fi, 63);
        run_v += __shfl(ai, 63);
    }
}

// mesh: faces [F][3] uint32 (vertex indices offset by the running vertex count); point cloud: points [P][3] fp32, colours [P] RGBA8
// and this workgroup's bounds of the emitted points in partials[v][gridDim.x][6]
template <bool PC>
__global__ __launch_bounds__(NT) void mesh_scatter_kernel(const float* __restrict__ pts, const uint8_t* __restrict__ mask, const void* __restrict__ rgb, int is_u8,
                                                         const int* __restrict__ img_h, const int* __restrict__ img_w, int max_area, int max_tiles,
                                                         const int* __restrict__ tile_off, const int* __restrict__ view_tot,
                                                         const long long* __restrict__ view_off, const long long* __restrict__ vert_off,
                                                         uint32_t* __restrict__ faces, float* __restrict__ points, uint32_t* __restrict__ colors,
                                                         float* __restrict__ partials) {
    __shared__ int wave_sums[NT / 64];
    __shared__ float lds_b[NT / 64 * 6];
    const int v = blockIdx.y;
    const int W = img_w[v], n = elems_of<PC>(img_h[v], W, max_area);
    const int tiles = (n + NT - 1) / NT;
    const size_t base = (size_t)v * max_area;
    const uint8_t* m = mask + base;
    const long long f0 = view_off[v];
    const long long U = view_tot[2 * v], L = view_tot[2 * v + 1];
    const uint32_t v0 = (uint32_t)vert_off[v];
    float b[6];
    bounds_init(b);
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int e = t * NT + threadIdx.x;
        bool up, lo;
        flags_of<PC>(m, W, n, e, up, lo);
        int tu, tl;
        const int pu = block_scan_1024(up, wave_sums, &tu);
        const int pl = PC ? 0 : block_scan_1024(lo, wave_sums, &tl);
        const size_t to = ((size_t)v * max_tiles + t) * 2;
        if (PC) {
            if (up) {
                const size_t o = (size_t)(f0 + tile_off[to] + pu);
                const float* p = pts + 3 * (base + e);
                points[3 * o] = p[0];
                points[3 * o + 1] = p[1];
                points[3 * o + 2] = p[2];
                colors[o] = pixel_q(rgb, is_u8, base + e) | 0xFF000000u;
                bounds_add(b, p);
            }
        } else {
            const int y = e / (W - 1);
            const uint32_t i1 = v0 + (uint32_t)(e + y), i2 = i1 + 1, i3 = i1 + (uint32_t)W, i4 = i3 + 1;
            if (up) {
                uint32_t* f = faces + 3 * (size_t)(f0 + tile_off[to] + pu);
                f[0] = i1; f[1] = i2; f[2] = i3;
                f += 3 * U;
                f[0] = i3; f[1] = i2; f[2] = i1;
            }
            if (lo) {
                uint32_t* f = faces + 3 * (size_t)(f0 + 2 * U + tile_off[to + 1] + pl);
                f[0] = i2; f[1] = i3; f[2] = i4;
                f += 3 * L;
                f[0] = i4; f[1] = i3; f[2] = i2;
            }
        }
    }
    if (PC) block_bounds(b, lds_b, partials + ((size_t)v * gridDim.x + blockIdx.x) * 6);
}

__global__ __launch_bounds__(NT) void mesh_color_kernel(const float* __restrict__ pts, const uint8_t* __restrict__ mask, const void* __restrict__ rgb, int is_u8,
                                                       const int* __restrict__ img_h, const int* __restrict__ img_w, int max_area,
                                                       const long long* __restrict__ vert_off, uint32_t* __restrict__ colors, float* __restrict__ partials) {
    __shared__ float lds_b[NT / 64 * 6];
    const int v = blockIdx.y;
    const int H = img_h[v], W = img_w[v], area = area_of(H, W, max_area);
    const size_t base = (size_t)v * max_area;
    const uint8_t* m = mask + base;
    uint32_t* out = colors + vert_off[v];
    float b[6];
    bounds_init(b);
    for (int p = blockIdx.x * NT + threadIdx.x; p < area; p += gridDim.x * NT) {
        const int y = p / W, x = p - y * W;
        uint32_t sr = 0, sg = 0, sb = 0, k = 0;
        if (m[p]) {
            const bool up = y > 0, dn = y < H - 1, lf = x > 0, rt = x < W - 1;
            const bool mr = rt && m[p + 1], ml = lf && m[p - 1], md = dn && m[p + W], mu = up && m[p - W];
            const bool mdl = lf && dn && m[p + W - 1], mur = up && rt && m[p - W + 1];
            // the (up to) six faces that use pixel p, each with the pixel that gives its colour
            const bool use[6] = {mr && md, ml && mdl, mu && mur, mdl && md, mur && mr, mu && ml};
            const int src[6] = {p, p - 1, p - W, p + W, p + 1, p};
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                if (!use[j]) continue;
                const uint32_t q = pixel_q(rgb, is_u8, base + src[j]);
                sr += q & 0xFF;
                sg += (q >> 8) & 0xFF;
                sb += q >> 16;
                ++k;
            }
        }
        uint32_t rgba;
        if (k) {
            rgba = ((sr + k / 2) / k) | (((sg + k / 2) / k) << 8) | (((sb + k / 2) / k) << 16);
            bounds_add(b, pts + 3 * (base + p));
        } else {
            rgba = pixel_q(rgb, is_u8, base + p);
        }
        out[p] = rgba | 0xFF000000u;
    }
    block_bounds(b, lds_b, partials + ((size_t)v * gridDim.x + blockIdx.x) * 6);
}

__global__ __launch_bounds__(256) void mesh_bounds_kernel(int n_parts, const float* __restrict__ partials, float* __restrict__ bounds_out) {
    bounds_final<false>(n_parts, partials, nullptr, bounds_out, nullptr);
}

}  // namespace mesh
}  // namespace d3r

using namespace d3r;
using namespace d3r::mesh;

// grid.x of every tile / pixel launch, and the tiles a view can have: a 512 x 384 view has 192 tiles; grid-stride beyond 1024
static int mesh_tiles(int max_area) { return (int)tiles_of(max_area, NT); }
static int mesh_blocks(int max_area) { return blocks_of(mesh_tiles(max_area), 1024); }

struct MeshWorkspace {
    int* tile_cnt;          // [n][max_tiles][2]
    int* view_tot;          // [n][2]
    long long* view_off;    // [n]
    long long* vert_off;    // [n]
    float* partials;        // [n][blocks][6]
    size_t bytes;
};

static MeshWorkspace mesh_workspace(void* base, int n_views, int max_area) {
    MeshWorkspace w;
    Carver c(base);
    w.tile_cnt = c.take<int>((size_t)n_views * mesh_tiles(max_area) * 2);
    w.view_tot = c.take<int>((size_t)n_views * 2);
    w.view_off = c.take<long long>(n_views);
    w.vert_off = c.take<long long>(n_views);
    w.partials = c.take<float>((size_t)n_views * mesh_blocks(max_area) * 6);
    w.bytes = c.bytes;
    return w;
}

extern "C" size_t d3r_scene_mesh_workspace_bytes(int n_views, int max_area) {
    if (n_views <= 0 || max_area <= 0) return 0;
    return mesh_workspace(nullptr, n_views, max_area).bytes;
}

extern "C" int d3r_scene_mesh(int n_views, const float* pts, const uint8_t* mask, const void* rgb, int rgb_is_u8, const int* img_h_dev,
                              const int* img_w_dev, int max_area, int as_pointcloud, uint32_t* faces_out, float* points_out, uint32_t* colors_out,
                              long long* counts_out, float* bounds_out, void* workspace, void* stream) {
    if (n_views <= 0 || n_views > 65535 || !pts || !mask || !rgb || !img_h_dev || !img_w_dev || max_area <= 0 || !colors_out || !counts_out ||
        !bounds_out || !workspace || (as_pointcloud ? !points_out : !faces_out))
        return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const MeshWorkspace w = mesh_workspace(workspace, n_views, max_area);
    const int tiles = mesh_tiles(max_area), bx = mesh_blocks(max_area);
    const dim3 grid(bx, n_views);
    if (as_pointcloud) {
        hipLaunchKernelGGL(mesh_count_kernel<true>, grid, dim3(NT), 0, st, mask, img_h_dev, img_w_dev, max_area, tiles, w.tile_cnt);
        hipLaunchKernelGGL(mesh_scan_tiles_kernel<true>, dim3(n_views), dim3(64), 0, st, img_h_dev, img_w_dev, max_area, tiles, w.tile_cnt, w.view_tot);
        hipLaunchKernelGGL(mesh_scan_views_kernel<true>, dim3(1), dim3(64), 0, st, n_views, img_h_dev, img_w_dev, max_area, w.view_tot, w.view_off,
                           w.vert_off, counts_out);
        hipLaunchKernelGGL(mesh_scatter_kernel<true>, grid, dim3(NT), 0, st, pts, mask, rgb, rgb_is_u8, img_h_dev, img_w_dev, max_area, tiles,
                           w.tile_cnt, w.view_tot, w.view_off, w.vert_off, faces_out, points_out, colors_out, w.partials);
    } else {
        hipLaunchKernelGGL(mesh_count_kernel<false>, grid, dim3(NT), 0, st, mask, img_h_dev, img_w_dev, max_area, tiles, w.tile_cnt);
        hipLaunchKernelGGL(mesh_scan_tiles_kernel<false>, dim3(n_views), dim3(64), 0, st, img_h_dev, img_w_dev, max_area, tiles, w.tile_cnt, w.view_tot);
        hipLaunchKernelGGL(mesh_scan_views_kernel<false>, dim3(1), dim3(64), 0, st, n_views, img_h_dev, img_w_dev, max_area, w.view_tot, w.view_off,
                           w.vert_off, counts_out);
        hipLaunchKernelGGL(mesh_scatter_kernel<false>, grid, dim3(NT), 0, st, pts, mask, rgb, rgb_is_u8, img_h_dev, img_w_dev, max_area, tiles,
                           w.tile_cnt, w.view_tot, w.view_off, w.vert_off, faces_out, points_out, colors_out, w.partials);
        hipLaunchKernelGGL(mesh_color_kernel, grid, dim3(NT), 0, st, pts, mask, rgb, rgb_is_u8, img_h_dev, img_w_dev, max_area, w.vert_off, colors_out,
                           w.partials);
    }
    hipLaunchKernelGGL(mesh_bounds_kernel, dim3(1), dim3(256), 0, st, n_views * bx, w.partials, bounds_out);
    return rc_of(hipGetLastError());
}
