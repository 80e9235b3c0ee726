// dust3r_amd -- dataset views prepared on the GPU, one call per batch (d3r_prepare_views, include/dust3r_hip.h).
//
// Three kernels over all the views of a batch (blockIdx.z = view). The vertical and depth kernels stream; the horizontal pass is bound by
// its LDS tap reads and integer multiply-adds (about 49 taps x 3 channels per intermediate sample for 12-megapixel sources), not by memory:
//   views_horizontal_kernel  source bytes -> uint8 intermediate [nrows][w][3] (only the rows and columns the final window needs).
//                            A block is 4 waves = 4 source rows x 64 output columns; each wave stages the run of source bytes its 64
//                            columns tap into LDS with aligned dword loads (every needed source byte is read from memory once per
//                            column tile; neighbouring tiles overlap by one filter support), then reads its taps from LDS.
//   views_vertical_kernel    intermediate -> img fp32 CHW: the vertical taps, ImgNorm through a 256-entry table (computed by torch, so
//                            the values are torch's), the HWC -> CHW layout and the portrait transpose folded into the store.
//   views_depth_kernel       one gather per output pixel through both crops (nearest neighbour), the back-projection to world
//                            coordinates and the validity mask.
// Lanes run along the OUTPUT row in the two kernels that write the results, so a wave stores 256 contiguous bytes per channel whether
// or not the view is transposed. No atomics, no scratch; the integer arithmetic and index rules live in views_math.hpp, shared with
// the host build that the CPU tests exercise.
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "views_math.hpp"

namespace d3r {
namespace vw {

constexpr int TILE_X = 64;      // output columns of a block = lanes of a wave
constexpr int TILE_R = 4;       // rows of a block = waves

__global__ __launch_bounds__(TILE_X * TILE_R) void views_horizontal_kernel(const d3r_view_plan* __restrict__ plans, uint8_t* __restrict__ ws,
                                                                            int lds_stride) {
    extern __shared__ uint32_t lds32[];
    const d3r_view_plan* P = plans + blockIdx.z;
    const int w = P->w, nrows = P->nrows;
    const int x0 = blockIdx.x * TILE_X, r0 = blockIdx.y * TILE_R;
    if (x0 >= w || r0 >= nrows) return;                                   // uniform over the block
    const int lane = threadIdx.x & (TILE_X - 1), wave = threadIdx.x / TILE_X;
    const int r = r0 + wave;
    const bool row_ok = r < nrows;
    const int crop_w = P->crop_w, kxs = P->kxs, off_x = P->off_x, src_w = P->src_w;
    const int32_t* __restrict__ bx = P->bx;
    const uint8_t* __restrict__ rgb = P->rgb;
    const int xl = min(x0 + TILE_X - 1, w - 1);
    int first, cnt0, flast, clast;
    clamp_bounds(bx[2 * (off_x + x0)], bx[2 * (off_x + x0) + 1], crop_w, kxs, &first, &cnt0);
    clamp_bounds(bx[2 * (off_x + xl)], bx[2 * (off_x + xl) + 1], crop_w, kxs, &flast, &clast);
    const int span_px = max(max(flast + clast, first + cnt0) - first, 0);
    // the run of source bytes of this wave's row, staged from its aligned-down dword
    const long total = (long)src_w * P->src_h * 3;
    const long byte0 = row_ok ? ((long)(P->crop_t + P->row0 + r) * src_w + P->crop_l + first) * 3 : 0;
    const long a0 = byte0 & ~3L;
    const int lead = (int)(byte0 - a0);
    const int nd = row_ok ? min((span_px * 3 + lead + 3) / 4, lds_stride / 4) : 0;
    uint32_t* row32 = lds32 + wave * (lds_stride / 4);
    for (int i = lane; i < nd; i += TILE_X) {
        const long a = a0 + 4L * i;
        uint32_t v;
        if (a + 4 <= total) {
            v = *reinterpret_cast<const uint32_t*>(rgb + a);
        } else {                                                           // the last bytes of the picture: no read past its end
            v = 0;
            for (int j = 0; j < 4; ++j)
                if (a + j < total) v |= (uint32_t)rgb[a + j] << (8 * j);
        }
        row32[i] = v;
    }
    __syncthreads();
    const int x = x0 + lane;
    if (!row_ok || x >= w) return;
    int f, c;
    clamp_bounds(bx[2 * (off_x + x)], bx[2 * (off_x + x) + 1], crop_w, kxs, &f, &c);
    const int32_t* __restrict__ k = P->kx + (long)(off_x + x) * kxs;
    const int rel = lead + (f - first) * 3;                               // offset of the first tap in the staged run
    const bool staged = rel >= 0 && rel + c * 3 <= nd * 4;
    const uint8_t* src = staged ? reinterpret_cast<const uint8_t*>(row32) + rel : rgb + byte0 + (long)(f - first) * 3;
    uint8_t* out = ws + P->tmp_off + ((long)r * w + x) * 3;
    out[0] = clip8(tap_sum(src, 3, k, c));
    out[1] = clip8(tap_sum(src + 1, 3, k, c));
    out[2] = clip8(tap_sum(src + 2, 3, k, c));
}

// view coordinates (x, y) of the output pixel (ox, oy)
__device__ __forceinline__ void view_xy(const d3r_view_plan* P, int ox, int oy, int* x, int* y) {
    const bool t = P->transpose != 0;
    *x = t ? oy : ox;
    *y = t ? ox : oy;
}

__global__ __launch_bounds__(TILE_X * TILE_R) void views_vertical_kernel(const d3r_view_plan* __restrict__ plans, const uint8_t* __restrict__ ws,
                                                                          const float* __restrict__ norm_lut, float* __restrict__ img, int H, int W) {
    __shared__ float lut[256];
    lut[threadIdx.x] = norm_lut[threadIdx.x];
    __syncthreads();
    const d3r_view_plan* P = plans + blockIdx.z;
    const int ox = blockIdx.x * TILE_X + (threadIdx.x & (TILE_X - 1)), oy = blockIdx.y * TILE_R + threadIdx.x / TILE_X;
    if (ox >= W || oy >= H) return;
    int x, y;
    view_xy(P, ox, oy, &x, &y);
    const int w = P->w, kys = P->kys, row0 = P->row0, nrows = P->nrows;
    const int rsy = P->off_y + y;
    int f, c;
    clamp_bounds(P->by[2 * rsy], P->by[2 * rsy + 1], P->crop_h, kys, &f, &c);
    const int lo = max(f, row0), hi = min(f + c, row0 + nrows);          // a consistent plan keeps every tap: lo == f, hi == f + c
    const int32_t* __restrict__ k = P->ky + (long)rsy * kys + (lo - f);
    const uint8_t* src = ws + P->tmp_off + ((long)(lo - row0) * w + x) * 3;
    const int n = max(hi - lo, 0), stride = w * 3;
    const size_t plane = (size_t)H * W;
    float* o = img + (size_t)blockIdx.z * 3 * plane + (size_t)oy * W + ox;
    o[0] = lut[clip8(tap_sum(src, stride, k, n))];
    o[plane] = lut[clip8(tap_sum(src + 1, stride, k, n))];
    o[2 * plane] = lut[clip8(tap_sum(src + 2, stride, k, n))];
}

// the depth sample, world point and mask of view pixel (x, y); shared with the host self test
__host__ __device__ inline void depth_sample(const d3r_view_plan* P, int x, int y, float* z_out, float* world, uint8_t* valid) {
    const int sx = nearest_index(P->off_x + x, P->crop_w, P->rs_w), sy = nearest_index(P->off_y + y, P->crop_h, P->rs_h);
    const float z = P->depth[(long)(P->crop_t + sy) * P->src_w + P->crop_l + sx];
    backproject(x, y, z, P->fu, P->fv, P->cu, P->cv, P->pose, world);
    *z_out = z;
    *valid = (uint8_t)(z > 0.0f && finite3(world));
}

__global__ __launch_bounds__(TILE_X * TILE_R) void views_depth_kernel(const d3r_view_plan* __restrict__ plans, float* __restrict__ depthmap,
                                                                       float* __restrict__ pts3d, uint8_t* __restrict__ valid_mask, int H, int W) {
    const d3r_view_plan* P = plans + blockIdx.z;
    const int ox = blockIdx.x * TILE_X + (threadIdx.x & (TILE_X - 1)), oy = blockIdx.y * TILE_R + threadIdx.x / TILE_X;
    if (ox >= W || oy >= H) return;
    int x, y;
    view_xy(P, ox, oy, &x, &y);
    float z, p[3];
    uint8_t ok;
    depth_sample(P, x, y, &z, p, &ok);
    const size_t i = ((size_t)blockIdx.z * H + oy) * W + ox;
    depthmap[i] = z;
    pts3d[3 * i] = p[0];
    pts3d[3 * i + 1] = p[1];
    pts3d[3 * i + 2] = p[2];
    valid_mask[i] = ok;
}

// every index the kernels form from this plan stays inside its buffers (the tables' contents are clamped by the kernels themselves)
static bool plan_ok(const d3r_view_plan& p, int H, int W, size_t workspace_bytes) {
    if (!p.rgb || !p.depth || !p.kx || !p.bx || !p.ky || !p.by || ((uintptr_t)p.rgb & 3)) return false;
    if (p.src_w <= 0 || p.src_h <= 0 || p.src_w > (1 << 15) || p.src_h > (1 << 15)) return false;
    if (p.crop_l < 0 || p.crop_t < 0 || p.crop_w <= 0 || p.crop_h <= 0 || p.crop_l + p.crop_w > p.src_w || p.crop_t + p.crop_h > p.src_h) return false;
    if (p.rs_w <= 0 || p.rs_h <= 0 || p.rs_w > (1 << 15) || p.rs_h > (1 << 15) || p.kxs <= 0 || p.kys <= 0 || p.kxs > (1 << 14) || p.kys > (1 << 14)) return false;
    if (p.w <= 0 || p.h <= 0 || p.off_x < 0 || p.off_y < 0 || p.off_x + p.w > p.rs_w || p.off_y + p.h > p.rs_h) return false;
    if (p.transpose ? (p.w != H || p.h != W) : (p.w != W || p.h != H)) return false;
    if (p.row0 < 0 || p.nrows <= 0 || p.row0 + p.nrows > p.crop_h || p.tmp_off < 0) return false;
    return (size_t)p.tmp_off + (size_t)p.nrows * p.w * 3 <= workspace_bytes;
}

}  // namespace vw
}  // namespace d3r

using namespace d3r::vw;

extern "C" int d3r_view_plan_bytes(void) { return (int)sizeof(d3r_view_plan); }

extern "C" int d3r_prepare_views(int n, const d3r_view_plan* plans_host, const void* plans_dev, int H, int W, const float* norm_lut, void* workspace,
                                 size_t workspace_bytes, float* img, float* depthmap, float* pts3d, uint8_t* valid_mask, void* stream) {
    if (n <= 0 || n > 65535 || H <= 0 || W <= 0 || H > (1 << 15) || W > (1 << 15) || !plans_host || !plans_dev || !norm_lut || !workspace || !img ||
        !depthmap || !pts3d || !valid_mask)
        return D3R_ERR_INVALID;
    int max_rows = 0, span_bytes = 0;
    for (int v = 0; v < n; ++v) {
        const d3r_view_plan& p = plans_host[v];
        if (!plan_ok(p, H, W, workspace_bytes)) return D3R_ERR_INVALID;
        max_rows = p.nrows > max_rows ? p.nrows : max_rows;
        const long span_px = (long)(TILE_X - 1) * p.crop_w / p.rs_w + p.kxs + 4;      // what 64 neighbouring columns tap, at most
        const long bytes = span_px * 3 + 8;
        span_bytes = (int)(bytes > span_bytes ? bytes : span_bytes);
    }
    const int lds_stride = (span_bytes > 12288 ? 12288 : (span_bytes + 15) / 16 * 16);      // 4 rows within 48 KiB; longer runs take the global path
    hipStream_t st = (hipStream_t)stream;
    const d3r_view_plan* pd = (const d3r_view_plan*)plans_dev;
    const int maxw = H > W ? H : W;
    hipLaunchKernelGGL(views_horizontal_kernel, dim3((maxw + TILE_X - 1) / TILE_X, (max_rows + TILE_R - 1) / TILE_R, n), dim3(TILE_X * TILE_R),
                       (size_t)lds_stride * TILE_R, st, pd, (uint8_t*)workspace, lds_stride);
    const dim3 grid((W + TILE_X - 1) / TILE_X, (H + TILE_R - 1) / TILE_R, n);
    hipLaunchKernelGGL(views_vertical_kernel, grid, dim3(TILE_X * TILE_R), 0, st, pd, (const uint8_t*)workspace, norm_lut, img, H, W);
    hipLaunchKernelGGL(views_depth_kernel, grid, dim3(TILE_X * TILE_R), 0, st, pd, depthmap, pts3d, valid_mask, H, W);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_selftest_resample_host(const uint8_t* src, int src_w, int src_h, int crop_l, int crop_t, int crop_w, int crop_h, int rs_w, int rs_h,
                                          const int32_t* kx, const int32_t* bx, int kxs, const int32_t* ky, const int32_t* by, int kys, uint8_t* out) {
    if (!src || !kx || !bx || !ky || !by || !out || crop_l < 0 || crop_t < 0 || crop_w <= 0 || crop_h <= 0 || crop_l + crop_w > src_w ||
        crop_t + crop_h > src_h || rs_w <= 0 || rs_h <= 0 || kxs <= 0 || kys <= 0)
        return D3R_ERR_INVALID;
    uint8_t* tmp = (uint8_t*)malloc((size_t)crop_h * rs_w * 3);
    if (!tmp) return D3R_ERR_ALLOC;
    for (int r = 0; r < crop_h; ++r)
        for (int x = 0; x < rs_w; ++x) {
            int f, c;
            clamp_bounds(bx[2 * x], bx[2 * x + 1], crop_w, kxs, &f, &c);
            const uint8_t* p = src + ((size_t)(crop_t + r) * src_w + crop_l + f) * 3;
            for (int ch = 0; ch < 3; ++ch) tmp[((size_t)r * rs_w + x) * 3 + ch] = clip8(tap_sum(p + ch, 3, kx + (size_t)x * kxs, c));
        }
    for (int y = 0; y < rs_h; ++y) {
        int f, c;
        clamp_bounds(by[2 * y], by[2 * y + 1], crop_h, kys, &f, &c);
        for (int x = 0; x < rs_w; ++x)
            for (int ch = 0; ch < 3; ++ch)
                out[((size_t)y * rs_w + x) * 3 + ch] = clip8(tap_sum(tmp + ((size_t)f * rs_w + x) * 3 + ch, rs_w * 3, ky + (size_t)y * kys, c));
    }
    free(tmp);
    return D3R_OK;
}

extern "C" int d3r_selftest_depth_host(const d3r_view_plan* plan, int H, int W, float* depthmap, float* pts3d, uint8_t* valid_mask) {
    if (!plan || !plan->depth || !depthmap || !pts3d || !valid_mask || H <= 0 || W <= 0) return D3R_ERR_INVALID;
    const d3r_view_plan& p = *plan;
    if (p.crop_l < 0 || p.crop_t < 0 || p.crop_w <= 0 || p.crop_h <= 0 || p.crop_l + p.crop_w > p.src_w || p.crop_t + p.crop_h > p.src_h || p.rs_w <= 0 ||
        p.rs_h <= 0 || p.off_x < 0 || p.off_y < 0 || p.off_x + p.w > p.rs_w || p.off_y + p.h > p.rs_h || (p.transpose ? (p.w != H || p.h != W) : (p.w != W || p.h != H)))
        return D3R_ERR_INVALID;
    for (int oy = 0; oy < H; ++oy)
        for (int ox = 0; ox < W; ++ox) {
            const size_t i = (size_t)oy * W + ox;
            depth_sample(plan, p.transpose ? oy : ox, p.transpose ? ox : oy, depthmap + i, pts3d + 3 * i, valid_mask + i);
        }
    return D3R_OK;
}
