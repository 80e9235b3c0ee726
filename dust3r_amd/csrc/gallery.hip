// dust3r_amd -- the depth / confidence gallery of the demo (the last lines of the reference's get_reconstructed_scene, dust3r/demo.py:168-184):
// every depth map divided by the maximum over ALL images, every confidence map divided by its maximum over all images and sent through
// matplotlib's `jet`, both then through rgb() (x * 0.5 + 0.5, clipped to [0, 1]); all images of a scene in one call.
//
// Layout: images are rows of [n][max_area] fp32 arrays (the scene's padded stacks), the pixel count of each image in a device table; what
// lies behind an image's count is never read into a result and never written. max_area is a multiple of 4 and every array 16-byte aligned,
// so every group of four pixels is one 16-byte access; the last group of an image with an odd count is handled element by element.
//   gallery_max_kernel     grid-stride over the groups of all images: the NaN-propagating maxima (numpy.max) of the valid depth and
//                          confidence pixels of this workgroup -> partials[2][blocks]. No float atomics.
//   gallery_image_kernel   every workgroup folds the partials (a maximum: the same value in every workgroup whatever the order) and copies
//                          the colour table into LDS, then per pixel
//                              depth_img = clip((d / dmax) * 0.5 + 0.5, 0, 1)          IEEE division, product and sum separately rounded
//                              conf_img  = table[lut_index(c / cmax)]                  gallery_math.hpp
//                          The table's rows already carry rgb()'s affine map (it acts on the looked-up colour, so it is a property of the
//                          row): 256 rows of float32(jet * 0.5 + 0.5) and the "bad" row (0.5, 0.5, 0.5, 0.5) that NaN -- 0 / 0 -- takes.
// The kernel boundary gives the visibility of the partials. This file is compiled with -ffp-contract=off: numpy rounds the product and
// the sum of the affine map separately, so no FMA may be formed from them.
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "reduce.hpp"
#include "gallery_math.hpp"

namespace d3r {
namespace gallery {

constexpr int NT = 256;             // threads per workgroup
constexpr int VEC = 4;              // pixels per thread and trip
constexpr int MAX_BLOCKS = 768;     // grid cap (3 workgroups per CU): one trip of the whole grid covers 768 * 256 * 4 pixels, grid-stride beyond

// an image's pixel count; 0 (the image is treated as empty) when it is negative or does not fit its row
D3R_DEV int npix_of(const int* __restrict__ npix, unsigned img, int max_area) {
    const int a = npix[img];
    return a >= 0 && a <= max_area ? a : 0;
}

// the workgroup's maxima -> every thread (red: 2 * NT / 64 floats of LDS), in the order of reduce.hpp
D3R_DEV void block_max2(float (&m)[2], float* red) {
    block_reduce_gather<NT, true>(m, red, [](float a, float b, int) { return nan_max(a, b); });
}

__global__ __launch_bounds__(NT) void gallery_max_kernel(const float* __restrict__ depth, const float* __restrict__ conf, const int* __restrict__ npix,
                                                         int n_imgs, int max_area, float* __restrict__ partials) {
    __shared__ float red[2 * NT / 64];
    const unsigned vpr = (unsigned)max_area / VEC, total = (unsigned)n_imgs * vpr;      // groups per row, groups in all (< 2^31: checked by the host)
    float m[2] = {-__builtin_huge_valf(), -__builtin_huge_valf()};                      // depth, confidence
    for (unsigned g = blockIdx.x * NT + threadIdx.x; g < total; g += gridDim.x * NT) {
        const unsigned img = g / vpr;
        const int p = (int)(g - img * vpr) * VEC, a = npix_of(npix, img, max_area);
        if (p >= a) continue;
        const size_t off = (size_t)img * max_area + p;
        const float4 d = *reinterpret_cast<const float4*>(depth + off), c = *reinterpret_cast<const float4*>(conf + off);
        const float dv[VEC] = {d.x, d.y, d.z, d.w}, cv[VEC] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if (p + k < a) {
                m[0] = nan_max(m[0], dv[k]);
                m[1] = nan_max(m[1], cv[k]);
            }
        }
    }
    block_max2(m, red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = m[0];
        partials[gridDim.x + blockIdx.x] = m[1];
    }
}

D3R_DEV float depth_value(float d, float dmax) {
    const float y = (d / dmax) * 0.5f + 0.5f;              // correctly rounded division; no contraction (see the head of the file)
    return y != y ? y : fminf(fmaxf(y, 0.f), 1.f);         // numpy's clip keeps NaN
}

__global__ __launch_bounds__(NT) void gallery_image_kernel(const float* __restrict__ depth, const float* __restrict__ conf, const int* __restrict__ npix,
                                                           int n_imgs, int max_area, const float* __restrict__ partials, int n_parts,
                                                           const float4* __restrict__ table, float* __restrict__ depth_img, float4* __restrict__ conf_img,
                                                           float* __restrict__ maxima_out) {
    __shared__ float4 lut[LUT_ROWS];
    __shared__ float red[2 * NT / 64];
    for (int i = threadIdx.x; i < LUT_ROWS; i += NT) lut[i] = table[i];
    float m[2] = {-__builtin_huge_valf(), -__builtin_huge_valf()};
    for (int i = threadIdx.x; i < n_parts; i += NT) {
        m[0] = nan_max(m[0], partials[i]);
        m[1] = nan_max(m[1], partials[n_parts + i]);
    }
    block_max2(m, red);                                    // its barrier also publishes lut
    const float dmax = m[0], cmax = m[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        maxima_out[0] = dmax;
        maxima_out[1] = cmax;
    }
    const unsigned vpr = (unsigned)max_area / VEC, total = (unsigned)n_imgs * vpr;
    for (unsigned g = blockIdx.x * NT + threadIdx.x; g < total; g += gridDim.x * NT) {
        const unsigned img = g / vpr;
        const int p = (int)(g - img * vpr) * VEC, a = npix_of(npix, img, max_area);
        if (p >= a) continue;
        const size_t off = (size_t)img * max_area + p;
        const float4 d = *reinterpret_cast<const float4*>(depth + off), c = *reinterpret_cast<const float4*>(conf + off);
        if (p + VEC <= a) {
            *reinterpret_cast<float4*>(depth_img + off) = make_float4(depth_value(d.x, dmax), depth_value(d.y, dmax), depth_value(d.z, dmax), depth_value(d.w, dmax));
            conf_img[off] = lut[lut_index(c.x / cmax)];
            conf_img[off + 1] = lut[lut_index(c.y / cmax)];
            conf_img[off + 2] = lut[lut_index(c.z / cmax)];
            conf_img[off + 3] = lut[lut_index(c.w / cmax)];
        } else {
            const float dv[VEC] = {d.x, d.y, d.z, d.w}, cv[VEC] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (int k = 0; k < VEC - 1; ++k) {
                if (p + k < a) {
                    depth_img[off + k] = depth_value(dv[k], dmax);
                    conf_img[off + k] = lut[lut_index(cv[k] / cmax)];
                }
            }
        }
    }
}

}  // namespace gallery
}  // namespace d3r

using namespace d3r::gallery;

static bool gallery_shape_ok(int n_imgs, int max_area) {
    return n_imgs > 0 && max_area > 0 && max_area % VEC == 0 && (long long)n_imgs * (max_area / VEC) <= 0x7FFFFFFFll;
}

static int gallery_blocks(int n_imgs, int max_area) {
    const long long groups = (long long)n_imgs * (max_area / VEC);
    return d3r::blocks_of(d3r::tiles_of(groups, NT), MAX_BLOCKS);
}

extern "C" void d3r_scene_gallery_launch_bound(int* max_blocks, int* threads, int* pixels_per_thread) {
    if (max_blocks) *max_blocks = MAX_BLOCKS;
    if (threads) *threads = NT;
    if (pixels_per_thread) *pixels_per_thread = VEC;
}

extern "C" size_t d3r_scene_gallery_workspace_bytes(int n_imgs, int max_area) {
    if (!gallery_shape_ok(n_imgs, max_area)) return 0;
    return align256((size_t)2 * gallery_blocks(n_imgs, max_area) * sizeof(float));
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int d3r_scene_gallery(int n_imgs, const float* depth, const float* conf, const int* npix_dev, int max_area, const float* table,
                                 float* depth_img, float* conf_img, float* maxima_out, void* workspace, void* stream) {
    if (!gallery_shape_ok(n_imgs, max_area) || !depth || !conf || !npix_dev || !table || !depth_img || !conf_img || !maxima_out || !workspace)
        return D3R_ERR_INVALID;
    if (!aligned16(depth) || !aligned16(conf) || !aligned16(table) || !aligned16(depth_img) || !aligned16(conf_img) || ((uintptr_t)maxima_out & 3) ||
        ((uintptr_t)npix_dev & 3) || ((uintptr_t)workspace & 3))
        return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = gallery_blocks(n_imgs, max_area);
    float* partials = (float*)workspace;
    hipLaunchKernelGGL(gallery_max_kernel, dim3(blocks), dim3(NT), 0, st, depth, conf, npix_dev, n_imgs, max_area, partials);
    hipLaunchKernelGGL(gallery_image_kernel, dim3(blocks), dim3(NT), 0, st, depth, conf, npix_dev, n_imgs, max_area, (const float*)partials, blocks,
                       (const float4*)table, depth_img, (float4*)conf_img, maxima_out);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_selftest_gallery_index_host(const float* ratios, int n, int* index_out) {
    if (n < 0 || (n > 0 && (!ratios || !index_out))) return D3R_ERR_INVALID;
    for (int i = 0; i < n; ++i) index_out[i] = lut_index(ratios[i]);
    return D3R_OK;
}
