// dust3r_amd -- a z-buffered software rasteriser for points and triangles, F cameras in one call: what scene.show(), scene.render_views()
// and demo.render_turntable draw with (dust3r_amd/viz.py render_batch). The reference's show() opens a trimesh / pyglet window; this is
// its headless counterpart and has no model in the reference.
//
// Two stages, so that the second can be checked exactly:
//   vertex stage (fp32)   X = R p + t as one fma chain per row, x = fx (X / Z) + cx, y likewise; sx = rint(16 x), sy = rint(16 y) as int32;
//                         zq = ZQ_MAX - rint((near / Z) ZQ_MAX). A vertex is INVALID (zq = 0xFFFFFFFF) when a coordinate of p is not finite,
//                         when not Z > near, or when not |x|, |y| <= GUARD px. There is no near-plane clipping: a face with an invalid
//                         vertex is dropped whole.
//   raster stage (integer only)  from (sx, sy, zq) on: coverage, depth and colour use int32 / int64 arithmetic alone.
// Conventions:
//   * pixel (px, py) has its centre at image coordinates (px, py) -- dust3r's (xy_grid; principal point W/2, H/2; pixel (u, v) of a
//     pointmap unprojects from exactly (u, v)) -- and covers [px - 1/2, px + 1/2): a point lands on pixel floor((sx + 8) / 16);
//   * zq is linear in 1 / Z, hence linear in screen space, and is interpolated with integer barycentrics; smaller = nearer;
//   * the frame buffer holds one uint64 key per pixel, (zq << 32) | primitive id, all ones = nothing drawn, lowered with atomicMin
//     (one global_atomic_umin_x2 on gfx950, no compare-and-swap loop). The minimum does not depend on arrival order: the same image on every
//     run; at equal depth the lower id wins. A plain load in front of the atomic skips it when the stored key is already smaller (the key
//     only ever decreases, so a stale value can only cause a redundant atomic, never a lost one);
//   * a face is sampled at the pixel centres (16 px, 16 py) with the TOP-LEFT fill rule: two faces that share an edge cover every pixel
//     exactly once. Both windings are drawn (no culling), zero-area faces are skipped. With the vertices ordered so that
//     area2 = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) > 0 and w0, w1, w2 the edge functions opposite v0, v1, v2 (w0 + w1 + w2 = area2):
//     a sample is covered when every w_k > 0, or = 0 on an edge (a -> b) that goes up (by < ay) or runs level to the right (by = ay, bx > ax);
//     zq = (w0 zq0 + w1 zq1 + w2 zq2) / area2 and each colour channel (w0 c0 + w1 c1 + w2 c2 + area2 / 2) / area2, integer divisions.
// Bounds: |sx|, |sy| <= 16 GUARD = 2^17 and the samples lie inside that range too (W, H <= GUARD), so coordinate differences are < 2^18 + 1,
// an edge function < 2^37 in magnitude, area2 < 2^37, and with zq < 2^24 the sums area2 zq < 2^61 and area2 255 + area2 / 2 < 2^46 fit int64.
#include "../../include/dust3r_hip.h"
#include "common.hpp"

namespace d3r {
namespace render {

constexpr int NT = 256;
constexpr float GUARD = 8192.f;               // px; W, H <= 8192
constexpr uint32_t ZQ_MAX = 0xFFFFFFu;        // D = 24 bits
constexpr uint32_t INVALID = 0xFFFFFFFFu;
constexpr unsigned long long EMPTY = ~0ull;
constexpr int SMALL_BOX = 64;                 // a face whose clipped bounding box has more samples than this is shared by its whole wave

struct Cam {
    float r[12];            // world -> camera, rows [R | t]
    float fx, fy, cx, cy;
};

D3R_DEV Cam load_cam(const float* __restrict__ w2c, int stride, const float* __restrict__ intr, int f) {
    Cam c;
#pragma unroll
    for (int k = 0; k < 12; ++k) c.r[k] = w2c[(size_t)f * stride + k];
    c.fx = intr[4 * f];
    c.fy = intr[4 * f + 1];
    c.cx = intr[4 * f + 2];
    c.cy = intr[4 * f + 3];
    return c;
}

struct Vtx {
    int sx, sy;
    uint32_t zq;
};

// the vertex stage: explicit fma / mul / div so that every kernel of this file rounds alike
D3R_DEV Vtx project(const Cam& c, float px, float py, float pz, float near) {
    Vtx v = {0, 0, INVALID};
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return v;
    const float X = __fmaf_rn(c.r[0], px, __fmaf_rn(c.r[1], py, __fmaf_rn(c.r[2], pz, c.r[3])));
    const float Y = __fmaf_rn(c.r[4], px, __fmaf_rn(c.r[5], py, __fmaf_rn(c.r[6], pz, c.r[7])));
    const float Z = __fmaf_rn(c.r[8], px, __fmaf_rn(c.r[9], py, __fmaf_rn(c.r[10], pz, c.r[11])));
    if (!(Z > near)) return v;
    const float x = __fmaf_rn(c.fx, __fdiv_rn(X, Z), c.cx);
    const float y = __fmaf_rn(c.fy, __fdiv_rn(Y, Z), c.cy);
    if (!(fabsf(x) <= GUARD && fabsf(y) <= GUARD)) return v;
    v.sx = __float2int_rn(__fmul_rn(16.f, x));
    v.sy = __float2int_rn(__fmul_rn(16.f, y));
    v.zq = ZQ_MAX - (uint32_t)__float2int_rn(__fmul_rn(__fdiv_rn(near, Z), (float)ZQ_MAX));
    return v;
}

D3R_DEV float depth_of(uint32_t zq, float near) { return __fdiv_rn(__fmul_rn(near, (float)ZQ_MAX), (float)(ZQ_MAX - zq)); }

// lower the key of one pixel; stats[0] counts the candidates, stats[1] the atomics that were issued
template <bool STATS> D3R_DEV void put(unsigned long long* __restrict__ fb, size_t at, unsigned long long key, unsigned long long* stats) {
    if (STATS) atomicAdd(stats, 1ull);
    if (fb[at] <= key) return;
    if (STATS) atomicAdd(stats + 1, 1ull);
    atomicMin(fb + at, key);
}

// ---- vertex stage on its own ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void render_project_kernel(int n_vert, const float* __restrict__ pos, const float* __restrict__ w2c, int stride,
                                                           const float* __restrict__ intr, float near, int* __restrict__ sxy, uint32_t* __restrict__ zq) {
    const int f = blockIdx.y;
    const Cam c = load_cam(w2c, stride, intr, f);
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < (size_t)n_vert; i += (size_t)gridDim.x * NT) {
        const Vtx v = project(c, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], near);
        const size_t o = (size_t)f * n_vert + i;
        sxy[2 * o] = v.sx;
        sxy[2 * o + 1] = v.sy;
        zq[o] = v.zq;
    }
}

// ---- points: a thread holds one point and walks the cameras f = blockIdx.y, + gridDim.y, ... (the point is read once) ---------------
template <bool STATS>
__global__ __launch_bounds__(NT) void render_points_kernel(int n_points, const float* __restrict__ pos, const uint8_t* __restrict__ mask, uint32_t id_base,
                                                          int n_cams, const float* __restrict__ w2c, int stride, const float* __restrict__ intr,
                                                          float near, int W, int H, int point_size, unsigned long long* __restrict__ fb,
                                                          unsigned long long* stats) {
    const int lo = -((point_size - 1) / 2), hi = point_size / 2;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < (size_t)n_points; i += (size_t)gridDim.x * NT) {
        if (mask && !mask[i]) continue;
        const float px = pos[3 * i], py = pos[3 * i + 1], pz = pos[3 * i + 2];
        for (int f = blockIdx.y; f < n_cams; f += gridDim.y) {
            const Cam c = load_cam(w2c, stride, intr, f);
            const Vtx v = project(c, px, py, pz, near);
            if (v.zq == INVALID) continue;
            const int bx = (v.sx + 8) >> 4, by = (v.sy + 8) >> 4;
            const unsigned long long key = ((unsigned long long)v.zq << 32) | (id_base + (uint32_t)i);
            const int y0 = max(by + lo, 0), y1 = min(by + hi, H - 1), x0 = max(bx + lo, 0), x1 = min(bx + hi, W - 1);
            for (int y = y0; y <= y1; ++y)
                for (int x = x0; x <= x1; ++x) put<STATS>(fb, ((size_t)f * H + y) * W + x, key, stats);
        }
    }
}

// ---- triangles ----------------------------------------------------------------------------------------------------------------------
struct Face {
    int x0, y0, x1, y1, x2, y2;      // ordered so that area2 > 0
    uint32_t z0, z1, z2;
    long long area2;                 // 0: nothing to draw
    bool swapped;                    // v1 and v2 were exchanged
};

D3R_DEV long long edge(int ax, int ay, int bx, int by, int px, int py) {
    return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}
D3R_DEV bool top_left(int ax, int ay, int bx, int by) { return by < ay || (by == ay && bx > ax); }

D3R_DEV Face make_face(Vtx a, Vtx b, Vtx c) {
    Face t = {};
    t.x0 = a.sx; t.y0 = a.sy; t.z0 = a.zq;
    t.x1 = b.sx; t.y1 = b.sy; t.z1 = b.zq;
    t.x2 = c.sx; t.y2 = c.sy; t.z2 = c.zq;
    if (a.zq == INVALID || b.zq == INVALID || c.zq == INVALID) return t;
    long long area2 = edge(a.sx, a.sy, b.sx, b.sy, c.sx, c.sy);
    if (area2 < 0) {
        t.x1 = c.sx; t.y1 = c.sy; t.z1 = c.zq;
        t.x2 = b.sx; t.y2 = b.sy; t.z2 = b.zq;
        t.swapped = true;
        area2 = -area2;
    }
    t.area2 = area2;
    return t;
}

// the sample at pixel (px, py): covered? its weights
D3R_DEV bool sample(const Face& t, int px, int py, long long& w0, long long& w1, long long& w2) {
    const int qx = 16 * px, qy = 16 * py;
    w0 = edge(t.x1, t.y1, t.x2, t.y2, qx, qy);
    w1 = edge(t.x2, t.y2, t.x0, t.y0, qx, qy);
    w2 = edge(t.x0, t.y0, t.x1, t.y1, qx, qy);
    if (w0 < 0 || w1 < 0 || w2 < 0) return false;
    if (w0 == 0 && !top_left(t.x1, t.y1, t.x2, t.y2)) return false;
    if (w1 == 0 && !top_left(t.x2, t.y2, t.x0, t.y0)) return false;
    if (w2 == 0 && !top_left(t.x0, t.y0, t.x1, t.y1)) return false;
    return true;
}

D3R_DEV uint32_t sample_zq(const Face& t, long long w0, long long w1, long long w2) {
    return (uint32_t)((w0 * (long long)t.z0 + w1 * (long long)t.z1 + w2 * (long long)t.z2) / t.area2);
}

// the pixels whose centres can lie inside the face, clipped to the frame (empty when bx0 > bx1 or by0 > by1)
D3R_DEV void pixel_box(const Face& t, int W, int H, int& bx0, int& by0, int& bx1, int& by1) {
    bx0 = max((min(t.x0, min(t.x1, t.x2)) + 15) >> 4, 0);
    by0 = max((min(t.y0, min(t.y1, t.y2)) + 15) >> 4, 0);
    bx1 = min(max(t.x0, max(t.x1, t.x2)) >> 4, W - 1);
    by1 = min(max(t.y0, max(t.y1, t.y2)) >> 4, H - 1);
}

D3R_DEV Face load_face(const uint32_t* __restrict__ faces, size_t j, int n_vert, const float* __restrict__ pos, const Cam& c, float near) {
    const uint32_t ia = faces[3 * j], ib = faces[3 * j + 1], ic = faces[3 * j + 2];
    if (ia >= (uint32_t)n_vert || ib >= (uint32_t)n_vert || ic >= (uint32_t)n_vert) return Face{};
    return make_face(project(c, pos[3 * (size_t)ia], pos[3 * (size_t)ia + 1], pos[3 * (size_t)ia + 2], near),
                     project(c, pos[3 * (size_t)ib], pos[3 * (size_t)ib + 1], pos[3 * (size_t)ib + 2], near),
                     project(c, pos[3 * (size_t)ic], pos[3 * (size_t)ic + 1], pos[3 * (size_t)ic + 2], near));
}

// One thread per (camera blockIdx.y, face). First pass: the thread draws its own face when the clipped box holds at most SMALL_BOX samples.
// Second pass, inside the same wave: the larger faces are taken one after the other, their data broadcast from the owning lane, and the 64
// lanes walk the box row by row, 64 samples at a time -- a lane sees at most ceil(W / 64) H samples of a face. (Narrowing each row to the
// span the face can reach was measured and lost: 94 instead of 80 registers, the mesh frame 17.9 instead of 15.4 ms, the glyphs no faster.)
template <bool STATS>
__global__ __launch_bounds__(NT) void render_triangles_kernel(int n_faces, const uint32_t* __restrict__ faces, int n_vert, const float* __restrict__ pos,
                                                             uint32_t id_base, const float* __restrict__ w2c, int stride, const float* __restrict__ intr,
                                                             float near, int W, int H, unsigned long long* __restrict__ fb, unsigned long long* stats) {
    const int f = blockIdx.y, lane = threadIdx.x & 63;
    const Cam c = load_cam(w2c, stride, intr, f);
    unsigned long long* img = fb + (size_t)f * H * W;
    const size_t n_round = ((size_t)n_faces + NT - 1) / NT * NT;             // whole workgroups: every lane of a wave reaches the ballot
    for (size_t j = (size_t)blockIdx.x * NT + threadIdx.x; j < n_round; j += (size_t)gridDim.x * NT) {
        Face t = {};
        int bx0 = 0, by0 = 0, bx1 = -1, by1 = -1;
        if (j < (size_t)n_faces) {
            t = load_face(faces, j, n_vert, pos, c, near);
            if (t.area2 > 0) pixel_box(t, W, H, bx0, by0, bx1, by1);
        }
        const bool any = t.area2 > 0 && bx0 <= bx1 && by0 <= by1;
        const bool large = any && (long long)(bx1 - bx0 + 1) * (by1 - by0 + 1) > SMALL_BOX;
        const uint32_t id = id_base + (uint32_t)j;
        if (any && !large) {
            for (int y = by0; y <= by1; ++y)
                for (int x = bx0; x <= bx1; ++x) {
                    long long w0, w1, w2;
                    if (sample(t, x, y, w0, w1, w2))
                        put<STATS>(img, (size_t)y * W + x, ((unsigned long long)sample_zq(t, w0, w1, w2) << 32) | id, stats);
                }
        }
        unsigned long long todo = __ballot(large);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            Face s = {};
            s.x0 = __shfl(t.x0, src); s.y0 = __shfl(t.y0, src); s.z0 = __shfl(t.z0, src);
            s.x1 = __shfl(t.x1, src); s.y1 = __shfl(t.y1, src); s.z1 = __shfl(t.z1, src);
            s.x2 = __shfl(t.x2, src); s.y2 = __shfl(t.y2, src); s.z2 = __shfl(t.z2, src);
            s.area2 = __shfl(t.area2, src);
            const int sx0 = __shfl(bx0, src), sy0 = __shfl(by0, src), sx1 = __shfl(bx1, src), sy1 = __shfl(by1, src);
            const uint32_t sid = __shfl(id, src);
            for (int y = sy0; y <= sy1; ++y)
                for (int x = sx0 + lane; x <= sx1; x += 64) {
                    long long w0, w1, w2;
                    if (sample(s, x, y, w0, w1, w2))
                        put<STATS>(img, (size_t)y * W + x, ((unsigned long long)sample_zq(s, w0, w1, w2) << 32) | sid, stats);
                }
        }
    }
}

// ---- resolve: key -> colour, depth, id ---------------------------------------------------------------------------------------------
D3R_DEV uint32_t mix(const Face& t, long long w0, long long w1, long long w2, uint32_t c0, uint32_t c1, uint32_t c2, int shift) {
    const long long a = (c0 >> shift) & 0xFF, b = (c1 >> shift) & 0xFF, c = (c2 >> shift) & 0xFF;
    return (uint32_t)((w0 * a + w1 * b + w2 * c + t.area2 / 2) / t.area2);
}

__global__ __launch_bounds__(NT) void render_resolve_kernel(const float* __restrict__ w2c, int stride, const float* __restrict__ intr, float near, int W, int H,
                                                           const unsigned long long* __restrict__ fb, int n_points, uint32_t point_id_base,
                                                           const uint32_t* __restrict__ point_rgba, int n_faces, uint32_t face_id_base,
                                                           const uint32_t* __restrict__ faces, int n_vert, const float* __restrict__ vert_pos,
                                                           const uint32_t* __restrict__ vert_rgba, uint32_t background, uint8_t* __restrict__ rgb_out,
                                                           float* __restrict__ depth_out, int* __restrict__ id_out) {
    const int f = blockIdx.y;
    const Cam c = load_cam(w2c, stride, intr, f);
    const size_t area = (size_t)H * W;
    for (size_t p = (size_t)blockIdx.x * NT + threadIdx.x; p < area; p += (size_t)gridDim.x * NT) {
        const size_t o = (size_t)f * area + p;
        const unsigned long long key = fb[o];
        uint32_t rgba = background;
        float depth = __builtin_huge_valf();
        int id = -1;
        if (key != EMPTY) {
            const uint32_t prim = (uint32_t)key, zq = (uint32_t)(key >> 32);
            id = (int)prim;
            depth = depth_of(zq, near);
            if (prim - point_id_base < (uint32_t)n_points) {
                rgba = point_rgba[prim - point_id_base];
            } else if (prim - face_id_base < (uint32_t)n_faces) {
                const size_t j = prim - face_id_base;
                const Face t = load_face(faces, j, n_vert, vert_pos, c, near);
                const int py = (int)(p / W), px = (int)(p - (size_t)py * W);
                long long w0, w1, w2;
                if (t.area2 > 0 && sample(t, px, py, w0, w1, w2)) {
                    const uint32_t c0 = vert_rgba[faces[3 * j]];
                    const uint32_t c1 = vert_rgba[faces[3 * j + (t.swapped ? 2 : 1)]], c2 = vert_rgba[faces[3 * j + (t.swapped ? 1 : 2)]];
                    rgba = mix(t, w0, w1, w2, c0, c1, c2, 0) | (mix(t, w0, w1, w2, c0, c1, c2, 8) << 8) | (mix(t, w0, w1, w2, c0, c1, c2, 16) << 16);
                }
            }
        }
        rgb_out[3 * o] = (uint8_t)rgba;
        rgb_out[3 * o + 1] = (uint8_t)(rgba >> 8);
        rgb_out[3 * o + 2] = (uint8_t)(rgba >> 16);
        if (depth_out) depth_out[o] = depth;
        if (id_out) id_out[o] = id;
    }
}

}  // namespace render
}  // namespace d3r

using namespace d3r::render;

static bool cams_ok(int n_cams, const float* w2c, int stride, const float* intr, float near) {
    return n_cams > 0 && n_cams <= 65535 && w2c && intr && (stride == 12 || stride == 16) && near > 0.f && near < __builtin_huge_valf();
}
static bool frame_ok(int W, int H) { return W > 0 && H > 0 && W <= (int)GUARD && H <= (int)GUARD; }
static int blocks_for(size_t n) { return (int)std::min<size_t>((n + NT - 1) / NT, 65536); }

extern "C" int d3r_render_project(int n_vert, const float* positions, int n_cams, const float* w2c, int w2c_stride, const float* intr, float near,
                                  int* sxy_out, uint32_t* zq_out, void* stream) {
    if (n_vert <= 0 || !positions || !cams_ok(n_cams, w2c, w2c_stride, intr, near) || !sxy_out || !zq_out) return D3R_ERR_INVALID;
    hipLaunchKernelGGL(render_project_kernel, dim3(blocks_for(n_vert), n_cams), dim3(NT), 0, (hipStream_t)stream, n_vert, positions, w2c, w2c_stride,
                       intr, near, sxy_out, zq_out);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_render_clear(int n_cams, int W, int H, unsigned long long* framebuffer, void* stream) {
    if (n_cams <= 0 || !frame_ok(W, H) || !framebuffer) return D3R_ERR_INVALID;
    return rc_of(hipMemsetAsync(framebuffer, 0xFF, (size_t)n_cams * W * H * sizeof(unsigned long long), (hipStream_t)stream));
}

extern "C" int d3r_render_points(int n_points, const float* positions, const uint8_t* mask, uint32_t id_base, int n_cams, const float* w2c,
                                 int w2c_stride, const float* intr, float near, int W, int H, int point_size, unsigned long long* framebuffer,
                                 unsigned long long* stats, void* stream) {
    if (n_points <= 0 || !positions || !cams_ok(n_cams, w2c, w2c_stride, intr, near) || !frame_ok(W, H) || point_size < 1 || point_size > 16 ||
        !framebuffer || (unsigned long long)id_base + (unsigned long long)n_points > 0x7FFFFFFFull)
        return D3R_ERR_INVALID;
    // a thread walks cameras blockIdx.y, + gridDim.y, ...: one row of the grid when the points alone fill the chip, more for small clouds
    const int gy = (int)std::min<long long>(n_cams, std::max<long long>(1, (1ll << 20) / n_points));
    const dim3 grid(blocks_for(n_points), gy);
    if (stats)
        hipLaunchKernelGGL(render_points_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, n_points, positions, mask, id_base, n_cams, w2c, w2c_stride,
                           intr, near, W, H, point_size, framebuffer, stats);
    else
        hipLaunchKernelGGL(render_points_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, n_points, positions, mask, id_base, n_cams, w2c, w2c_stride,
                           intr, near, W, H, point_size, framebuffer, stats);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_render_triangles(int n_faces, const uint32_t* faces, int n_vert, const float* positions, uint32_t id_base, int n_cams,
                                    const float* w2c, int w2c_stride, const float* intr, float near, int W, int H, unsigned long long* framebuffer,
                                    unsigned long long* stats, void* stream) {
    if (n_faces <= 0 || !faces || n_vert <= 0 || !positions || !cams_ok(n_cams, w2c, w2c_stride, intr, near) || !frame_ok(W, H) || !framebuffer ||
        (unsigned long long)id_base + (unsigned long long)n_faces > 0x7FFFFFFFull)
        return D3R_ERR_INVALID;
    const dim3 grid(blocks_for(n_faces), n_cams);
    if (stats)
        hipLaunchKernelGGL(render_triangles_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, n_faces, faces, n_vert, positions, id_base, w2c, w2c_stride,
                           intr, near, W, H, framebuffer, stats);
    else
        hipLaunchKernelGGL(render_triangles_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, n_faces, faces, n_vert, positions, id_base, w2c, w2c_stride,
                           intr, near, W, H, framebuffer, stats);
    return rc_of(hipGetLastError());
}

extern "C" int d3r_render_resolve(int n_cams, const float* w2c, int w2c_stride, const float* intr, float near, int W, int H,
                                  const unsigned long long* framebuffer, int n_points, uint32_t point_id_base, const uint32_t* point_rgba, int n_faces,
                                  uint32_t face_id_base, const uint32_t* faces, int n_vert, const float* vert_positions, const uint32_t* vert_rgba,
                                  uint32_t background_rgba, uint8_t* rgb_out, float* depth_out, int* id_out, void* stream) {
    if (!cams_ok(n_cams, w2c, w2c_stride, intr, near) || !frame_ok(W, H) || !framebuffer || !rgb_out || n_points < 0 || n_faces < 0 ||
        (n_points > 0 && !point_rgba) || (n_faces > 0 && (!faces || !vert_positions || !vert_rgba || n_vert <= 0)))
        return D3R_ERR_INVALID;
    hipLaunchKernelGGL(render_resolve_kernel, dim3(blocks_for((size_t)W * H), n_cams), dim3(NT), 0, (hipStream_t)stream, w2c, w2c_stride, intr, near, W, H,
                       framebuffer, n_points, point_id_base, point_rgba, n_faces, face_id_base, faces, n_vert, vert_positions, vert_rgba, background_rgba,
                       rgb_out, depth_out, id_out);
    return rc_of(hipGetLastError());
}
