// dust3r_amd -- Conv2d(3x3, stride 1, pad 1) on the x2 bilinear map of a low-resolution NHWC split-fp16 map, the map interpolated inside the convolution
// (AMODE_CONV_UP2, kernels.hpp; gfx950). The DPT head's two such stages: head.0's output -> x2 -> 3x3 128 -> 128 + ReLU + 1x1 + postprocess (EPI_HEAD4), and
// refinenet-0's output -> x2 -> head.0 (3x3 256 -> 128, EPI_T), each in ONE launch: the 3.2 / 1.6 GB maps (32 pairs) are neither written by upsample2x_quad_kernel nor
// streamed back by the convolution. Bit-identical to that two-kernel route.
//
// A block owns a 16 x 32 tile of output pixels of one image; its eight waves are the 128 (n) x 64 (m) waves of gemm.hip's 512 x 128 tile (wave w: tile rows 2 w and
// 2 w + 1; fragment fj: row 2 w + fj / 2, columns 16 (fj & 1) ... + 15), so every wave holds all output channels of its pixels and EPI_HEAD4 applies unchanged;
// EPI_T stores typed rows through a wave-private LDS tile with the tile's row -> pixel map.
// Per 32-channel K slice:
//   1. the tile's SOURCE neighbourhood (at most 11 x 19 low-resolution pixels x 128 B) arrives in LDS by DMA, issued one slice ahead: right behind the patch build of
//      the previous slice, in flight during that slice's first K step (the second step's vmcnt(0) drains it with the weight rows);
//   2. every thread evaluates ~5 (pixel, 8-channel group) items of the 18 x 34 PATCH of map pixels around the tile with the stand-alone kernel's arithmetic
//      (kernels.hpp up2_*: rows interpolated along x, then along y, fp32; split2) and writes hi / lo chunks in the K loop's row image; pixels outside the map are
//      zero, which is the convolution's padding;
//   3. the nine taps run as nine K steps whose A fragments are read from the patch at the tap's offset while the weight rows stream through the two-slot ring of the
//      generic kernel. K order (slice, tap, channel) and the three MFMAs per product are those of gemm_kernel: the same sums in the same order.
// LDS: patch 612 x 128 B = 76.5 KiB | 2 x 16 KiB weight slots | 32 KiB source slot = 140.5 KiB, one block per CU.
// Patch swizzle: pixel q's chunk c sits at slot c ^ (q & 7) of its 128-byte row. A fragment read touches 16 CONSECUTIVE patch pixels q0 ... q0 + 15 of one patch row
// (q0 = any value: the three kx phases shift it by 0 / 1 / 2) and, per lane group, one chunk: checked against the ds_read_b128 service groups of gfx950
// ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, + 32) for all q0 mod 16 and both the hi and the lo chunk -- 16 distinct 16-byte slots of the 256-byte bank row in every
// group, i.e. conflict-free in all three phases. (The generic kernel's key (row >> 1) & 7 is conflict-free only for q0 = 0 mod 4 and 2-way elsewhere.)
#include <stdlib.h>

#include <atomic>

#include "kernels.hpp"
#include "gemm_head4.hpp"

namespace d3r {

namespace {
constexpr int TH = UP2_TILE_H, TW = UP2_TILE_W, PH = TH + 2, PW = TW + 2;      // tile and patch (tile + the 3x3 halo) in map pixels
constexpr int SH = TH / 2 + 3, SW = TW / 2 + 3;                                // source rows / columns a patch can touch: floor((PH - 1) / 2) + 2 starts, + 1 neighbour
constexpr int NT = 512, NPIX = PH * PW, NSRC = SH * SW;
constexpr int PATCH_BYTES = NPIX * 128, WSLOT = 128 * 128, SRC_PASSES = (NSRC * 8 + NT - 1) / NT, SRC_BYTES = SRC_PASSES * NT * 16;
constexpr int W_OFF = PATCH_BYTES, SRC_OFF = W_OFF + 2 * WSLOT, LDS_BYTES = SRC_OFF + SRC_BYTES;
constexpr int ITEMS = NPIX * 4, ITEM_PASSES = (ITEMS + NT - 1) / NT;           // (patch pixel, 8-channel group) items per slice
static_assert(TH == 16 && TW == 32, "eight waves of 64 pixels: two tile rows of two 16-pixel fragments each");
static_assert(LDS_BYTES <= 160 * 1024, "one block per CU");

D3R_DEV void lds_load8_x3(const char* p, float (&v)[8]) {      // load8<D3R_F16X3> on an LDS copy of a group [hi x8][lo x8]
    using TX = Traits<D3R_F16X3>;
    const uint4 h = *reinterpret_cast<const uint4*>(p), l = *reinterpret_cast<const uint4*>(p + 16);
    v[0] = TX::join_lo(h.x, l.x); v[1] = TX::join_hi(h.x, l.x); v[2] = TX::join_lo(h.y, l.y); v[3] = TX::join_hi(h.y, l.y);
    v[4] = TX::join_lo(h.z, l.z); v[5] = TX::join_hi(h.z, l.z); v[6] = TX::join_lo(h.w, l.w); v[7] = TX::join_hi(h.w, l.w);
}
}  // namespace

template <int EPI> __global__ __launch_bounds__(NT, 2) void conv_up2_kernel(GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using TR = Traits<D3R_F16X3>;
    constexpr int FI = 8, FJ = 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Ho = p.Hin, Wo = p.Win, Hi = Ho >> 1, Wi = Wo >> 1;
    // ---- block -> tile: XCD-contiguous ids, tiles of an image row by row (neighbours share their halo's source lines in one L2)
    const int tiles_x = Wo / TW, tiles_y = Ho / TH;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int b = lid / (tiles_x * tiles_y), rem = lid - b * (tiles_x * tiles_y);
    const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const float sh = up2_scale(Hi), sw = up2_scale(Wi);
    int sy_base, sx_base;       // first source row / column of the patch: the source index is monotonic in the output index
    {
        float l_, h_;
        up2_src(sh, max(oy0 - 1, 0), sy_base, l_, h_);
        up2_src(sw, max(ox0 - 1, 0), sx_base, l_, h_);
    }

    // ---- DMA sources: weight rows as in gemm_kernel (lane-linear LDS image, chunk ^= (row >> 1) & 7, [hi0..hi3 | lo0..lo3]); source pixels in memory order
    const int lrow = wave * 8 + (lane >> 3);
    const int lslot = (lane & 7) ^ ((lrow >> 1) & 7);
    const int lchunk = (lslot & 3) * 2 + (lslot >> 2);
    const char* wsrc[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) wsrc[q] = reinterpret_cast<const char*>(p.wgt) + ((size_t)(q * 64 + lrow) * p.K) * 4 + lchunk * 16;
    const char* ssrc[SRC_PASSES];
#pragma unroll
    for (int q = 0; q < SRC_PASSES; ++q) {
        const int it = q * NT + tid, sp = min(it >> 3, NSRC - 1), c = it & 7;      // items past the neighbourhood re-fetch its last pixel into the slot's slack
        const int sy = sp / SW, sx = sp - sy * SW;
        const int gy = min(sy_base + sy, Hi - 1), gx = min(sx_base + sx, Wi - 1);
        ssrc[q] = reinterpret_cast<const char*>(p.act) + (((size_t)b * Hi + gy) * Wi + gx) * (size_t)p.cstride * 4 + c * 16;
    }
    const uint32_t wave_u = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
    const uint32_t lds0 = lds_addr(smem) + wave_u * 1024;      // wave-uniform: one 1 KiB DMA piece per wave and pass
    auto stage_w = [&](int kt, int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 2; ++q) glds16(wsrc[q] + (size_t)kt * 128, lds0 + W_OFF + buf * WSLOT + q * (8 * 1024));
    };
    auto stage_src = [&](int sl) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < SRC_PASSES; ++q) glds16(ssrc[q] + (size_t)sl * 128, lds0 + SRC_OFF + q * (8 * 1024));
    };

    // ---- one item of the patch: map pixel (oy0 - 1 + py, ox0 - 1 + px), channels 8 g ... 8 g + 7 of the slice
    auto build_item = [&](int j) __attribute__((always_inline)) {
        const int pp = j >> 2, g = j & 3;
        const int py = pp / PW, px = pp - py * PW;
        const int oy = oy0 - 1 + py, ox = ox0 - 1 + px;
        uint4 h = make_uint4(0, 0, 0, 0), l = make_uint4(0, 0, 0, 0);
        if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) {
            int y0, x0;
            float ly, hy, lx, hx;
            up2_src(sh, oy, y0, ly, hy);
            up2_src(sw, ox, x0, lx, hx);
            const int y1 = min(y0 + 1, Hi - 1), x1 = min(x0 + 1, Wi - 1);
            const int r0 = min(y0 - sy_base, SH - 1) * SW, r1 = min(y1 - sy_base, SH - 1) * SW, c0 = min(x0 - sx_base, SW - 1), c1 = min(x1 - sx_base, SW - 1);
            const char* sb = smem + SRC_OFF + g * 32;
            float v00[8], v01[8], v10[8], v11[8], o[8];
            lds_load8_x3(sb + (r0 + c0) * 128, v00);
            lds_load8_x3(sb + (r0 + c1) * 128, v01);
            lds_load8_x3(sb + (r1 + c0) * 128, v10);
            lds_load8_x3(sb + (r1 + c1) * 128, v11);
            // which rounding form the stand-alone kernel gives this pixel (kernels.hpp up2_pixel_forms); both forms are evaluated, the choice is a register select
            int y0p;
            float l_, h_;
            up2_src(sh, max(oy - 1, 0), y0p, l_, h_);
            bool top_rev, y_rr;
            up2_pixel_forms(oy, ox, y0, y0p, top_rev, y_rr);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float t0n = up2_lerp(hx, v00[k], lx, v01[k]), t0r = up2_lerp_rev(hx, v00[k], lx, v01[k]), t1 = up2_lerp(hx, v10[k], lx, v11[k]);
                const float t0 = top_rev ? t0r : t0n;
                const float fused = up2_lerp(hy, t0, ly, t1), rr = up2_lerp_rr(hy, t0, ly, t1);
                o[k] = y_rr ? rr : fused;
            }
            TR::split2(o[0], o[1], h.x, l.x); TR::split2(o[2], o[3], h.y, l.y);
            TR::split2(o[4], o[5], h.z, l.z); TR::split2(o[6], o[7], h.w, l.w);
        }
        char* dst = smem + pp * 128;
        const int key = pp & 7;
        *reinterpret_cast<uint4*>(dst + ((g ^ key) << 4)) = h;
        *reinterpret_cast<uint4*>(dst + (((4 + g) ^ key) << 4)) = l;
    };

    // ---- fragment read addresses
    const int frow = lane & 15, fgrp = lane >> 4;
    const int wchi = (fgrp ^ ((frow >> 1) & 7)) * 16, wclo = ((4 + fgrp) ^ ((frow >> 1) & 7)) * 16;      // weight fragment rows start at multiples of 16
    int ppb[FJ];      // patch pixel of this lane's row of fragment fj at tap (0, 0)
#pragma unroll
    for (int fj = 0; fj < FJ; ++fj) ppb[fj] = (2 * wave + (fj >> 1)) * PW + (fj & 1) * 16 + frow;

    f32x4_t acc[FI][FJ];
#pragma unroll
    for (int a = 0; a < FI; ++a)
#pragma unroll
        for (int c = 0; c < FJ; ++c) acc[a][c] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    const int nsl = p.Cin >> 5, nk = nsl * 9;
    stage_src(0);
    stage_w(0, 0);
    __builtin_amdgcn_s_setprio(2);
    int buf = 0, kt = 0;
    for (int sl = 0; sl < nsl; ++sl) {
        d3r_wait_vm0();
        __syncthreads();      // the slice's source pixels (and the weight rows of its first step) have landed; every wave is done with the previous slice's patch
#pragma unroll 1
        for (int i = 0; i < ITEM_PASSES; ++i) {
            const int j = i * NT + tid;
            if (j < ITEMS) build_item(j);
        }
        __syncthreads();      // the patch is visible; the source slot is free
        if (sl + 1 < nsl) stage_src(sl + 1);
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap, ++kt) {
            if (tap > 0) {        // step kt's weight rows landed; every wave is done with the slot of step kt - 1
                d3r_wait_vm0();
                __syncthreads();
            }
            if (kt + 1 < nk) stage_w(kt + 1, buf ^ 1);
            const int ky = tap / 3, kx = tap - ky * 3;
            const int toff = ky * PW + kx;
            const char* wb = smem + W_OFF + buf * WSLOT;
            uint4 qf[FJ], ql[FJ];
#pragma unroll
            for (int fj = 0; fj < FJ; ++fj) {
                const int pp = ppb[fj] + toff, key = pp & 7;
                const char* qr = smem + pp * 128;
                qf[fj] = *reinterpret_cast<const uint4*>(qr + ((fgrp ^ key) << 4));
                ql[fj] = *reinterpret_cast<const uint4*>(qr + (((4 + fgrp) ^ key) << 4));
            }
#pragma unroll
            for (int fi = 0; fi < FI; ++fi) {
                const char* pr = wb + (frow + fi * 16) * 128;
                const uint4 pf = *reinterpret_cast<const uint4*>(pr + wchi), pl = *reinterpret_cast<const uint4*>(pr + wclo);
#pragma unroll
                for (int fj = 0; fj < FJ; ++fj) TR::mma16x3(acc[fi][fj], pf, pl, qf[fj], ql[fj]);
            }
            buf ^= 1;
        }
    }
    __builtin_amdgcn_s_setprio(0);

    if constexpr (EPI == EPI_HEAD4) {
        // ---- epilogue: the fused head tail on this lane's pixel
        float r4[4];
        head4_tail<FI, FJ>(p, acc, lane, r4);
        const int g = lane >> 4;
        const int oy = oy0 + 2 * wave + (g >> 1), ox = ox0 + (g & 1) * 16 + frow;
        const size_t m = ((size_t)b * Ho + oy) * Wo + ox;
        postprocess_store(r4[0], r4[1], r4[2], r4[3], reinterpret_cast<float*>(p.out), reinterpret_cast<float*>(p.out2), m, p.ldo, p.ldo2, p.post);
    } else {
        // ---- epilogue: typed store (EPI_T: bias, optional ReLU) as gemm_kernel's wide split-fp16 epilogue does it -- accumulators -> a wave-private [64 pixels][32
        // channels] LDS tile in the final byte layout -> whole 128-byte lines, 8 lanes per pixel. The value is that epilogue's fma(acc, 1, fma(0, 0, bias)).
        __syncthreads();      // every wave is done with the patch and the weight slots
        constexpr int WROW = 144;
        char* wreg = smem + wave * (64 * WROW);
        const float* bsrc = p.bias ? p.bias : reinterpret_cast<const float*>(p.wgt);
        const bool has_bias = p.bias != nullptr;
        const int i4 = (lane >> 4) * 4, rrow = lane >> 3, rch = lane & 7;
#pragma unroll
        for (int g = 0; g < FI / 2; ++g) {
            const int ig = g * 32;
            float4 bq[2];
#pragma unroll
            for (int fl = 0; fl < 2; ++fl) {
                const float4 t = *reinterpret_cast<const float4*>(bsrc + max(min(ig + fl * 16 + i4, p.n_store - 4), 0));
                bq[fl] = make_float4(has_bias ? t.x : 0.f, has_bias ? t.y : 0.f, has_bias ? t.z : 0.f, has_bias ? t.w : 0.f);
            }
#pragma unroll
            for (int fj = 0; fj < FJ; ++fj)
#pragma unroll
                for (int fl = 0; fl < 2; ++fl) {
                    const f32x4_t a = acc[g * 2 + fl][fj];
                    const float4 q4 = bq[fl];
                    float v0 = __builtin_fmaf(a[0], 1.f, __builtin_fmaf(0.f, 0.f, q4.x)), v1 = __builtin_fmaf(a[1], 1.f, __builtin_fmaf(0.f, 0.f, q4.y));
                    float v2 = __builtin_fmaf(a[2], 1.f, __builtin_fmaf(0.f, 0.f, q4.z)), v3 = __builtin_fmaf(a[3], 1.f, __builtin_fmaf(0.f, 0.f, q4.w));
                    if (p.flags & GF_RELU) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
                    uint2 hh, ll;
                    TR::split2(v0, v1, hh.x, ll.x);
                    TR::split2(v2, v3, hh.y, ll.y);
                    const int c0 = fl * 16 + i4;
                    char* w = wreg + (fj * 16 + frow) * WROW + (c0 >> 3) * 32 + (c0 & 7) * 2;
                    *reinterpret_cast<uint2*>(w) = hh;
                    *reinterpret_cast<uint2*>(w + 16) = ll;
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int pass = 0; pass < 8; ++pass) {
                const int row = pass * 8 + rrow, fj = row >> 4;
                const uint4 v = *reinterpret_cast<const uint4*>(wreg + row * WROW + rch * 16);
                const int oy = oy0 + 2 * wave + (fj >> 1), ox = ox0 + (fj & 1) * 16 + (row & 15);
                const size_t m = ((size_t)b * Ho + oy) * Wo + ox;
                const int i8 = ig + (rch >> 1) * 8;
                if (i8 < p.n_store) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(p.out) + (m * p.ldo + i8) * 4 + (rch & 1) * 16) = v;      // n_store % 8 == 0
            }
            asm volatile("" ::: "memory");
        }
    }
}

template <int EPI> static hipError_t launch_up2_t(const GemmParams& p, hipStream_t s) {
    static std::atomic<unsigned long long> attr_done{0};
    raise_dynamic_lds_once(attr_done, reinterpret_cast<const void*>(conv_up2_kernel<EPI>), LDS_BYTES);
    const int grid = (p.M / (p.Hin * p.Win)) * (p.Hin / TH) * (p.Win / TW);
    hipLaunchKernelGGL(conv_up2_kernel<EPI>, dim3(grid), dim3(NT), LDS_BYTES, s, p);
    return hipGetLastError();
}
hipError_t launch_conv_up2(const GemmParams& p, hipStream_t s) {
    if (!p.act || !p.wgt || !p.out) return hipErrorInvalidValue;
    if (p.epi == EPI_HEAD4) return p.res1 && p.res2 && p.out2 ? launch_up2_t<EPI_HEAD4>(p, s) : hipErrorInvalidValue;
    if (p.epi == EPI_T) return !p.res1 && !p.res2 && !p.out2 ? launch_up2_t<EPI_T>(p, s) : hipErrorInvalidValue;
    return hipErrorInvalidValue;
}

}  // namespace d3r
