// dust3r_amd -- the fused DPT head tail (EPI_HEAD4, kernels.hpp) as ONE device function for the two kernels whose waves hold every output channel of their
// rows: gemm_kernel (gemm.hip: the 512 x 128 / 256 x 128 R tiles) and conv_up2_kernel (gemm_up2.hip: the same eight 128 (n) x 64 (m) waves on a
// two-dimensional pixel tile). Bias, ReLU (GF_RELU), Conv2d(C, 4, 1) on the fp32 accumulators, the 1x1 bias: `r` receives the four pre-activation values of
// the row this lane stores -- row lane_group * 16 + (lane & 15) of the wave's 64 -- and the caller hands them to postprocess_store with ITS row -> pixel map.
#pragma once
#include "kernels.hpp"

namespace d3r {

template <int FI, int FJ> D3R_DEV void head4_tail(const GemmParams& p, const f32x4_t (&acc)[FI][FJ], int lane, float (&r)[4]) {
    static_assert(FI == 8 && FJ == 4, "a wave of 128 (n) x 64 (m): one row fragment per lane group");
    const int i4 = (lane >> 4) * 4;  // first of this lane's 4 consecutive channels inside a fragment
    const float* hw = reinterpret_cast<const float*>(p.res1);
    const float* hb = reinterpret_cast<const float*>(p.res2);
    const float* bsrc = p.bias ? p.bias : hw;
    const int C = p.n_store;
    const bool has_bias = p.bias != nullptr;
    const float floor_v = (p.flags & GF_RELU) ? 0.f : -3.0e38f;
    float part[FJ][4];
#pragma unroll
    for (int fj = 0; fj < FJ; ++fj) part[fj][0] = part[fj][1] = part[fj][2] = part[fj][3] = 0.f;
    // 1x1 weights and bias of fragment column fi: requested one fragment ahead (double buffered); the fence keeps hipcc from hoisting
    // all 40 loads (160 registers next to the 128 accumulators) to the top
    float4 wb[2][5];
    auto request = [&](int fi, float4 (&d)[5]) __attribute__((always_inline)) {
        const int n = fi * 16 + i4;                     // n0 == 0: one tile spans the channels
        const int nc = min(n, C - 4);                   // channels >= C: zero accumulators (padded weight rows), zero 1x1 weights
        d[4] = *reinterpret_cast<const float4*>(bsrc + nc);
#pragma unroll
        for (int o = 0; o < 4; ++o) d[o] = *reinterpret_cast<const float4*>(hw + (size_t)o * C + nc);
    };
    request(0, wb[0]);
#pragma unroll
    for (int fi = 0; fi < FI; ++fi) {
        if (fi + 1 < FI) request(fi + 1, wb[(fi + 1) & 1]);
        const float live = fi * 16 + i4 < C ? 1.f : 0.f;
        const float4 bt = wb[fi & 1][4];
        const float4 bi = make_float4(has_bias ? bt.x : 0.f, has_bias ? bt.y : 0.f, has_bias ? bt.z : 0.f, has_bias ? bt.w : 0.f);
        float4 w4[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float4 t = wb[fi & 1][o];
            w4[o] = make_float4(t.x * live, t.y * live, t.z * live, t.w * live);
        }
#pragma unroll
        for (int fj = 0; fj < FJ; ++fj) {
            const f32x4_t a = acc[fi][fj];
            // ReLU as a select-free maximum (a branch here splits the block and the register allocator spills around it)
            const float v0 = fmaxf(a[0] + bi.x, floor_v), v1 = fmaxf(a[1] + bi.y, floor_v), v2 = fmaxf(a[2] + bi.z, floor_v), v3 = fmaxf(a[3] + bi.w, floor_v);
#pragma unroll
            for (int o = 0; o < 4; ++o)
                part[fj][o] = fmaf(v3, w4[o].w, fmaf(v2, w4[o].z, fmaf(v1, w4[o].y, fmaf(v0, w4[o].x, part[fj][o]))));
        }
        asm volatile("" ::: "memory");
    }
    // the four lane groups hold four quarters of a row's channels: add them up; lane group g then owns the rows of fragment g
    const int g = lane >> 4;
    float r4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int fj = 0; fj < FJ; ++fj)
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float t = rows_sum4(part[fj][o]);
            r4[o] = (fj == g) ? t : r4[o];
        }
    r[0] = r4[0] + hb[0]; r[1] = r4[1] + hb[1]; r[2] = r4[2] + hb[2]; r[3] = r4[3] + hb[3];
}

}  // namespace d3r
