// dust3r_amd -- the persistent split-fp16 GEMM (gemm_p4.hpp) for the q | k attention projections: bias / folded LayerNorm, 2-D RoPE and the head scatter
// [B][heads][ntok][64] in the drain (EPK_HEADS, EPK_HEADS_D). A translation unit of its own: the build keeps one resource report per file.
#include "gemm_p4.hpp"

namespace d3r {
namespace p4 {

// the attention-projection instances (EPK_HEADS, EPK_HEADS_D): mg_ntok, mg_tokw = floor(2^32 / d) + 1 of the divisors ntok and tok_w of the row -> (image, token) map
template <int EPK>
__global__ __launch_bounds__(NT, 1) void gemm_p4_heads_kernel(GemmParams p, int tiles_m, int tiles_n, int ntiles, uint32_t mg_ntok, uint32_t mg_tokw) {
    gemm_p4_body<EPK, 2, false>(p, tiles_m, tiles_n, ntiles, mg_ntok, mg_tokw);
}

}  // namespace p4

template <int EPK> static hipError_t launch_p4_heads(const GemmParams& p, hipStream_t s) {
    static std::atomic<unsigned long long> attr_done{0};
    raise_dynamic_lds_once(attr_done, reinterpret_cast<const void*>(p4::gemm_p4_heads_kernel<EPK>), p4::LDS);
    const int cus = device_cus();
    const int tiles_m = p.M / p4::BM, tiles_n = p.n_store / p4::BN, ntiles = tiles_m * tiles_n;
    int grid = cus < ntiles ? cus : ntiles;
    grid &= ~7;                          // as launch_p4 (gemm_p4.hip)
    if (grid < 8) return hipErrorInvalidValue;
    // (both divisors >= 2: gemm_p4_eligible)
    const uint32_t mg_ntok = (uint32_t)((1ull << 32) / (unsigned)p.ntok + 1), mg_tokw = (uint32_t)((1ull << 32) / (unsigned)p.tok_w + 1);
    hipLaunchKernelGGL((p4::gemm_p4_heads_kernel<EPK>), dim3(grid), dim3(p4::NT), p4::LDS, s, p, tiles_m, tiles_n, ntiles, mg_ntok, mg_tokw);
    return hipGetLastError();
}

hipError_t launch_gemm_p4_heads(const GemmParams& p, hipStream_t s) {
    if (!p.rope_table || !p.head_dst[0] || (p.n_store > p.head_c && !p.head_dst[1]) || (p.n_store > 2 * p.head_c && !p.head_dst[2])) return hipErrorInvalidValue;
    // the rotation in the compiled form of the gemm.hip epilogue the same launch would take: wide (ntok % 32 == 0, ldv % 8 == 0) or direct
    return (p.ntok & 31) == 0 && (p.ldv & 7) == 0 ? launch_p4_heads<p4::EPK_HEADS>(p, s) : launch_p4_heads<p4::EPK_HEADS_D>(p, s);
}

}  // namespace d3r
