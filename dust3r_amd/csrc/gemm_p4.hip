// dust3r_amd -- persistent split-fp16 GEMM whose epilogue runs UNDER the next tile's K loop (gfx950; round 6).
//
// What it is for (reference call sites): the nn.Linear layers of the 24 encoder / 2 x 12 decoder blocks at batch sizes whose GEMMs fill the
// chip (dust3r/model.py:136-137,180-186 -> croco Block / DecoderBlock: proj, fc1, fc2). In gemm.hip one block computes one tile and then
// stores it: for K <= 1024 a tile spends 15-25 % of its life in the epilogue with the CU's matrix pipes idle (tools/tile_probe.py: the same
// launches without their epilogue run 505-514 TFLOP/s against 371-438 with it).
//
// Shape. One block per CU, FOUR waves, one per SIMD, each with the whole 512-entry register file: 256 accumulator registers = TWO sets of
// the 128 (n) x 64 (m) wave tile (8 x 4 fragments of v_mfma_f32_16x16x32_f16, the wave tile of gemm.hip's 256 x 256 shape, so the LDS read
// traffic per MFMA is the same). Block tile M 256 x N 128. A block walks its tiles (the XCD-contiguous panel order of gemm.hip, strided by
// the grid); set C accumulates tile t while set D -- tile t - 1 -- is drained ONE FRAGMENT PER K STEP (two when the tile has fewer than 32
// steps), a few instructions behind each group of four MFMAs: accumulator -> bias / folded LayerNorm / GELU / residual -> split -> the lanes
// that hold the two halves of an 8-element group swap them (v_permlane16_swap) -> one 16-byte global store per lane. No LDS staging.
// Operands arrive by global_load_lds DMA into a THREE-slot ring that never drains between tiles (the loads run two K steps ahead of the
// math, across tile boundaries); one s_barrier per K step, in the MIDDLE of the step's MFMA stream (the slot it publishes is the NEXT
// step's, the slot it frees is filled behind it), the 12 DMA pieces of a step and the head fragments of the next are spread between the
// MFMA rows. Every VMEM operation of the kernel is issued from inline asm and counted by hand (hipcc's own counter cannot see the DMA: any
// load it knows about would wait for everything in flight): vmcnt(n) below always names how many YOUNGER operations may stay outstanding.
//
// Arithmetic: per output element the same MFMA sequence as every gemm.hip tile (per 32 k: lo.hi, hi.lo, hi.hi; K ascending) and the same
// epilogue expressions and summation trees, so results are bit-identical to them (tests/test_kernels_gpu.py::test_persistent_gemm_*).
#include "gemm_p4.hpp"

namespace d3r {
namespace p4 {

template <int EPK, int NF, bool L32>
__global__ __launch_bounds__(NT, 1) void gemm_p4_kernel(GemmParams p, int tiles_m, int tiles_n, int ntiles) {
    gemm_p4_body<EPK, NF, L32>(p, tiles_m, tiles_n, ntiles, 0u, 0u);
}

}  // namespace p4

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------
// Which launches can run here: split-fp16 nn.Linear operands, whole 256 x 128 tiles, at least 18 K steps, one of the epilogues above.
bool gemm_p4_eligible(const GemmParams& p, int dt) {
    if (dt != D3R_F16X3 || p.amode != AMODE_LINEAR) return false;
    if (p.M % p4::BM != 0 || p.n_store % p4::BN != 0 || p.K % 32 != 0 || (p.K >> 5) < 18) return false;
    if (p.n_store > p.n_pad || p.ln_part_in || p.trace || (p.flags & (GF_RELU | GF_NOWIDE))) return false;
    if ((size_t)256 * p.lda * 4 >= (1ull << 31) || (size_t)128 * p.K * 4 >= (1ull << 31)) return false;       // 32-bit row offsets inside a tile
    if (p.epi == EPI_F32) {
        if (!(p.flags & GF_X3RES) || !p.out2 || (p.ldo2 & 7) || (p.res1 && (p.ldr & 7)) || p.res2 || (p.ln_part && p.n_store % 32 != 0)) return false;
        if ((size_t)16 * p.ldo2 * 4 >= (1ull << 31) || (p.res1 && (size_t)16 * p.ldr * 4 >= (1ull << 31))) return false;
        return true;
    }
    if (p.epi == EPI_GELU || p.epi == EPI_T) {
        if (p.res1 || p.res2 || p.out2 || (p.ldo & 7) || !p.out) return false;
        if (p.ln_rstd && (!p.ln_nmr || !p.ln_colsum)) return false;
        if ((size_t)16 * p.ldo * 4 >= (1ull << 31)) return false;
        return true;
    }
    if (p.epi == EPI_HEADS) {
        // q | k projections: every region rotated (HEAD_ROPE) -- V^T needs the operand roles swapped, HEAD_PLAIN is declined; whole heads pairs per tile; 16-row fragments
        // inside one image; a token grid whose table rows fit the kernel's LDS copy; row / token quotients exact by multiplication (x d < 2^32)
        const int regions = p.head_c > 0 ? p.n_store / p.head_c : 0;
        // the grid is a multiple of 8 blocks (one range of tiles per XCD): fewer tiles would be no launch, so the forced mode (D3R_GEMM_PERSIST=1) hands them back
        if ((long)(p.M / p4::BM) * (p.n_store / p4::BN) < 8) return false;
        if (p.res1 || p.res2 || p.out2 || p.head_c % 128 != 0 || regions < 1 || regions > 3 || regions * p.head_c != p.n_store) return false;
        for (int r = 0; r < regions; ++r) if (p.head_kind[r] != HEAD_ROPE) return false;
        if (p.ln_rstd && (!p.ln_nmr || !p.ln_colsum)) return false;
        if (p.ntok <= 0 || p.ntok % 16 != 0 || p.M % p.ntok != 0 || p.tok_w < 2 || p.ntok % p.tok_w != 0 || p.heads * 64 != p.head_c) return false;
        if (p.tok_w > p4::ROPE_POS || p.ntok / p.tok_w > p4::ROPE_POS || (unsigned long long)p.M * p.ntok >= (1ull << 32)) return false;
        return true;
    }
    return false;
}

template <int EPK, int NF, bool L32 = false> static hipError_t launch_p4(const GemmParams& p, hipStream_t s) {
    static std::atomic<unsigned long long> attr_done{0};
    raise_dynamic_lds_once(attr_done, reinterpret_cast<const void*>(p4::gemm_p4_kernel<EPK, NF, L32>), p4::LDS);
    const int cus = device_cus();
    const int tiles_m = p.M / p4::BM, tiles_n = p.n_store / p4::BN, ntiles = tiles_m * tiles_n;
    int grid = cus < ntiles ? cus : ntiles;
    grid &= ~7;                          // XCD-contiguous tile ranges need the grid stride to keep a block on its XCD (v & 7 == blockIdx & 7)
    if (grid < 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL((p4::gemm_p4_kernel<EPK, NF, L32>), dim3(grid), dim3(p4::NT), p4::LDS, s, p, tiles_m, tiles_n, ntiles);
    return hipGetLastError();
}

hipError_t launch_gemm_p4(const GemmParams& p, hipStream_t s) {
    // Two fragments per K step (16 draining steps) everywhere. The one-fragment form (NF = 1: 32 unrolled step bodies) measured SLOWER on MI355X
    // (typed store 408 vs 436 TFLOP/s, GELU 338 vs ~400 at K = 1024): ~100 KB of straight-line code per tile against a 64 KB instruction cache.
    // It stays in the template but is not instantiated.
    if (p.epi == EPI_F32) return p.ln_part ? launch_p4<p4::EPK_X3RES_LN, 2>(p, s) : launch_p4<p4::EPK_X3RES, 2>(p, s);
    if (p.epi == EPI_GELU) return launch_p4<p4::EPK_GELU, 2>(p, s);
    if (p.epi == EPI_HEADS) return launch_gemm_p4_heads(p, s);      // gemm_p4_heads.hip
    return launch_p4<p4::EPK_TYPED, 2>(p, s);
}

}  // namespace d3r
