// dust3r_amd -- the GEMM dispatch as ONE pure host function (included by kernels.hpp, below GemmParams): shape, operand type, epilogue, the four
// D3R_GEMM_* values and a CU count go in, the route of the launch comes out. launch_gemm (gemm.hip) runs the plan, the engine's profile (engine.hip) and
// the host queries of the C ABI (capi.hip) report the same plan: a new route is added HERE and nowhere else. No HIP call and no getenv in this file.
#pragma once

namespace d3r {

struct GemmEnv {             // read by gemm_env() (gemm.hip), once per launch or query
    int forced_cfg = -1;     // D3R_GEMM_CFG=0..9|11: the tile configuration pinned from the environment (parity tests, A/B runs); -1 = not set
    int persist = -1;        // D3R_GEMM_PERSIST: -1 the heuristic decides, 0 never, 1 every eligible launch on the persistent kernel
    long t128w8 = 1100;      // D3R_GEMM_T128W8: 128 x 128 launches of fewer tiles run on eight waves (0 = never)
    bool nowide = false;     // D3R_GEMM_NOWIDE=1
    long up2_min_tiles = -1; // D3R_UP2_MIN_TILES (tests): fewest pixel tiles of a fused x2 + convolution launch; -1 = one per compute unit
};
struct GemmPlan {
    int cfg = GEMM_CFG_128;  // GEMM_CFG_*, GEMM_CFG_P4 included, already mapped onto the shapes the operand type has: what profiles and host queries report
    bool w8 = false;         // cfg == GEMM_CFG_128 on EIGHT waves (include/dust3r_hip.h: D3R_TILE_128W8)
    int splitk = 1;          // blocks per tile along K (GemmParams::splitk of the launch)
    int flags = 0;           // what the launch ORs into p.flags
    bool up2 = false;        // an AMODE_CONV_UP2 launch runs fused (gemm_up2.hip); false: there is no such launch, the caller materialises the map
};

// x2 bilinear map + 3x3 convolution in one launch (AMODE_CONV_UP2, gemm_up2.hip): split-fp16, whole 16 x 32 tiles of output pixels, whole 32-channel K slices,
// one wave per 64 pixels holding all <= 128 output channels, the fused head tail or a typed store as the epilogue,
// and at least one tile per compute unit -- below that the 512-pixel tiles leave CUs idle that the two-kernel route's smaller tiles fill.
constexpr int UP2_TILE_H = 16, UP2_TILE_W = 32;
inline bool conv_up2_fused(const GemmParams& p, int dt, const GemmEnv& env, int cus) {
    if (dt != D3R_F16X3 || p.amode != AMODE_CONV_UP2) return false;
    // epilogues: the fused head tail, or a typed store (bias, ReLU) of whole 8-channel groups without residuals or a ReLU copy
    if (p.epi == EPI_T) { if (p.res1 || p.res2 || p.out2 || p.ldo % 8 != 0 || p.n_store % 8 != 0 || p.ldo < p.n_store || (p.flags & ~(GF_RELU | GF_NTSTORE | GF_NOWIDE))) return false; }
    else if (p.epi != EPI_HEAD4) return false;
    if (p.ksize != 3 || p.stride != 1 || p.pad != 1 || p.Hout != p.Hin || p.Wout != p.Win || (p.Hin & 1) || (p.Win & 1)) return false;
    if (p.Hin % UP2_TILE_H != 0 || p.Win % UP2_TILE_W != 0 || p.Cin <= 0 || p.Cin % 32 != 0 || p.cstride % 8 != 0 || p.cstride < p.Cin) return false;
    if (p.n_store > 128 || p.n_store % 4 != 0 || p.n_pad < 128 || p.K != 9 * p.Cin) return false;
    const long tiles = (long)(p.M / (p.Hin * p.Win)) * (p.Hin / UP2_TILE_H) * (p.Win / UP2_TILE_W);
    return tiles >= (env.up2_min_tiles >= 0 ? env.up2_min_tiles : (long)cus);
}

// tracing: a trace buffer (gemm_set_trace) is attached to this launch
inline GemmPlan gemm_plan(const GemmParams& p, int dt, const GemmEnv& env, int cus, bool tracing) {
    GemmPlan plan;
    // ---- flags. GF_NOWIDE under D3R_GEMM_NOWIDE=1: it changes the V^T route of the 16-bit attention projections, hence the tiles a heads launch may take
    // (the folded-LayerNorm producer launches keep their wide epilogue: it is where the row sums and the typed residual stream are written)
    if (env.nowide && !p.ln_part && !(p.flags & GF_X3RES)) plan.flags |= GF_NOWIDE;
    plan.flags |= GF_NTSTORE;      // wide epilogues store with the non-temporal policy (measured +3..10 % on isolated GEMMs, +1 % on the forward)
    const bool nowide = (p.flags | plan.flags) & GF_NOWIDE;
    tracing = tracing || p.trace;
    if (p.amode == AMODE_CONV_UP2) {      // one shape, or no launch at all
        plan.cfg = GEMM_CFG_512x128;
        plan.up2 = !tracing && p.force_cfg < 0 && env.forced_cfg < 0 && conv_up2_fused(p, dt, env, cus);
        return plan;
    }

    // ---- persistent kernel (gemm_p4.hip) for this launch? Measured on MI355X inside the 32-pair forward (tools/launch_table.py, profiles/r06_*): it wins where the
    // epilogue is a large share of a tile's life and the tiles fill whole rounds of the CUs -- fc1 + GELU 395 -> 427 (encoder) / 363 -> 398 TFLOP/s (decoder),
    // the typed-residual projections at K <= 1024 348 -> 362, typed stores +4..12 % -- ties at K = 4096 (fc2: the K loop dominates; the one-tile-per-block
    // kernels keep it) and loses where its 256 x 128 tiles leave the last round of CUs mostly empty (the decoder's N = 768 GEMMs: 576 tiles = 2.25 rounds).
    // A trace buffer, direct stores (GF_NOWIDE), force_cfg or D3R_GEMM_CFG keep a launch off it.
    if (dt == D3R_F16X3 && !tracing && !nowide && p.force_cfg < 0 && env.forced_cfg < 0 && env.persist != 0 && gemm_p4_eligible(p, dt)) {
        const long tiles = (long)(p.M / 256) * (p.n_store / 128);
        const long rounds = (tiles + cus - 1) / cus;
        // the last round at least ~half full on average: >= 88 % of the tile slots used
        // Attention projections (EPI_HEADS; eligible: rotated regions only): the q | k launch the engine splits off a q | k | v projection (engine.hip gemm_heads), and only
        // where it fills its rounds almost exactly (>= 95 % of the slots: the encoder's 49152 x 2048 = 3072 tiles = 12 rounds). The split costs the V launch the rounds it
        // shared with q | k: the decoder's V alone (N = 768) fills rounds on no kernel, its q | k 90 % -- not split, not measured. One-region launches (the
        // cross-attention q) stay on the one-tile-per-block kernels as recorded (tests/golden/gemm_plan_table.json).
        const bool heads_ok = p.epi != EPI_HEADS || (p.n_store == 2 * p.head_c && tiles * 100 >= rounds * cus * 95);
        if (env.persist == 1 || (tiles >= cus && tiles * 100 >= rounds * cus * 88 && !(p.epi == EPI_F32 && p.K > 1024) && heads_ok)) {
            plan.cfg = GEMM_CFG_P4;
            return plan;
        }
    }

    // ---- one tile per block. Tile configuration choice, from measurements on MI355X (tools/gpu_probe.py gemm, profiles/): the 256x256 tile wins
    // once there are at least ~3 full rounds of 256 resident blocks (M = 49152: 760-1070 vs 640-830 TF/s), the 128x128 tile
    // (2 blocks per CU: one block's prologue / epilogue hides behind the other's K loop) wins below that; N <= 128 problems
    // (DPT head convolutions) take the 512x128 / 256x128 tiles so that no half-empty 256-wide tile is computed.
    const int n_rows = p.n_rows > 0 ? p.n_rows : p.n_pad;
    const bool wide_vt = (dt == D3R_BF16 || dt == D3R_F16) && (p.ntok & 63) == 0 && !nowide;
    const bool heads = p.epi == EPI_HEADS && !wide_vt;   // "heads" = needs a square tile (operand-role swap for V^T)
    const bool ok256 = cdiv(p.n_store, 256) * 256 <= n_rows && (p.epi != EPI_HEADS || p.head_c % 256 == 0);
    // the launches the split-fp16-only shapes are written for: no attention heads (their V^T regions need a square tile), no fused head tail; `lin`: nn.Linear operands
    const bool x3_plain = dt == D3R_F16X3 && p.epi != EPI_HEADS && p.epi != EPI_HEAD4;
    const bool x3_lin = x3_plain && p.amode == AMODE_LINEAR;
    const long tiles128 = (long)cdiv(p.M, 128) * cdiv(p.n_store, 128);
    const auto raw = [&]() -> int {
        // force_cfg, else D3R_GEMM_CFG, pins the tile configuration (parity tests, A/B runs); infeasible choices are ignored
        int forced = p.force_cfg >= 0 ? p.force_cfg : env.forced_cfg;
        // retired shapes: 4 (four-wave 256 x 128) runs on the eight-wave 256 x 128 tile, 5 / 6 (four-stage, ping-pong 256 x 256) on the two-stage one
        if (forced == GEMM_CFG_256x128W4) forced = GEMM_CFG_256x128;
        if (forced == GEMM_CFG_256S4 || forced == GEMM_CFG_256PP) forced = GEMM_CFG_256;
        if (forced == GEMM_CFG_384x192 && x3_lin && cdiv(p.n_store, 192) * 192 <= n_rows) return forced;
        if (forced == GEMM_CFG_96x64 && x3_plain) return forced;
        if (forced == GEMM_CFG_128 || forced == GEMM_CFG_64 || (forced == GEMM_CFG_256 && ok256) ||
            ((forced == GEMM_CFG_256x128 || forced == GEMM_CFG_512x128 || forced == GEMM_CFG_256x128R) && !heads))
            return forced;
        if (!heads && p.n_store <= 128) {
            if (cdiv(p.M, 512) >= 512) return GEMM_CFG_512x128;
            if (cdiv(p.M, 256) >= 512) return GEMM_CFG_256x128;
            return GEMM_CFG_128;
        }
        // split-fp16, nn.Linear launches without attention heads whose (M / 384) x (N / 192) tiles fill whole rounds of the 256 CUs: the decoder's 24576-row
        // GEMMs at 32 pairs per step (N = 768 / 3072 -> 256 / 1024 tiles; on the 128 x 128 tile 1152 tiles = 2.25 rounds of the 512 slots). Measured
        // (profiles/r04_i, r04_k). In isolation, us per launch, default tile -> this one: fc2 24576 x 768 x 3072 + residual 389 -> 280, fc1 24576 x 3072 x 768
        // + GELU 384 -> 364, plain stores 108 -> 88 / 222 -> 161 / 286 -> 224 (N = 768 / 1536 / 2304), the fp32-residual projections at K = 768 90 -> 94.
        // On the forward the isolated gains mostly vanish (in the network the default tiles run faster than back to back on one shape, and the two decoder
        // sides overlap their tails on the two streams): every eligible launch on it 194.55 -> 196.75 and 191.7 -> 192.7 pairs/s (two boxes, every run above every
        // baseline run); WITHOUT the K <= 1024 projections 191.7 -> 190.9 -- so the rule is "every eligible launch".
        if (x3_lin && p.n_store % 192 == 0 && cdiv(p.n_store, 192) * 192 <= n_rows) {
            const long t384 = (long)cdiv(p.M, 384) * cdiv(p.n_store, 192);
            // whole rounds of THIS device's compute units (256 on MI355X; a partitioned device has fewer)
            if (t384 >= cus * 9 / 10 && (t384 % cus == 0 || t384 % cus >= cus * 9 / 10)) return GEMM_CFG_384x192;
        }
        // split-fp16, launches without attention heads (their V^T regions need a square tile): the two-blocks-per-CU 256 x 128 shape with the
        // weights of a K step in registers. Measured on MI355X (profiles/r03_c/gemmtrace_cfg7.log, bench_r*.log): it wins where the epilogue
        // is an HBM burst that the other block's MFMAs can run under -- the fp32-residual projections at K <= 1024 (proj 49152 x 1024 x
        // 1024: 337 vs 296 TFLOP/s) -- and loses 1-6 % where the epilogue is VALU work (GELU, typed stores: on gfx950 VALU and MFMA of a
        // SIMD overlap only by half, tools/issue_probe.hip) or the K loop dominates (fc2): default = those projections only.
        if (x3_lin && p.n_store > 128 && p.epi == EPI_F32 && p.res1 != nullptr && p.K <= 1024 && (long)cdiv(p.M, 256) * cdiv(p.n_store, 128) >= 1024)
            return GEMM_CFG_256x128R;
        // split-fp16, small problems (the one- and two-pair forwards of dust3r/demo.py:156 / visloc.py:88, batch_size = 1): below ~1.5
        // 128 x 128 tiles per CU the chip is not full -- the 64 x 64 tile by four waves of 32 x 32 runs the same problem on four times the
        // waves. The crossover, 200 tiles of 128 x 128, was measured against 400 / 600 / 1000 / 2000 for 1-8 pairs per call: the best or within
        // noise of it everywhere (profiles/r03_f/latency_small_tiles.log).
        if (dt == D3R_F16X3 && p.n_store > 128 && tiles128 < 200) {
            // round 6: M 96 x N 64 instead, where its tiles come to 1.5 ... 2 per CU. The small tiles run at the rate their operand rows arrive: the 96 x 64
            // shape moves 17 % fewer bytes per flop, but a CU needs two or three resident blocks' worth of loads in flight to keep that rate -- measured on MI355X
            // (tools/tile_probe.py, profiles/r06_f; 64 x 64 -> 96 x 64, us per launch): 3072 x 1024 x 4096 81 -> 71, 2304 x 1024 x 4096 75 -> 61, 3072 x 768 x 3072 66 -> 53,
            // 1536 x 1536 x 768 20 -> 18, 768 x 3072 x 768 20 -> 18 (384 or 512 tiles); 1536 x 1024 x 4096 56 -> 61 (256 tiles: one block per CU), 1152 x 768 x 3072 33 -> 40 (144),
            // 1536 x 2304 x 768 28 -> 30 (576). nn.Linear operands without attention heads only. INSIDE the forward (same process, rule on | off) the
            // K = 768 / 1024 cases do not carry over -- one pair 10.04 vs 9.96 ms (the decoder's two sides run side by side: twice the tiles in flight), two pairs 14.49 vs
            // 14.68 -- so the rule keeps the long K loops only (K >= 2048: fc2 of the encoder at two / three pairs, of the decoder at four).
            const long t96 = (long)cdiv(p.M, 96) * cdiv(p.n_store, 64);
            if (x3_lin && p.K >= 2048 && t96 * 2 >= (long)cus * 3 && t96 <= (long)cus * 2) return GEMM_CFG_96x64;
            return GEMM_CFG_64;
        }
        // fp16 + fp8 rows: the 256-wide tile is 1.3-1.6x ahead of the 128 x 128 one per tile (its K loop lost a third of its MFMA work, the small
        // tile's LDS read traffic per MFMA is twice as high), so it pays from a single round of resident blocks on: measured +1.5 % on the
        // forward with the decoder's 24576 x 768 GEMMs (288 tiles, two such launches side by side on the two streams) on it
        const long t256 = (dt == D3R_F16F8 || dt == D3R_F16X2F8) ? 250 : 700;
        if (ok256 && (long)cdiv(p.M, 256) * cdiv(p.n_store, 256) >= t256) return GEMM_CFG_256;
        return GEMM_CFG_128;
    };
    int cfg = raw();
    // ---- operand types that lack a shape: 7 / 8 / 9 / 11 exist in split-fp16 only, the 2.5-unit K loop on the two square tiles
    if ((cfg == GEMM_CFG_256x128R || cfg == GEMM_CFG_64 || cfg == GEMM_CFG_96x64 || cfg == GEMM_CFG_384x192) && dt != D3R_F16X3) cfg = cfg == GEMM_CFG_256x128R ? GEMM_CFG_256x128 : GEMM_CFG_128;
    if (dt == D3R_F16X2F8 && cfg != GEMM_CFG_256) cfg = GEMM_CFG_128;
    plan.cfg = cfg;
    // ---- 128 x 128 launches of fewer than 1100 tiles (the one- to four-pair forwards) on the eight-wave shape. Measured (profiles/r03_k):
    // one pair 10.59 -> 10.26 ms, two 16.0 -> 15.3, four 26.3 -> 25.9; applied to the 1152-tile launches of the 32-pair step as well:
    // -0.1 %, hence the limit. D3R_GEMM_T128W8 moves it (0 = never).
    plan.w8 = cfg == GEMM_CFG_128 && dt == D3R_F16X3 && tiles128 < env.t128w8;
    // ---- split-K (kernels.hpp): only with the caller's buffers, split-fp16 nn.Linear launches of the small-batch forwards (the problems the heuristic sends to the
    // 64 x 64 tile: fewer than 200 tiles of 128 x 128), the plain K loop; at most 3 blocks per CU after the split, at least 16 K steps (of 32) per slice.
    if (cfg == GEMM_CFG_64 && p.sk_slab && p.sk_cnt && p.splitk != 1 && p.amode == AMODE_LINEAR && !tracing && p.force_cfg < 0) {
        constexpr int tile = 64, minsteps = 16;
        const long maxblocks = (long)cus * 3;
        const long tiles = (long)cdiv(p.M, tile) * cdiv(p.n_store, tile);
        const int nk32 = p.K / 32;
        for (int c : {8, 6, 4, 3, 2}) {
            if (tiles * c <= maxblocks && nk32 % c == 0 && nk32 / c >= minsteps && (size_t)tiles * c * tile * tile <= p.sk_slab_floats && tiles <= p.sk_cnt_n) { plan.splitk = c; break; }
        }
    }
    return plan;
}

}  // namespace d3r
