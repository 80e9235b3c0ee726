// dust3r_amd -- internal kernel launch interface (C++ side, below the C-ABI of include/dust3r_hip.h).
#pragma once
#include "common.hpp"

namespace d3r {

// ------------------------------------------------------------------------------ GEMM / conv
// AMODE_CONV_UP2 (split-fp16): Conv2d(3x3, stride 1, pad 1) whose input is the x2 bilinear map (align_corners = True, no crop) of `act`, a low-resolution NHWC map of
// Hin / 2 x Win / 2 pixels -- Hin, Win, Hout, Wout and M describe the convolution on the map, which is never materialised (gemm_up2.hip; conv_up2_fused below decides)
enum { AMODE_LINEAR = 0, AMODE_CONV = 1, AMODE_CONV_UP2 = 2 };
enum { EPI_T = 0, EPI_F32 = 1, EPI_GELU = 2, EPI_HEADS = 3, EPI_CONVT = 4, EPI_HEAD4 = 5 };
// EPI_HEAD4 (split-fp16, tiles whose waves hold all <= 128 output channels of their rows: the 512 x 128 / 256 x 128 R shapes): the DPT head's
// tail fused into its last 3x3 convolution -- bias, ReLU (GF_RELU), Conv2d(C, 4, 1) on the fp32 accumulators, postprocess, store of
// pts / conf (dpt_head.py:63 + postprocess.py:10-58). Field reuse: out = pts (float*), ldo = its pixel stride, out2 = conf (float*),
// ldo2 = its pixel stride, res1 = the 1x1 weights [4][n_store] fp32, res2 = its bias [4] fp32. Nothing of the C-channel map is stored.
enum { HEAD_ROPE = 1, HEAD_VT = 2, HEAD_PLAIN = 3 };
enum { GF_RELU = 1, GF_NOWIDE = 4, GF_NTSTORE = 8, GF_X3RES = 16 };   // GF_X3RES (EPI_F32, split-fp16): res1 and the result live in split-fp16 rows only (out2); no fp32 row is stored   // GF_NTSTORE: wide epilogues store with the non-temporal policy (set by every plan, gemm_plan.hpp)
// tile map of both GEMM kernels: block ids walk column panels GEMM_PANEL tiles wide, row by row
constexpr int GEMM_PANEL = 8;
// 4 / 5 / 6 name retired shapes; pinned (D3R_GEMM_CFG, force_cfg) they run configurations 2 / 1 / 1
enum { GEMM_CFG_128 = 0, GEMM_CFG_256 = 1, GEMM_CFG_256x128 = 2, GEMM_CFG_512x128 = 3, GEMM_CFG_256x128W4 = 4, GEMM_CFG_256S4 = 5, GEMM_CFG_256PP = 6, GEMM_CFG_256x128R = 7, GEMM_CFG_64 = 8, GEMM_CFG_384x192 = 9, GEMM_CFG_P4 = 10, GEMM_CFG_96x64 = 11 };

struct GemmParams {
    const void* act = nullptr;   // [M][lda] (linear) or NHWC image batch (conv), element type DT
    const void* wgt = nullptr;   // [n_pad][K], element type DT, rows >= N zero filled
    const float* bias = nullptr; // [n_pad] or null
    int M = 0, K = 0, n_pad = 0; // K in elements, multiple of 128/sizeof(DT); n_pad: multiple of 128, >= n_store
    int n_rows = 0;              // weight rows actually allocated (>= n_pad; 0 = n_pad): bounds the tile width choice
    int force_cfg = -1;          // GEMM_CFG_* to override the heuristic (tests / probes)
    int n_store = 0;             // columns written (multiple of 4, <= n_pad)
    int lda = 0;
    int amode = AMODE_LINEAR;
    // implicit-GEMM conv geometry (NHWC, K index = (ky, kx, cin))
    int Hin = 0, Win = 0, Cin = 0, cstride = 0, Hout = 0, Wout = 0, ksize = 1, stride = 1, pad = 0;
    const void* zero_page = nullptr;
    // epilogue
    int epi = EPI_T;
    int flags = 0;
    void* out = nullptr; int ldo = 0;
    const void* res1 = nullptr; const void* res2 = nullptr; int ldr = 0;
    void* out2 = nullptr; int ldo2 = 0;
    int ct_cout = 0;             // EPI_CONVT: (padded) output channels per tap
    // EPI_HEADS: column n belongs to region n / head_c; head (n % head_c) / 64
    int head_c = 1 << 30;
    int head_kind[3] = {0, 0, 0};
    void* head_dst[3] = {nullptr, nullptr, nullptr};
    int heads = 0, ntok = 1, tok_w = 1, ldv = 0;
    const float* rope_table = nullptr;  // [max_pos][16] (cos, sin) pairs
    // diagnostics (d3r_gemm_set_trace): 8 x uint64 per block -- wall-clock ticks at entry / K-loop start / K-loop end / epilogue
    // issued / stores drained, then HW_ID, XCC_ID, blockIdx
    unsigned long long* trace = nullptr;
    PostMode post;               // EPI_HEAD4: depth_mode / conf_mode of the head's postprocess
    // ---- LayerNorm folded into the GEMMs on both sides of it (round 5, split-fp16 engine; engine.hip `ln_fold`) ----------------------------
    // LN(x) W^T + b = rstd (x (W diag(gamma))^T - mean s) + b',  s_n = sum_k gamma_k W_nk,  b' = b + W beta.
    // PRODUCER (an EPI_F32 launch, wide epilogue): next to the fp32 rows it stores (and their typed copy out2 = the RAW x the consumer GEMM
    //   reads as its activation operand) it writes ln_part[m][n / 32] = (sum, sum of squares) of the 32 stored values of row m in that column
    //   group, summed in ONE fixed tree whatever the tile shape (quad sums, then xor 1 / 2 / 4 over the 8 quads) -- so the statistics, like every
    //   output, do not depend on the tile configuration. n_store % 32 == 0.
    // CONSUMER (weights = W diag(gamma) packed at load time, bias = b'): every epilogue forms rstd_m (acc - mean_m s_n) + b'_n as
    //   fma(acc, ln_rstd[m], fma(ln_colsum[n], ln_nmr[m], bias[n])) with ln_nmr = -mean rstd; with ln_rstd == nullptr the same expression
    //   runs on (1, 0, 0): fma(acc, 1, fma(0, 0, b)) = acc + b bit for bit.
    float* ln_part = nullptr;
    const float* ln_rstd = nullptr; const float* ln_nmr = nullptr; const float* ln_colsum = nullptr;
    // CONSUMER of a small problem: the partial sums [M][K / 32][2] of its input rows; the kernel's prologue then forms ln_rstd / ln_nmr of its tile's rows itself (and WRITES
    // them to those two arrays) with the arithmetic of ln_finalize_kernel, which is not launched
    const float* ln_part_in = nullptr; float ln_eps = 1e-6f, ln_inv_c = 0.f;
    // ---- split-K for SMALL problems (round 6; split-fp16, nn.Linear operands, the plain K loop): `splitk` blocks share a tile, each over 1 / splitk of the K steps;
    // every block stores its fp32 partial tile in sk_slab ([tile][slice][wave][fragment][lane] float4), the block that draws the last ticket of sk_cnt[tile] adds the
    // slices up in slice order (deterministic whichever block is last) and runs the epilogue. Chosen by gemm_plan when the caller lends the launch the two buffers.
    int splitk = 1; float* sk_slab = nullptr; unsigned* sk_cnt = nullptr; size_t sk_slab_floats = 0; int sk_cnt_n = 0;
};
void gemm_set_trace(unsigned long long* buf, size_t capacity_blocks);

// gemm_p4.hip: the persistent split-fp16 kernel whose epilogue runs under the next tile's K loop (tile configuration 10 in profiles)
bool gemm_p4_eligible(const GemmParams& p, int dt);
hipError_t launch_gemm_p4(const GemmParams& p, hipStream_t s);
hipError_t launch_gemm_p4_heads(const GemmParams& p, hipStream_t s);      // gemm_p4_heads.hip: its EPI_HEADS launches (every region HEAD_ROPE)
// gemm_up2.hip: AMODE_CONV_UP2 launches on 16 x 32 pixel tiles (eight waves of 128 (n) x 64 (m), profiled as tile configuration 3)
hipError_t launch_conv_up2(const GemmParams& p, hipStream_t s);
}  // namespace d3r
#include "gemm_plan.hpp"      // GemmEnv, GemmPlan, gemm_plan(): the dispatch decision, pure
namespace d3r {
GemmEnv gemm_env();                                      // the four D3R_GEMM_* values, read on every call (probes and tests move them inside one process)
GemmPlan gemm_plan_for(const GemmParams& p, int dt);     // gemm_plan under gemm_env(), the current device's CU count and the trace switch: what launch_gemm(dt, p, s) runs
hipError_t launch_gemm(int dt, const GemmParams& p, hipStream_t s);
// the same launch on a plan the caller already took from gemm_plan_for (the engine marks its profile with plan.cfg, then launches)
hipError_t launch_gemm(int dt, const GemmParams& p, const GemmPlan& plan, hipStream_t s);

// The weight rows of an N-column GEMM as the loader allocates them: N rounded up to the 128-column tile is computed, rows up to a 256-wide tile exist and stay zero
inline int gemm_n_pad(int N) { return rup(N, 128); }
inline int gemm_n_rows(int N) { return rup(N, 256); }
// the operand types of the GEMM entries, of the implicit-GEMM convolution entries, and the channel rows a convolution reads: whole K steps per tap, inside a pixel's row
inline bool gemm_dtype(int dt) { return dt == D3R_BF16 || dt == D3R_F16 || dt == D3R_F32 || dt == D3R_F16X3 || dt == D3R_F16F8 || dt == D3R_F16X2F8; }
inline bool conv_dtype(int dt) { return dt == D3R_BF16 || dt == D3R_F16 || dt == D3R_F32 || dt == D3R_F16X3; }
inline bool conv_operand_ok(int dt, int cin_pad, int cstride) { return conv_dtype(dt) && cin_pad > 0 && cin_pad % (128 / (int)dt_bytes(dt)) == 0 && cstride >= cin_pad; }
// depth_mode / conf_mode of the heads' postprocess as d3r_model_set_postprocess and the kernel entries accept them
inline bool post_mode(PostMode& pm, int depth_mode, int conf_mode, float vmin, float vmax) {
    if (depth_mode < POST_DEPTH_EXP || depth_mode > POST_DEPTH_SQUARE || conf_mode < POST_CONF_EXP || conf_mode > POST_CONF_SIGMOID) return false;
    if (!(vmin < vmax) || (conf_mode == POST_CONF_SIGMOID && !(vmax < __builtin_huge_valf() && vmin > -__builtin_huge_valf()))) return false;
    pm.depth = depth_mode; pm.conf = conf_mode; pm.cmin = vmin; pm.cmax = vmax;
    return true;
}

// nn.Linear-shaped operands [M][lda] x [N][K]^T: weight rows as the loader allocates them (engine.hip Lin). The caller adds the epilogue (the epi_* builders below).
inline GemmParams linear_gemm_params(const void* act, int lda, const void* wgt, const float* bias, int M, int N, int K) {
    GemmParams p;
    p.act = act; p.lda = lda; p.wgt = wgt; p.bias = bias; p.M = M; p.K = K;
    p.n_pad = gemm_n_pad(N); p.n_rows = gemm_n_rows(N); p.n_store = N;
    return p;
}

// The implicit-GEMM launches of the DPT head, built in ONE place for the engine (engine.hip conv / conv_head4) and for the kernel-level C ABI
// (capi.hip d3r_conv2d_nhwc_x / d3r_conv_head4): what the kernel tests pin is what the engine launches.
// conv_gemm_params: operand, geometry and weight-row fields of Conv2d(k, stride, pad) on NHWC rows of `cstride` elements per pixel whose first cin_pad
// channels are read; weight rows as the loader allocates them (round_up(Cout, 256) rows of k k cin_pad). The caller adds the epilogue.
inline GemmParams conv_gemm_params(const void* in, int B, int Hin, int Win, int cstride, const void* wgt, const float* bias, int cin_pad, int Cout, int k,
                                   int stride, int pad, const void* zero_page) {
    GemmParams p;
    p.amode = AMODE_CONV; p.act = in; p.wgt = wgt; p.bias = bias;
    p.Hin = Hin; p.Win = Win; p.Cin = cin_pad; p.cstride = cstride; p.ksize = k; p.stride = stride; p.pad = pad;
    p.Hout = (Hin + 2 * pad - k) / stride + 1; p.Wout = (Win + 2 * pad - k) / stride + 1;
    p.M = B * p.Hout * p.Wout; p.K = k * k * cin_pad; p.n_pad = gemm_n_pad(Cout); p.n_rows = gemm_n_rows(Cout); p.n_store = Cout;
    p.zero_page = zero_page;
    return p;
}
// The same 3x3 convolution (stride 1, pad 1) reading the x2 bilinear map of the low-resolution map `src` (B, Hi, Wi) without materialising it: AMODE_CONV_UP2.
// Whether such a launch exists is the plan's answer (GemmPlan::up2, gemm_plan.hpp conv_up2_fused); where it does not, the caller runs launch_upsample2x and
// conv_gemm_params on the map.
inline GemmParams conv_up2_gemm_params(const void* src, int B, int Hi, int Wi, int cstride, const void* wgt, const float* bias, int cin_pad, int Cout, const void* zero_page) {
    GemmParams p = conv_gemm_params(src, B, 2 * Hi, 2 * Wi, cstride, wgt, bias, cin_pad, Cout, 3, 1, 1, zero_page);
    p.amode = AMODE_CONV_UP2;
    return p;
}
// head4_tile: the plan of an EPI_HEAD4 launch -- 512 x 128 where the heuristic picks it, else the FORCED 256 x 128 R (p.force_cfg is set) -- or false when
// the launch cannot hold every output channel of a row in one wave (more than 128 channels, another precision mode): the caller takes the two-kernel route.
// Fewer pixels (one or two images) take the same tile by four waves stacked along m. ANY pixel count below the 512 x 128 tile's takes this shape (round 5): with the
// heuristic's 128 x 128 choice for < 512 tiles the head of ONE 512 x 160 pair took the two-kernel route and a batch of three the fused one -- 3e-6 apart, the only place where
// a batch was not bit-equal to its one-pair calls (tests/test_timed_configs_gpu.py::test_full_size_released_resolutions_match_oracle)
inline bool head4_tile(GemmParams& p, int dt, GemmPlan& plan) {
    if (p.ksize != 3 || p.n_store > 128 || p.n_store % 4 != 0) return false;
    plan = gemm_plan_for(p, dt);
    if (plan.cfg != GEMM_CFG_512x128) {
        p.force_cfg = GEMM_CFG_256x128R;
        plan = gemm_plan_for(p, dt);
    }
    return plan.cfg == GEMM_CFG_512x128 || plan.cfg == GEMM_CFG_256x128R;
}

// The epilogue half of a launch, one builder per kind, on top of the operand builders above: the ONLY places that know which GemmParams fields an epilogue reads and
// reuses. The engine (engine.hip) and the kernel-level C ABI (capi.hip) both launch what these fill.
// typed store (EPI_T): bias, ReLU (flags), up to two residual maps and a ReLU copy, all with the output's row stride
inline void epi_typed_store(GemmParams& p, void* out, int ldo, int flags, const void* res1 = nullptr, const void* res2 = nullptr, void* relu_copy = nullptr) {
    p.epi = EPI_T; p.flags = flags; p.out = out; p.ldo = ldo; p.res1 = res1; p.res2 = res2; p.ldr = ldo; p.out2 = relu_copy; p.ldo2 = ldo;
}
// the DPT head's tail (EPI_HEAD4, the field reuse stated at the enum): ReLU, the 1x1 convolution w4 / b4, postprocess, pts / conf at their pixel strides
inline void epi_head_tail(GemmParams& p, const float* w4, const float* b4, float* pts, int pstride, float* conf, int conf_stride, const PostMode& post) {
    p.epi = EPI_HEAD4; p.flags = GF_RELU; p.out = pts; p.ldo = pstride; p.out2 = conf; p.ldo2 = conf_stride; p.res1 = w4; p.res2 = b4; p.post = post;
}
// ConvTranspose2d(k, stride k) as a GEMM over the th x tw token grid (EPI_CONVT): N = k k cout_pad columns scattered to the k k pixels of every token
inline void epi_convt(GemmParams& p, int k, int cout_pad, int th, int tw, void* out, int ldo) {
    p.epi = EPI_CONVT; p.ksize = k; p.ct_cout = cout_pad; p.Hin = th; p.Win = tw; p.out = out; p.ldo = ldo;
}
// typed residual stream (EPI_F32 with GF_X3RES): out_rows = split-fp16 rows of (acc + bias + res_rows), every row `ld` elements apart; ln_part: GemmParams::ln_part or null
inline void epi_typed_residual(GemmParams& p, const void* res_rows, void* out_rows, int ld, float* ln_part) {
    p.epi = EPI_F32; p.flags = GF_X3RES; p.ldo = ld; p.res1 = res_rows; p.ldr = ld; p.out2 = out_rows; p.ldo2 = ld; p.ln_part = ln_part;
}
// consumer of a folded LayerNorm over the K columns of its input rows (any epilogue; p.bias is the folded bias): GemmParams::ln_rstd ... ln_part_in
inline void ln_consumer(GemmParams& p, const float* rstd, const float* nmr, const float* colsum, const float* part_in, float eps) {
    p.ln_rstd = rstd; p.ln_nmr = nmr; p.ln_colsum = colsum; p.ln_part_in = part_in; p.ln_eps = eps; p.ln_inv_c = 1.0f / (float)p.K;
}
// head scatter (EPI_HEADS): n_regions (<= 3) regions of head_c columns, region r stored as kinds[r] at dsts[r] (dsts null: a host query of the plan)
inline void epi_heads(GemmParams& p, int head_c, int n_regions, const int* kinds, void* const* dsts, int heads, int ntok, int tok_w, int ldv, const float* rope_table) {
    p.epi = EPI_HEADS; p.head_c = head_c; p.heads = heads; p.ntok = ntok; p.tok_w = tok_w; p.ldv = ldv; p.rope_table = rope_table;
    for (int r = 0; r < n_regions; ++r) { p.head_kind[r] = kinds[r]; p.head_dst[r] = dsts ? dsts[r] : nullptr; }
}

// ------------------------------------------------------------------------------ attention
struct AttnParams {
    const void* q = nullptr;   // [B][H][Nq][64]
    const void* k = nullptr;   // [B][H][Nk][64]
    const void* vt = nullptr;  // [B][H][64][ldv]   (ldv >= round_up(Nk, 64), pad zero filled)
    void* out = nullptr;       // [B][Nq][H*64]
    int B = 0, H = 0, Nq = 0, Nk = 0, ldv = 0;
    float scale = 0.125f;
    int out_dt = -1;           // layout of `out` when it differs from the operands' (D3R_F16F8 rows out of a split-fp16 attention); -1: same
};
hipError_t launch_attention(int dt, const AttnParams& p, hipStream_t s);

// ------------------------------------------------------------------------------ elementwise
// LayerNorm over the last dim of an fp32 [rows][C] tensor -> DT [rows][C]
hipError_t launch_layernorm(int dt, const float* x, const float* gamma, const float* beta, void* out, int rows, int C,
                            float eps, hipStream_t s);
// the same from split-fp16 input rows into split-fp16 output rows (enc_norm / dec_norm of a folded-LayerNorm engine: the residual stream is typed)
hipError_t launch_layernorm_x3in(const void* x3rows, const float* gamma, const float* beta, void* out, int rows, int C, float eps, hipStream_t s);
// fp32 -> DT copy (rows x C, contiguous)
hipError_t launch_convert(int dt, const float* x, void* out, size_t n, hipStream_t s);
// NCHW fp32 image -> [B*th*tw][3*ps*ps] patch rows of DT (k = (c, py, px))
hipError_t launch_patchify(int dt, const float* img, void* out, int B, int H, int W, int ps, hipStream_t s);
// standalone in-place 2-D RoPE on tokens[B][N][H][D] (fp32 / bf16 / f16): the reference's native op
hipError_t launch_rope2d(int dt, void* tokens, const int64_t* pos, int B, int N, int H, int D, float base, float F0,
                         hipStream_t s);
hipError_t launch_rope_table(float* table, int max_pos, float base, float F0, hipStream_t s);
// bilinear x2, align_corners=True, NHWC DT -> NHWC DT (optionally also relu copy), output cropped to (Ho, Wo)
hipError_t launch_upsample2x(int dt, const void* in, void* out, void* out_relu, int B, int Hi, int Wi, int C, int cstride,
                             int Ho, int Wo, hipStream_t s);
// final DPT stage: relu'd NHWC DT [pix][C] x W[4][C] + b -> postprocess -> pts3d [pix][3], conf [pix]
hipError_t launch_head_final(int dt, const void* feat, int C, const float* w, const float* b, float* pts, float* conf,
                             size_t npix, int pstride, int cstride, PostMode post, hipStream_t s);
// linear head: proj output fp32 [B*th*tw][(3+1)*ps*ps] -> pixel_shuffle -> postprocess
hipError_t launch_linear_head_post(const float* feat, float* pts, float* conf, int B, int th, int tw, int ps, int pstride, int cstride,
                                   PostMode post, hipStream_t s);
hipError_t launch_fill_zero(void* p, size_t bytes, hipStream_t s);
// folded LayerNorm (GemmParams::ln_part): per row, the G = C / 32 partial (sum, sum of squares) pairs of the producing GEMM -> rstd[m] and
// nmr[m] = -mean rstd (fixed summation order; variance = E[x^2] - mean^2 combined in fp64, eps inside the root like nn.LayerNorm)
hipError_t launch_ln_finalize(const float* part, int rows, int C, float eps, float* rstd, float* nmr, hipStream_t s);
// load-time fold of a LayerNorm into the nn.Linear that consumes it: for each of the N rows of W (fp32 [N][K]): colsum[n] = sum_k r(gamma_k W_nk)
// with r() the rounding of the packed operand type (split-fp16: hi + lo), bias_out[n] = bias_in[n] (or 0) + sum_k beta_k W_nk; fp64 sums
hipError_t launch_ln_fold_vectors(int dt, const float* W, const float* gamma, const float* beta, const float* bias_in, float* colsum, float* bias_out, int N, int K, hipStream_t s);

// load-time weight packing on the device (fp32 PyTorch-layout source -> engine layout in DT)
enum { PACK_MAT = 0, PACK_CONV = 1, PACK_CONVT = 2 };
struct PackParams {
    const float* src = nullptr; void* dst = nullptr;
    size_t numel = 0;
    int kind = PACK_MAT, cols = 0, row_off = 0, dst_cols = 0, cin = 0, cin_pad = 0, ksize = 1, cout_pad = 0;
    const float* kscale = nullptr;   // PACK_MAT: multiply column k of the source by kscale[k] before the conversion (LayerNorm gamma folded into the weights)
};
hipError_t launch_pack_weight(int dt, const PackParams& p, hipStream_t s);
// A Conv2d weight [Cout][Cin][k][k] into rows of k k cin_pad (PACK_CONV), or a ConvTranspose2d weight [Cin][Cout][k][k] into the GEMM matrix of cin_pad columns
// whose N = k k cout_pad rows EPI_CONVT scatters (PACK_CONVT)
inline PackParams conv_pack_params(const float* src, void* dst, bool transposed, int Cout, int Cin, int k, int cin_pad, int cout_pad) {
    PackParams pp;
    pp.src = src; pp.dst = dst; pp.numel = (size_t)Cout * Cin * k * k; pp.ksize = k;
    if (transposed) { pp.kind = PACK_CONVT; pp.cols = Cout; pp.cout_pad = cout_pad; pp.dst_cols = cin_pad; }
    else { pp.kind = PACK_CONV; pp.cin = Cin; pp.cin_pad = cin_pad; pp.dst_cols = k * k * cin_pad; }
    return pp;
}
// The load-time fold of ONE nn.Linear behind a LayerNorm, built in one place (engine.hip) for the engine (finalize_fold) and for the kernel-level C ABI
// (capi.hip d3r_ln_fold_pack): W [N][K] fp32 packed as W diag(gamma) into the rows of `dst` (PACK_MAT with kscale = gamma; K columns per row, padding rows
// zeroed by the caller), then launch_ln_fold_vectors.
hipError_t launch_ln_fold_pack(int dt, const float* W, const float* gamma, const float* beta, const float* bias_in, void* dst, float* colsum, float* bias_out, int N, int K,
                               hipStream_t s);
hipError_t launch_pack_convt_bias(const float* src, float* dst, int cout, int cout_pad, int taps, hipStream_t s);

// ------------------------------------------------------------------------------ aligner
struct AlignerDev;  // defined in aligner.hip

// Row statistics of a folded LayerNorm from the producer's G partial (sum x, sum x^2) pairs, formed by TPR = 1, 2 or 4 ADJACENT lanes per row in the consumer GEMM's prologue
// (GemmParams::ln_part_in) with EXACTLY the arithmetic of ln_finalize_kernel (elementwise.hip: 32 lanes per row, lane g adds pairs g and g + 32 in fp64, xor butterfly 1 .. 16):
// a butterfly over lanes is a balanced binary tree with adjacent pairing, and fp addition commutes, so a thread that owns W = 32 / TPR consecutive lane values reproduces the tree's
// lower levels in registers (a[i] += a[i + o], o = 1, 2, ...) and the upper levels by lane exchange (xor 1, xor 2 = the kernel's xor W, xor 2 W). rstd = 1 / sqrt(max(var, 0) + eps),
// nmr = -mean rstd; every lane of the row returns them.
#if defined(__HIPCC__)
// (sum, sum of squares) of the 4 values a lane holds in the read phase of a typed-residual-stream epilogue: the leaves of the fixed tree of GemmParams::ln_part.
// Contraction is switched OFF here: under -ffp-contract=fast hipcc fuses `x*x + y*y` in one kernel and not in another (gemm.hip's instances kept four rounded
// products, gemm_p4.hip's first version fused them: 6 % of the sums' last bits differed), and the statistics must not depend on which kernel stored the row.
// Four rounded products, pairwise sums -- the arithmetic rounds 5's engine ran and its oracle-parity figures were measured with.
D3R_DEV void ln_quad_sums(const float4& v, float& sm, float& sq) {
#pragma clang fp contract(off)
    const float xx = v.x * v.x, yy = v.y * v.y, zz = v.z * v.z, ww = v.w * v.w;
    sm = (v.x + v.y) + (v.z + v.w);
    sq = (xx + yy) + (zz + ww);
}
// x2 bilinear map (align_corners = True, ATen's source index): the arithmetic shared by upsample2x_quad_kernel (elementwise.hip) and the convolution that interpolates its
// own A operand (gemm_up2.hip), which must reproduce the materialised map bit for bit. Under -ffp-contract=fast hipcc contracts `h*a + l*b` differently from context to
// context -- and, after SLP vectorisation, from one output of the quad kernel to the next -- so every product and fma is written out, with contraction OFF, in the form the
// stand-alone kernel compiled to before the arithmetic was shared (read from its gfx950 disassembly and confirmed on an MI355X against an fp32 emulation of every
// candidate form, element by element; its outputs did not move):
//   up2_scale    the source step of an axis of n input samples
//   up2_src      output index o -> first source sample i0, weights (h, l) of samples i0 and min(i0 + 1, n - 1); the product is rounded before the subtraction
//   up2_lerp     h a + l b as fma(h, a, round(l b)): v_mul_f32 + v_fmac_f32, the form of every interpolation but the two below
//   up2_lerp_rev fma(l, b, round(h a)): the x interpolation of the FIRST source row of a quad (a 2 x 2 block of map pixels on even coordinates) at its EVEN column --
//                the vectoriser packed rows 0 and 1 of that column into one v_pk_mul_f32 / v_pk_fma_f32 pair with the operands of row 0 crossed
//   up2_lerp_rr  round(h a) + round(l b): the y interpolation of the pixel on even row AND even column (v_pk_mul_f32 + v_add_f32)
// up2_pixel_forms states which pixel takes which: a map pixel (oy, ox) with first source row y0 interpolates its top source row with up2_lerp_rev iff ox is even and
// that row is row 0 of its quad (oy even, or oy odd and row oy - 1 starts at the same source row), and its two rows with up2_lerp_rr iff oy and ox are even.
D3R_DEV float up2_scale(int n) { return n > 1 ? (float)(n - 1) / (float)(2 * n - 1) : 0.f; }
D3R_DEV void up2_src(float scale, int o, int& i0, float& l, float& h) {
#pragma clang fp contract(off)
    const float f = scale * (float)o;
    i0 = (int)f;
    l = f - (float)i0;
    h = 1.f - l;
}
D3R_DEV float up2_lerp(float h, float a, float l, float b) {
#pragma clang fp contract(off)
    const float t = l * b;
    return __builtin_fmaf(h, a, t);
}
D3R_DEV float up2_lerp_rev(float h, float a, float l, float b) {
#pragma clang fp contract(off)
    const float t = h * a;
    return __builtin_fmaf(l, b, t);
}
D3R_DEV void up2_pixel_forms(int oy, int ox, int y0, int y0_prev_row, bool& top_rev, bool& y_rr) {
    const bool ecol = !(ox & 1), erow = !(oy & 1);
    top_rev = ecol && (erow || y0 == y0_prev_row);
    y_rr = ecol && erow;
}
D3R_DEV float up2_lerp_rr(float h, float a, float l, float b) {
#pragma clang fp contract(off)
    const float s = h * a, t = l * b;
    return s + t;
}
template <int TPR> D3R_DEV void ln_row_stats(const float2* __restrict__ pr, int G, int sub, float inv_c, float eps, float& rstd, float& nmr) {
    static_assert(TPR == 1 || TPR == 2 || TPR == 4, "threads per row");
    constexpr int W = 32 / TPR;
    double a[W], b[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const int g = sub * W + i;
        double s = 0.0, t = 0.0;
        if (g < G) { const float2 v = pr[g]; s = (double)v.x; t = (double)v.y; }
        if (g + 32 < G) { const float2 v = pr[g + 32]; s += (double)v.x; t += (double)v.y; }
        a[i] = s; b[i] = t;
    }
#pragma unroll
    for (int o = 1; o < W; o <<= 1)
#pragma unroll
        for (int i = 0; i < W; i += 2 * o) { a[i] += a[i + o]; b[i] += b[i + o]; }
    double s = a[0], t = b[0];
    if constexpr (TPR >= 2) { s += __shfl_xor(s, 1); t += __shfl_xor(t, 1); }
    if constexpr (TPR == 4) { s += __shfl_xor(s, 2); t += __shfl_xor(t, 2); }
    const double mean = s * (double)inv_c;
    double var = t * (double)inv_c - mean * mean;
    var = var > 0.0 ? var : 0.0;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
    nmr = (float)(-mean) * rstd;
}
#endif

}  // namespace d3r
