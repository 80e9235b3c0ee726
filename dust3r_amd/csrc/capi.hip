// dust3r_amd -- C-ABI wrappers of the building-block kernels (include/dust3r_hip.h).
#include "../../include/dust3r_hip.h"
#include "kernels.hpp"

using namespace d3r;

extern "C" int d3r_rope2d(void* tokens, const int64_t* positions, int B, int N, int H, int D, float base, float F0, int dtype, void* stream) {
    if (!tokens || !positions) return D3R_ERR_INVALID;
    return rc_of(launch_rope2d(dtype, tokens, positions, B, N, H, D, base, F0, (hipStream_t)stream));
}

extern "C" int d3r_layernorm(const float* x, const float* gamma, const float* beta, void* out, int rows, int C, float eps, int dtype, void* stream) {
    if (!x || !gamma || !beta || !out) return D3R_ERR_INVALID;
    return rc_of(launch_layernorm(dtype, x, gamma, beta, out, rows, C, eps, (hipStream_t)stream));
}

extern "C" int d3r_linear(const void* act, const void* wgt, const float* bias, void* out, const float* residual, int M, int N, int K, int epilogue,
                          int dtype, void* stream) {
    if (!act || !wgt || !out || N % 4 != 0) return D3R_ERR_INVALID;
    GemmParams p = linear_gemm_params(act, K, wgt, bias, M, N, K);
    p.epi = epilogue == 1 ? EPI_F32 : (epilogue == 2 ? EPI_GELU : EPI_T);
    p.out = out; p.ldo = N; p.res1 = epilogue == 1 ? residual : nullptr; p.ldr = N;
    return rc_of(launch_gemm(dtype, p, (hipStream_t)stream));
}

// nn.Linear whose output joins the typed residual stream of a folded-LayerNorm engine (GemmParams GF_X3RES): out_rows = split-fp16 rows of
// (act . wgt^T + bias + residual_rows), ln_part (optional) = the (sum, sum of squares) of every 32-column group of every stored row.
extern "C" int d3r_linear_x3res(const void* act, const void* wgt, const float* bias, void* out_rows, const void* residual_rows, float* ln_part, int M, int N,
                                int K, void* stream) {
    if (!act || !wgt || !out_rows || N % 8 != 0) return D3R_ERR_INVALID;
    GemmParams p = linear_gemm_params(act, K, wgt, bias, M, N, K);
    epi_typed_residual(p, residual_rows, out_rows, N, ln_part);
    return rc_of(launch_gemm(D3R_F16X3, p, (hipStream_t)stream));
}

extern "C" int d3r_rope_table(float* table, int max_pos, float base, float F0, void* stream) {
    if (!table || max_pos <= 0 || !(base > 0.f)) return D3R_ERR_INVALID;
    return rc_of(launch_rope_table(table, max_pos, base, F0, (hipStream_t)stream));
}

// The shape half of an EPI_HEADS launch (d3r_linear_heads, d3r_linear_heads_tile_config): the argument checks of the header, then the GemmParams
// fields the dispatch reads. Weight rows as d3r_linear allocates them.
static bool heads_shape(GemmParams& p, const void* act, const void* wgt, const float* bias, int dtype, int M, int K, int n_regions, int head_c, const int* kinds, void* const* dsts, int heads, int ntok, int tok_w, int ldv, const float* rope_table, int max_pos) {
    if (!gemm_dtype(dtype)) return false;
    if (M <= 0 || K <= 0 || n_regions < 1 || n_regions > 3 || !kinds || heads <= 0 || head_c != heads * 64 || ntok <= 0 || tok_w <= 0) return false;
    if (M % ntok != 0 || ntok % tok_w != 0 || (ntok / tok_w > tok_w ? ntok / tok_w : tok_w) > max_pos) return false;
    if (ldv < rup(ntok, 64) || ldv % 64 != 0) return false;
    for (int r = 0; r < n_regions; ++r)
        if ((kinds[r] != HEAD_ROPE && kinds[r] != HEAD_VT && kinds[r] != HEAD_PLAIN) || (dsts && !dsts[r])) return false;
    p = linear_gemm_params(act, K, wgt, bias, M, n_regions * head_c, K);
    epi_heads(p, head_c, n_regions, kinds, dsts, heads, ntok, tok_w, ldv, rope_table);
    return true;
}

extern "C" int d3r_linear_heads(const void* act, const void* wgt, const float* bias, int M, int K, int n_regions, int head_c, const int* kinds, void* const* dsts,
                                int heads, int ntok, int tok_w, int ldv, const float* rope_table, int max_pos, float* ln_rstd, float* ln_nmr,
                                const float* ln_colsum, const float* ln_part_in, float ln_eps, float* sk_slab, size_t sk_slab_floats, unsigned* sk_cnt,
                                int sk_cnt_n, int dtype, void* stream) {
    if (!act || !wgt || !dsts || !rope_table) return D3R_ERR_INVALID;
    GemmParams p;
    if (!heads_shape(p, act, wgt, bias, dtype, M, K, n_regions, head_c, kinds, dsts, heads, ntok, tok_w, ldv, rope_table, max_pos)) return D3R_ERR_INVALID;
    if ((ln_rstd || ln_nmr || ln_colsum || ln_part_in) && (dtype != D3R_F16X3 || !ln_rstd || !ln_nmr || !ln_colsum)) return D3R_ERR_INVALID;
    if (ln_rstd) ln_consumer(p, ln_rstd, ln_nmr, ln_colsum, ln_part_in, ln_eps);
    if (sk_slab && sk_cnt) { p.splitk = 0; p.sk_slab = sk_slab; p.sk_slab_floats = sk_slab_floats; p.sk_cnt = sk_cnt; p.sk_cnt_n = sk_cnt_n; }      // launch_gemm decides whether it splits (engine.hip launch(), lend_sk: gemm_linear)
    return rc_of(launch_gemm(dtype, p, (hipStream_t)stream));
}

extern "C" int d3r_linear_heads_tile_config(int M, int K, int n_regions, int head_c, const int* kinds, int heads, int ntok, int tok_w, int ldv, int max_pos,
                                            int dtype) {
    static const float dummy = 0.f;
    GemmParams p;
    if (!heads_shape(p, &dummy, &dummy, nullptr, dtype, M, K, n_regions, head_c, kinds, nullptr, heads, ntok, tok_w, ldv, nullptr, max_pos)) return D3R_ERR_INVALID;      // (operands never dereferenced)
    const GemmPlan plan = gemm_plan_for(p, dtype);
    return plan.w8 ? D3R_TILE_128W8 : plan.cfg;
}

// ---- The folded-LayerNorm chain alone, for the kernel tests: the launches the engine makes between a typed-residual GEMM (d3r_linear_x3res,
// the producer of the partial sums) and the GEMM that consumes the statistics. d3r_linear_heads above is the consumer with the head-scatter epilogue.
extern "C" int d3r_ln_finalize(const float* part, int rows, int C, float eps, float* rstd, float* nmr, void* stream) {
    if (!part || !rstd || !nmr || rows <= 0 || C <= 0 || C % 32 != 0 || C > 2048) return D3R_ERR_INVALID;
    return rc_of(launch_ln_finalize(part, rows, C, eps, rstd, nmr, (hipStream_t)stream));
}

// What finalize_fold (engine.hip) runs for one matrix, through the same function: split-fp16 is the only layout a fold engine packs.
extern "C" int d3r_ln_fold_pack(const float* W, const float* gamma, const float* beta, const float* bias_in, void* dst_rows, float* colsum, float* bias_out, int N,
                                int K, int dtype, void* stream) {
    if (!W || !gamma || !beta || !dst_rows || !colsum || !bias_out || N <= 0 || K <= 0 || K % 8 != 0 || dtype != D3R_F16X3) return D3R_ERR_INVALID;
    return rc_of(launch_ln_fold_pack(dtype, W, gamma, beta, bias_in, dst_rows, colsum, bias_out, N, K, (hipStream_t)stream));
}

// d3r_linear (split-fp16, typed store or GELU) as the consumer of a folded LayerNorm: the ln_* fields exactly as d3r_linear_heads fills them.
extern "C" int d3r_linear_ln(const void* act_rows, const void* wgt, const float* bias_fold, void* out, int M, int N, int K, int epilogue, float* ln_rstd,
                             float* ln_nmr, const float* ln_colsum, const float* ln_part_in, float ln_eps, void* stream) {
    if (!act_rows || !wgt || !out || !ln_rstd || !ln_nmr || !ln_colsum || M <= 0 || N <= 0 || N % 8 != 0 || K <= 0 || (epilogue != 0 && epilogue != 2)) return D3R_ERR_INVALID;
    if (ln_part_in && (K % 32 != 0 || K > 2048)) return D3R_ERR_INVALID;
    GemmParams p = linear_gemm_params(act_rows, K, wgt, bias_fold, M, N, K);
    p.epi = epilogue == 2 ? EPI_GELU : EPI_T;
    p.out = out; p.ldo = N;
    ln_consumer(p, ln_rstd, ln_nmr, ln_colsum, ln_part_in, ln_eps);
    return rc_of(launch_gemm(D3R_F16X3, p, (hipStream_t)stream));
}

// enc_norm / dec_norm of a folded-LayerNorm engine: LayerNorm from split-fp16 rows into split-fp16 rows
extern "C" int d3r_layernorm_x3rows(const void* rows, const float* gamma, const float* beta, void* out_rows, int M, int C, float eps, void* stream) {
    if (!rows || !gamma || !beta || !out_rows || M <= 0 || C <= 0 || C % 8 != 0 || C > 2048) return D3R_ERR_INVALID;
    return rc_of(launch_layernorm_x3in(rows, gamma, beta, out_rows, M, C, eps, (hipStream_t)stream));
}

extern "C" int d3r_conv_k_slice_major(void) { return 1; }

extern "C" int d3r_conv2d_nhwc(const void* in, const void* wgt, const float* bias, void* out, const void* res1, const void* res2, void* out_relu_copy,
                               int B, int Hin, int Win, int Cin, int Cout, int ksize, int stride, int pad, int relu, const void* zero_page, int dtype,
                               void* stream) {
    if (!in || !wgt || !out || !zero_page || Cout % 4 != 0) return D3R_ERR_INVALID;
    GemmParams p = conv_gemm_params(in, B, Hin, Win, Cin, wgt, bias, Cin, Cout, ksize, stride, pad, zero_page);
    epi_typed_store(p, out, Cout, relu ? GF_RELU : 0, res1, res2, out_relu_copy);
    return rc_of(launch_gemm(dtype, p, (hipStream_t)stream));
}

// ---- the DPT head's kernels alone (include/dust3r_hip.h): the launches of engine.hip run_dpt (through conv / conv_head4 / launch), for the kernel tests -------------------------------
extern "C" int d3r_pack_conv_weight(const float* src, void* dst, int transposed, int Cout, int Cin, int ksize, int cin_pad, int cout_pad, int dtype,
                                    void* stream) {
    if (!src || !dst || Cout <= 0 || Cin <= 0 || ksize <= 0 || !conv_operand_ok(dtype, cin_pad, cin_pad)) return D3R_ERR_INVALID;
    if (cin_pad < Cin || (transposed && (cout_pad < Cout || cout_pad % 4 != 0))) return D3R_ERR_INVALID;
    return rc_of(launch_pack_weight(dtype, conv_pack_params(src, dst, transposed != 0, Cout, Cin, ksize, cin_pad, cout_pad), (hipStream_t)stream));      // engine.hip pack_slot's
}

extern "C" int d3r_pack_convt_bias(const float* src, float* dst, int Cout, int cout_pad, int ksize, void* stream) {
    if (!src || !dst || Cout <= 0 || cout_pad < Cout || ksize <= 0) return D3R_ERR_INVALID;
    return rc_of(launch_pack_convt_bias(src, dst, Cout, cout_pad, ksize * ksize, (hipStream_t)stream));
}

extern "C" int d3r_conv2d_nhwc_x(const void* in, const void* wgt, const float* bias, void* out, const void* res1, const void* res2, void* out_relu_copy,
                                 int B, int Hin, int Win, int cstride, int cin_pad, int Cout, int n_store, int ldo, int ksize, int stride, int pad, int flags,
                                 const void* zero_page, int dtype, void* stream) {
    if (!in || !wgt || !out || !zero_page || !conv_operand_ok(dtype, cin_pad, cstride) || B <= 0 || Hin <= 0 || Win <= 0 || Cout <= 0 || ksize <= 0 || stride <= 0 || pad < 0) return D3R_ERR_INVALID;
    if (n_store < 0) n_store = Cout;
    if (n_store % 4 != 0 || n_store > gemm_n_pad(Cout) || ldo < n_store || (flags & ~(GF_RELU | GF_NOWIDE))) return D3R_ERR_INVALID;
    if (Hin + 2 * pad < ksize || Win + 2 * pad < ksize) return D3R_ERR_INVALID;
    GemmParams p = conv_gemm_params(in, B, Hin, Win, cstride, wgt, bias, cin_pad, Cout, ksize, stride, pad, zero_page);
    p.n_store = n_store;
    epi_typed_store(p, out, ldo, flags, res1, res2, out_relu_copy);      // engine.hip conv()
    return rc_of(launch_gemm(dtype, p, (hipStream_t)stream));
}

extern "C" int d3r_convt_gemm(const void* act, const void* wgt, const float* bias, void* out, int B, int th, int tw, int lda, int cin_pad, int cout_pad,
                              int ksize, int ldo, int dtype, void* stream) {
    if (!act || !wgt || !out || !conv_operand_ok(dtype, cin_pad, lda) || B <= 0 || th <= 0 || tw <= 0 || ksize <= 0) return D3R_ERR_INVALID;
    if (cout_pad <= 0 || cout_pad % 4 != 0 || ldo < cout_pad) return D3R_ERR_INVALID;
    const int N = ksize * ksize * cout_pad;
    GemmParams p = linear_gemm_params(act, lda, wgt, bias, B * th * tw, N, cin_pad);      // engine.hip run_dpt, the EPI_CONVT launch: lin_params on the packed matrix
    epi_convt(p, ksize, cout_pad, th, tw, out, ldo);
    return rc_of(launch_gemm(dtype, p, (hipStream_t)stream));
}

extern "C" int d3r_conv_head4(const void* in, const void* wgt, const float* bias, const float* w4, const float* b4, float* pts, float* conf, int B, int Hin,
                              int Win, int cstride, int cin_pad, int Cout, int ksize, int pstride, int conf_stride, int depth_mode, int conf_mode,
                              float conf_vmin, float conf_vmax, const void* zero_page, int dtype, void* stream) {
    PostMode pm;
    if (!in || !wgt || !w4 || !b4 || !pts || !conf || !zero_page || !conv_operand_ok(dtype, cin_pad, cstride) || B <= 0 || Hin <= 0 || Win <= 0 || Cout <= 0 || ksize <= 0) return D3R_ERR_INVALID;
    if (pstride < 3 || conf_stride < 1 || !post_mode(pm, depth_mode, conf_mode, conf_vmin, conf_vmax)) return D3R_ERR_INVALID;
    GemmParams p = conv_gemm_params(in, B, Hin, Win, cstride, wgt, bias, cin_pad, Cout, ksize, 1, 1, zero_page);      // engine.hip conv_head4()
    epi_head_tail(p, w4, b4, pts, pstride, conf, conf_stride, pm);
    GemmPlan plan;
    if (!head4_tile(p, dtype, plan)) return D3R_DECLINED;
    return rc_of(launch_gemm(dtype, p, plan, (hipStream_t)stream));
}

// x2 bilinear map of `src` + a 3x3 convolution on it: ONE launch where the plan has it (engine.hip conv_up2 / conv_up2_head4: the map is never stored), else the x2 map
// into `map` and `conv_on_map`, the entry of the convolution alone. `p`: the AMODE_CONV_UP2 launch, built by the parameter builders the engine uses (kernels.hpp).
template <typename ConvOnMap>
static int up2_fused_or_two_launches(const GemmParams& p, int dtype, const void* src, void* map, int B, int Hi, int Wi, int cstride, void* stream, ConvOnMap conv_on_map) {
    const GemmPlan plan = gemm_plan_for(p, dtype);
    if (plan.up2) return rc_of(launch_gemm(dtype, p, plan, (hipStream_t)stream));
    if (!map) return D3R_ERR_INVALID;
    const int rc = rc_of(launch_upsample2x(dtype, src, map, nullptr, B, Hi, Wi, cstride, cstride, 2 * Hi, 2 * Wi, (hipStream_t)stream));
    return rc != D3R_OK ? rc : conv_on_map();
}
extern "C" int d3r_up2_conv_route(int dtype, int B, int Hi, int Wi, int cstride, int cin_pad, int Cout, int head4) {
    if (!conv_dtype(dtype) || B <= 0 || Hi <= 0 || Wi <= 0 || Cout <= 0 || cin_pad <= 0 || cstride < cin_pad) return D3R_ERR_INVALID;
    GemmParams p = conv_up2_gemm_params(nullptr, B, Hi, Wi, cstride, nullptr, nullptr, cin_pad, Cout, nullptr);
    if (head4) epi_head_tail(p, nullptr, nullptr, nullptr, 3, nullptr, 1, PostMode());
    else epi_typed_store(p, nullptr, rup(Cout, 8), 0);
    return gemm_plan_for(p, dtype).up2 ? 1 : 0;
}
extern "C" int d3r_up2_conv2d_nhwc_x(const void* src, void* map, const void* wgt, const float* bias, void* out, int B, int Hi, int Wi, int cstride, int cin_pad, int Cout,
                                     int ldo, int flags, const void* zero_page, int dtype, void* stream) {
    if (!src || !wgt || !out || !zero_page || !conv_operand_ok(dtype, cin_pad, cstride) || B <= 0 || Hi <= 0 || Wi <= 0 || Cout <= 0) return D3R_ERR_INVALID;
    if (cstride % 8 != 0 || Cout % 4 != 0 || ldo < Cout || (flags & ~(GF_RELU | GF_NOWIDE))) return D3R_ERR_INVALID;
    GemmParams p = conv_up2_gemm_params(src, B, Hi, Wi, cstride, wgt, bias, cin_pad, Cout, zero_page);
    epi_typed_store(p, out, ldo, flags);      // engine.hip conv_up2: d3r_conv2d_nhwc_x's launch without residuals or ReLU copy
    return up2_fused_or_two_launches(p, dtype, src, map, B, Hi, Wi, cstride, stream, [&] {
        return d3r_conv2d_nhwc_x(map, wgt, bias, out, nullptr, nullptr, nullptr, B, 2 * Hi, 2 * Wi, cstride, cin_pad, Cout, Cout, ldo, 3, 1, 1, flags, zero_page, dtype, stream);
    });
}
extern "C" int d3r_up2_conv_head4(const void* src, void* map, const void* wgt, const float* bias, const float* w4, const float* b4, float* pts, float* conf, int B,
                                  int Hi, int Wi, int cstride, int cin_pad, int Cout, int pstride, int conf_stride, int depth_mode, int conf_mode, float conf_vmin,
                                  float conf_vmax, const void* zero_page, int dtype, void* stream) {
    PostMode pm;
    if (!src || !wgt || !w4 || !b4 || !pts || !conf || !zero_page || !conv_operand_ok(dtype, cin_pad, cstride) || B <= 0 || Hi <= 0 || Wi <= 0 || Cout <= 0) return D3R_ERR_INVALID;
    if (cstride % 8 != 0 || pstride < 3 || conf_stride < 1 || !post_mode(pm, depth_mode, conf_mode, conf_vmin, conf_vmax)) return D3R_ERR_INVALID;
    GemmParams p = conv_up2_gemm_params(src, B, Hi, Wi, cstride, wgt, bias, cin_pad, Cout, zero_page);
    epi_head_tail(p, w4, b4, pts, pstride, conf, conf_stride, pm);      // engine.hip conv_up2_head4
    return up2_fused_or_two_launches(p, dtype, src, map, B, Hi, Wi, cstride, stream, [&] {
        return d3r_conv_head4(map, wgt, bias, w4, b4, pts, conf, B, 2 * Hi, 2 * Wi, cstride, cin_pad, Cout, 3, pstride, conf_stride, depth_mode, conf_mode, conf_vmin, conf_vmax,
                              zero_page, dtype, stream);
    });
}

extern "C" int d3r_head_final(const void* feat, int C, const float* w4, const float* b4, float* pts, float* conf, size_t npix, int pstride, int conf_stride,
                              int depth_mode, int conf_mode, float conf_vmin, float conf_vmax, int dtype, void* stream) {
    PostMode pm;
    if (!feat || !w4 || !b4 || !pts || !conf || !conv_dtype(dtype) || C <= 0 || C % 8 != 0 || npix == 0 || pstride < 3 || conf_stride < 1) return D3R_ERR_INVALID;
    if (!post_mode(pm, depth_mode, conf_mode, conf_vmin, conf_vmax)) return D3R_ERR_INVALID;
    return rc_of(launch_head_final(dtype, feat, C, w4, b4, pts, conf, npix, pstride, conf_stride, pm, (hipStream_t)stream));
}

extern "C" int d3r_linear_head_post(const float* feat, float* pts, float* conf, int B, int th, int tw, int ps, int pstride, int conf_stride, int depth_mode,
                                    int conf_mode, float conf_vmin, float conf_vmax, void* stream) {
    PostMode pm;
    if (!feat || !pts || !conf || B <= 0 || th <= 0 || tw <= 0 || ps <= 0 || pstride < 3 || conf_stride < 1) return D3R_ERR_INVALID;
    if (!post_mode(pm, depth_mode, conf_mode, conf_vmin, conf_vmax)) return D3R_ERR_INVALID;
    return rc_of(launch_linear_head_post(feat, pts, conf, B, th, tw, ps, pstride, conf_stride, pm, (hipStream_t)stream));
}

extern "C" int d3r_attention(const void* q, const void* k, const void* vt, void* out, int B, int H, int Nq, int Nk, int ldv, float scale, int dtype,
                             void* stream) {
    if (!q || !k || !vt || !out) return D3R_ERR_INVALID;
    AttnParams a;
    a.q = q; a.k = k; a.vt = vt; a.out = out; a.B = B; a.H = H; a.Nq = Nq; a.Nk = Nk; a.ldv = ldv; a.scale = scale;
    return rc_of(launch_attention(dtype, a, (hipStream_t)stream));
}

// d3r_attention with the layout of the output rows named: `out_rows` is the dtype id of the GEMM that reads them (the engine's proj launch), so a
// split-fp16 attention can be asked for the fp16 + fp8 activation rows its kernels store for the fp16f8 / fp16x2f8 modes.
extern "C" int d3r_attention_rows(const void* q, const void* k, const void* vt, void* out, int B, int H, int Nq, int Nk, int ldv, float scale, int dtype,
                                  int out_rows, void* stream) {
    if (!q || !k || !vt || !out || out_rows < D3R_BF16 || out_rows > D3R_F16X2F8) return D3R_ERR_INVALID;
    AttnParams a;
    a.q = q; a.k = k; a.vt = vt; a.out = out; a.B = B; a.H = H; a.Nq = Nq; a.Nk = Nk; a.ldv = ldv; a.scale = scale; a.out_dt = out_rows;
    return rc_of(launch_attention(dtype, a, (hipStream_t)stream));
}

extern "C" int d3r_upsample2x_nhwc(const void* in, void* out, int B, int Hi, int Wi, int C, int Ho, int Wo, int dtype, void* stream) {
    if (!in || !out) return D3R_ERR_INVALID;
    return rc_of(launch_upsample2x(dtype, in, out, nullptr, B, Hi, Wi, C, C, Ho, Wo, (hipStream_t)stream));
}

// Diagnostics: per-block phase timestamps of every following GEMM launch into `buf` (8 x uint64 per block; NULL switches it off).
extern "C" int d3r_gemm_set_trace(void* buf, size_t capacity_blocks) {
    gemm_set_trace((unsigned long long*)buf, buf ? capacity_blocks : 0);
    return D3R_OK;
}

// 0: there is one build flavour, without the ablation kernels of earlier rounds; kept for the C ABI
extern "C" int d3r_build_has_probes(void) { return 0; }

// Diagnostics, host only (no GPU, no launch): the tile configuration of the plan (gemm_plan.hpp) that d3r_linear runs for an nn.Linear-shaped problem
// (same `epilogue` codes as d3r_linear; with_residual: an fp32 residual is added). The dispatch table of DESIGN.md section 4.1 as a function.
extern "C" int d3r_gemm_tile_config(int dtype, int M, int N, int K, int epilogue, int with_residual) {
    if (M <= 0 || N <= 0 || K <= 0 || N % 4 != 0) return D3R_ERR_INVALID;
    if (!gemm_dtype(dtype)) return D3R_ERR_INVALID;
    static const float dummy = 0.f;
    GemmParams p = linear_gemm_params(&dummy, K, &dummy, nullptr, M, N, K);      // (never dereferenced: the rules only ask whether the operands exist)
    p.epi = epilogue == 1 ? EPI_F32 : (epilogue == 2 ? EPI_GELU : EPI_T);
    p.res1 = (epilogue == 1 && with_residual) ? &dummy : nullptr;
    p.out = const_cast<float*>(&dummy);
    return gemm_plan_for(p, dtype).cfg;
}

