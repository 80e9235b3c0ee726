// dust3r_amd -- C-ABI wrappers of the building-block kernels (include/dust3r_hip.h).
#include "../../include/dust3r_hip.h"
#include "kernels.hpp"

using namespace d3r;

static inline int rup(int a, int b) { return (a + b - 1) / b * b; }

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
    p.epi = EPI_F32; p.flags = GF_X3RES; p.res1 = residual_rows; p.ldr = N; p.out2 = out_rows; p.ldo2 = N; p.ln_part = ln_part;
    return rc_of(launch_gemm(D3R_F16X3, p, (hipStream_t)stream));
}

extern "C" int d3r_rope_table(float* table, int max_pos, float base, float F0, void* stream) {
    if (!table || max_pos <= 0 || !(base > 0.f)) return D3R_ERR_INVALID;
    return rc_of(launch_rope_table(table, max_pos, base, F0, (hipStream_t)stream));
}

// The shape half of an EPI_HEADS launch (d3r_linear_heads, d3r_linear_heads_tile_config): the argument checks of the header, then the GemmParams
// fields the dispatch reads. Weight rows as d3r_linear allocates them.
static bool heads_shape(GemmParams& p, const void* act, const void* wgt, const float* bias, int dtype, int M, int K, int n_regions, int head_c, const int* kinds, int heads, int ntok, int tok_w, int ldv, int max_pos) {
    if (dtype != D3R_BF16 && dtype != D3R_F16 && dtype != D3R_F32 && dtype != D3R_F16X3 && dtype != D3R_F16F8 && dtype != D3R_F16X2F8) return false;
    if (M <= 0 || K <= 0 || n_regions < 1 || n_regions > 3 || !kinds || heads <= 0 || head_c != heads * 64 || ntok <= 0 || tok_w <= 0) return false;
    if (M % ntok != 0 || ntok % tok_w != 0 || (ntok / tok_w > tok_w ? ntok / tok_w : tok_w) > max_pos) return false;
    if (ldv < rup(ntok, 64) || ldv % 64 != 0) return false;
    for (int r = 0; r < n_regions; ++r)
        if (kinds[r] != HEAD_ROPE && kinds[r] != HEAD_VT && kinds[r] != HEAD_PLAIN) return false;
    p = linear_gemm_params(act, K, wgt, bias, M, n_regions * head_c, K);
    p.epi = EPI_HEADS; p.head_c = head_c; p.heads = heads; p.ntok = ntok; p.tok_w = tok_w; p.ldv = ldv;
    for (int r = 0; r < n_regions; ++r) p.head_kind[r] = kinds[r];
    return true;
}

extern "C" int d3r_linear_heads(const void* act, const void* wgt, const float* bias, int M, int K, int n_regions, int head_c, const int* kinds, void* const* dsts,
                                int heads, int ntok, int tok_w, int ldv, const float* rope_table, int max_pos, float* ln_rstd, float* ln_nmr,
                                const float* ln_colsum, const float* ln_part_in, float ln_eps, float* sk_slab, size_t sk_slab_floats, unsigned* sk_cnt,
                                int sk_cnt_n, int dtype, void* stream) {
    if (!act || !wgt || !dsts || !rope_table) return D3R_ERR_INVALID;
    GemmParams p;
    if (!heads_shape(p, act, wgt, bias, dtype, M, K, n_regions, head_c, kinds, heads, ntok, tok_w, ldv, max_pos)) return D3R_ERR_INVALID;
    for (int r = 0; r < n_regions; ++r) {
        if (!dsts[r]) return D3R_ERR_INVALID;
        p.head_dst[r] = dsts[r];
    }
    if ((ln_rstd || ln_nmr || ln_colsum || ln_part_in) && (dtype != D3R_F16X3 || !ln_rstd || !ln_nmr || !ln_colsum)) return D3R_ERR_INVALID;
    p.rope_table = rope_table;
    if (ln_rstd) { p.ln_rstd = ln_rstd; p.ln_nmr = ln_nmr; p.ln_colsum = ln_colsum; p.ln_part_in = ln_part_in; p.ln_eps = ln_eps; p.ln_inv_c = 1.0f / (float)K; }
    if (sk_slab && sk_cnt) { p.splitk = 0; p.sk_slab = sk_slab; p.sk_slab_floats = sk_slab_floats; p.sk_cnt = sk_cnt; p.sk_cnt_n = sk_cnt_n; }      // launch_gemm decides whether it splits (engine.hip launch(), lend_sk: gemm_linear)
    return rc_of(launch_gemm(dtype, p, (hipStream_t)stream));
}

extern "C" int d3r_linear_heads_tile_config(int M, int K, int n_regions, int head_c, const int* kinds, int heads, int ntok, int tok_w, int ldv, int max_pos,
                                            int dtype) {
    static const float dummy = 0.f;
    GemmParams p;
    if (!heads_shape(p, &dummy, &dummy, nullptr, dtype, M, K, n_regions, head_c, kinds, heads, ntok, tok_w, ldv, max_pos)) return D3R_ERR_INVALID;      // (operands never dereferenced)
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
    p.ln_rstd = ln_rstd; p.ln_nmr = ln_nmr; p.ln_colsum = ln_colsum; p.ln_part_in = ln_part_in; p.ln_eps = ln_eps; p.ln_inv_c = 1.0f / (float)K;
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
    p.epi = EPI_T; p.flags = relu ? GF_RELU : 0; p.out = out; p.ldo = Cout; p.res1 = res1; p.res2 = res2; p.ldr = Cout;
    p.out2 = out_relu_copy; p.ldo2 = Cout;
    return rc_of(launch_gemm(dtype, p, (hipStream_t)stream));
}

// ---- the DPT head's kernels alone (include/dust3r_hip.h): the launches of engine.hip run_dpt (through conv / conv_head4 / launch), for the kernel tests -------------------------------
static inline bool conv_dtype(int dtype) { return dtype == D3R_BF16 || dtype == D3R_F16 || dtype == D3R_F32 || dtype == D3R_F16X3; }
static inline bool post_mode(PostMode& pm, int depth_mode, int conf_mode, float vmin, float vmax) {      // d3r_model_set_postprocess's rules
    if (depth_mode < POST_DEPTH_EXP || depth_mode > POST_DEPTH_SQUARE || conf_mode < POST_CONF_EXP || conf_mode > POST_CONF_SIGMOID) return false;
    if (!(vmin < vmax) || (conf_mode == POST_CONF_SIGMOID && !(vmax < __builtin_huge_valf() && vmin > -__builtin_huge_valf()))) return false;
    pm.depth = depth_mode; pm.conf = conf_mode; pm.cmin = vmin; pm.cmax = vmax;
    return true;
}

extern "C" int d3r_pack_conv_weight(const float* src, void* dst, int transposed, int Cout, int Cin, int ksize, int cin_pad, int cout_pad, int dtype,
                                    void* stream) {
    if (!src || !dst || !conv_dtype(dtype) || Cout <= 0 || Cin <= 0 || ksize <= 0) return D3R_ERR_INVALID;
    if (cin_pad < Cin || cin_pad % (128 / (int)dt_bytes(dtype)) != 0 || (transposed && (cout_pad < Cout || cout_pad % 4 != 0))) return D3R_ERR_INVALID;
    PackParams pp;
    pp.src = src; pp.dst = dst; pp.numel = (size_t)Cout * Cin * ksize * ksize; pp.ksize = ksize;
    if (transposed) { pp.kind = PACK_CONVT; pp.cols = Cout; pp.cout_pad = cout_pad; pp.dst_cols = cin_pad; }                 // engine.hip reg_convt / PK_CONVT
    else { pp.kind = PACK_CONV; pp.cin = Cin; pp.cin_pad = cin_pad; pp.dst_cols = ksize * ksize * cin_pad; }                 // engine.hip reg_conv / PK_CONV
    return rc_of(launch_pack_weight(dtype, pp, (hipStream_t)stream));
}

extern "C" int d3r_pack_convt_bias(const float* src, float* dst, int Cout, int cout_pad, int ksize, void* stream) {
    if (!src || !dst || Cout <= 0 || cout_pad < Cout || ksize <= 0) return D3R_ERR_INVALID;
    return rc_of(launch_pack_convt_bias(src, dst, Cout, cout_pad, ksize * ksize, (hipStream_t)stream));
}

extern "C" int d3r_conv2d_nhwc_x(const void* in, const void* wgt, const float* bias, void* out, const void* res1, const void* res2, void* out_relu_copy,
                                 int B, int Hin, int Win, int cstride, int cin_pad, int Cout, int n_store, int ldo, int ksize, int stride, int pad, int flags,
                                 const void* zero_page, int dtype, void* stream) {
    if (!in || !wgt || !out || !zero_page || !conv_dtype(dtype) || B <= 0 || Hin <= 0 || Win <= 0 || Cout <= 0 || ksize <= 0 || stride <= 0 || pad < 0) return D3R_ERR_INVALID;
    if (n_store < 0) n_store = Cout;
    if (cin_pad <= 0 || cin_pad % (128 / (int)dt_bytes(dtype)) != 0 || cstride < cin_pad) return D3R_ERR_INVALID;      // whole K steps per tap, inside a pixel's row
    if (n_store % 4 != 0 || n_store > rup(Cout, 128) || ldo < n_store || (flags & ~(GF_RELU | GF_NOWIDE))) return D3R_ERR_INVALID;
    if (Hin + 2 * pad < ksize || Win + 2 * pad < ksize) return D3R_ERR_INVALID;
    GemmParams p = conv_gemm_params(in, B, Hin, Win, cstride, wgt, bias, cin_pad, Cout, ksize, stride, pad, zero_page);
    p.n_store = n_store;
    p.epi = EPI_T; p.flags = flags; p.out = out; p.ldo = ldo; p.res1 = res1; p.res2 = res2; p.ldr = ldo; p.out2 = out_relu_copy; p.ldo2 = ldo;      // engine.hip conv()
    return rc_of(launch_gemm(dtype, p, (hipStream_t)stream));
}

extern "C" int d3r_convt_gemm(const void* act, const void* wgt, const float* bias, void* out, int B, int th, int tw, int lda, int cin_pad, int cout_pad,
                              int ksize, int ldo, int dtype, void* stream) {
    if (!act || !wgt || !out || !conv_dtype(dtype) || B <= 0 || th <= 0 || tw <= 0 || ksize <= 0) return D3R_ERR_INVALID;
    if (cin_pad <= 0 || cin_pad % (128 / (int)dt_bytes(dtype)) != 0 || lda < cin_pad || cout_pad <= 0 || cout_pad % 4 != 0 || ldo < cout_pad) return D3R_ERR_INVALID;
    const int N = ksize * ksize * cout_pad;
    GemmParams p = linear_gemm_params(act, lda, wgt, bias, B * th * tw, N, cin_pad);      // engine.hip run_dpt, the EPI_CONVT launch: lin_params on the packed matrix
    p.epi = EPI_CONVT; p.ksize = ksize; p.ct_cout = cout_pad;
    p.Hin = th; p.Win = tw; p.out = out; p.ldo = ldo;
    return rc_of(launch_gemm(dtype, p, (hipStream_t)stream));
}

extern "C" int d3r_conv_head4(const void* in, const void* wgt, const float* bias, const float* w4, const float* b4, float* pts, float* conf, int B, int Hin,
                              int Win, int cstride, int cin_pad, int Cout, int ksize, int pstride, int conf_stride, int depth_mode, int conf_mode,
                              float conf_vmin, float conf_vmax, const void* zero_page, int dtype, void* stream) {
    if (!in || !wgt || !w4 || !b4 || !pts || !conf || !zero_page || !conv_dtype(dtype) || B <= 0 || Hin <= 0 || Win <= 0 || Cout <= 0 || ksize <= 0) return D3R_ERR_INVALID;
    if (cin_pad <= 0 || cin_pad % (128 / (int)dt_bytes(dtype)) != 0 || cstride < cin_pad || pstride < 3 || conf_stride < 1) return D3R_ERR_INVALID;
    GemmParams p = conv_gemm_params(in, B, Hin, Win, cstride, wgt, bias, cin_pad, Cout, ksize, 1, 1, zero_page);      // engine.hip conv_head4()
    p.epi = EPI_HEAD4; p.flags = GF_RELU; p.out = pts; p.ldo = pstride; p.out2 = conf; p.ldo2 = conf_stride; p.res1 = w4; p.res2 = b4;
    if (!post_mode(p.post, depth_mode, conf_mode, conf_vmin, conf_vmax)) return D3R_ERR_INVALID;
    GemmPlan plan;
    if (!head4_tile(p, dtype, plan)) return D3R_DECLINED;
    return rc_of(launch_gemm(dtype, p, plan, (hipStream_t)stream));
}

// x2 bilinear map of `src` + d3r_conv_head4 on it: ONE launch where the plan has it (engine.hip conv_up2_head4: the map is never stored), else the two launches of
// today through `map`. Both built by the parameter builders the engine uses (kernels.hpp).
static GemmParams up2_head4_capi_params(const void* src, const void* wgt, const float* bias, const float* w4, const float* b4, float* pts, float* conf, int B, int Hi,
                                        int Wi, int cstride, int cin_pad, int Cout, int pstride, int conf_stride, const void* zero_page) {
    GemmParams p = conv_up2_gemm_params(src, B, Hi, Wi, cstride, wgt, bias, cin_pad, Cout, zero_page);
    p.epi = EPI_HEAD4; p.flags = GF_RELU; p.out = pts; p.ldo = pstride; p.out2 = conf; p.ldo2 = conf_stride; p.res1 = w4; p.res2 = b4;
    return p;
}
// the typed-store form (engine.hip conv_up2): d3r_conv2d_nhwc_x's launch without residuals or ReLU copy
static GemmParams up2_conv_capi_params(const void* src, const void* wgt, const float* bias, void* out, int B, int Hi, int Wi, int cstride, int cin_pad, int Cout, int ldo,
                                       int flags, const void* zero_page) {
    GemmParams p = conv_up2_gemm_params(src, B, Hi, Wi, cstride, wgt, bias, cin_pad, Cout, zero_page);
    p.epi = EPI_T; p.flags = flags; p.out = out; p.ldo = ldo; p.ldr = ldo; p.ldo2 = ldo;
    return p;
}
extern "C" int d3r_up2_conv_route(int dtype, int B, int Hi, int Wi, int cstride, int cin_pad, int Cout, int head4) {
    if (!conv_dtype(dtype) || B <= 0 || Hi <= 0 || Wi <= 0 || Cout <= 0 || cin_pad <= 0 || cstride < cin_pad) return D3R_ERR_INVALID;
    const GemmParams p = head4 ? up2_head4_capi_params(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, B, Hi, Wi, cstride, cin_pad, Cout, 3, 1, nullptr)
                               : up2_conv_capi_params(nullptr, nullptr, nullptr, nullptr, B, Hi, Wi, cstride, cin_pad, Cout, rup(Cout, 8), 0, nullptr);
    return gemm_plan_for(p, dtype).up2 ? 1 : 0;
}
extern "C" int d3r_up2_conv2d_nhwc_x(const void* src, void* map, const void* wgt, const float* bias, void* out, int B, int Hi, int Wi, int cstride, int cin_pad, int Cout,
                                     int ldo, int flags, const void* zero_page, int dtype, void* stream) {
    if (!src || !wgt || !out || !zero_page || !conv_dtype(dtype) || B <= 0 || Hi <= 0 || Wi <= 0 || Cout <= 0) return D3R_ERR_INVALID;
    if (cin_pad <= 0 || cin_pad % (128 / (int)dt_bytes(dtype)) != 0 || cstride < cin_pad || cstride % 8 != 0 || Cout % 4 != 0 || ldo < Cout || (flags & ~(GF_RELU | GF_NOWIDE))) return D3R_ERR_INVALID;
    GemmParams p = up2_conv_capi_params(src, wgt, bias, out, B, Hi, Wi, cstride, cin_pad, Cout, ldo, flags, zero_page);
    const GemmPlan plan = gemm_plan_for(p, dtype);
    if (plan.up2) return rc_of(launch_gemm(dtype, p, plan, (hipStream_t)stream));
    if (!map) return D3R_ERR_INVALID;
    const int rc = rc_of(launch_upsample2x(dtype, src, map, nullptr, B, Hi, Wi, cstride, cstride, 2 * Hi, 2 * Wi, (hipStream_t)stream));
    if (rc != D3R_OK) return rc;
    return d3r_conv2d_nhwc_x(map, wgt, bias, out, nullptr, nullptr, nullptr, B, 2 * Hi, 2 * Wi, cstride, cin_pad, Cout, Cout, ldo, 3, 1, 1, flags, zero_page, dtype, stream);
}
extern "C" int d3r_up2_conv_head4(const void* src, void* map, const void* wgt, const float* bias, const float* w4, const float* b4, float* pts, float* conf, int B,
                                  int Hi, int Wi, int cstride, int cin_pad, int Cout, int pstride, int conf_stride, int depth_mode, int conf_mode, float conf_vmin,
                                  float conf_vmax, const void* zero_page, int dtype, void* stream) {
    if (!src || !wgt || !w4 || !b4 || !pts || !conf || !zero_page || !conv_dtype(dtype) || B <= 0 || Hi <= 0 || Wi <= 0 || Cout <= 0) return D3R_ERR_INVALID;
    if (cin_pad <= 0 || cin_pad % (128 / (int)dt_bytes(dtype)) != 0 || cstride < cin_pad || cstride % 8 != 0 || pstride < 3 || conf_stride < 1) return D3R_ERR_INVALID;
    GemmParams p = up2_head4_capi_params(src, wgt, bias, w4, b4, pts, conf, B, Hi, Wi, cstride, cin_pad, Cout, pstride, conf_stride, zero_page);
    if (!post_mode(p.post, depth_mode, conf_mode, conf_vmin, conf_vmax)) return D3R_ERR_INVALID;
    const GemmPlan plan = gemm_plan_for(p, dtype);
    if (plan.up2) return rc_of(launch_gemm(dtype, p, plan, (hipStream_t)stream));
    if (!map) return D3R_ERR_INVALID;
    const int rc = rc_of(launch_upsample2x(dtype, src, map, nullptr, B, Hi, Wi, cstride, cstride, 2 * Hi, 2 * Wi, (hipStream_t)stream));
    if (rc != D3R_OK) return rc;
    return d3r_conv_head4(map, wgt, bias, w4, b4, pts, conf, B, 2 * Hi, 2 * Wi, cstride, cin_pad, Cout, 3, pstride, conf_stride, depth_mode, conf_mode, conf_vmin, conf_vmax,
                          zero_page, dtype, stream);
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
    if (dtype != D3R_BF16 && dtype != D3R_F16 && dtype != D3R_F32 && dtype != D3R_F16X3 && dtype != D3R_F16F8 && dtype != D3R_F16X2F8) return D3R_ERR_INVALID;
    static const float dummy = 0.f;
    GemmParams p = linear_gemm_params(&dummy, K, &dummy, nullptr, M, N, K);      // (never dereferenced: the rules only ask whether the operands exist)
    p.epi = epilogue == 1 ? EPI_F32 : (epilogue == 2 ? EPI_GELU : EPI_T);
    p.res1 = (epilogue == 1 && with_residual) ? &dummy : nullptr;
    p.out = const_cast<float*>(&dummy);
    return gemm_plan_for(p, dtype).cfg;
}

