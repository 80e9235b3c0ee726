// dust3r_amd -- model engine: weight packing + forward orchestration for
// AsymmetricCroCo3DStereo.forward (reference dust3r/model.py:199-211).
//
// The engine owns its device memory (weights packed once at load time into the layouts the
// kernels want; one workspace arena grown on demand) and enqueues the whole forward -- ~600
// kernel launches -- from C++ on the caller's stream, so the Python host makes ONE ctypes call
// per batch. Data layout in HBM:
//   residual streams  fp32  [tokens][C]           (LayerNorm, residual adds stay fp32)
//   GEMM operands     dtype [tokens][C]           (bf16 / f16 / f32 / split-fp16 per d3r_model_config.dtype; with D3R_DTYPE_F16F8 the
//                                                  inputs and weights of the transformer blocks' linears are fp16 + fp8 rows, the rest split-fp16)
//   q, k              dtype [B][H][N][64]  (RoPE applied), v^T dtype [B][H][64][ldv]
//   DPT feature maps  dtype NHWC, channel stride padded to the next K-tile multiple
//   outputs           fp32  pts3d [B][H][W][3], conf [B][H][W]   (the reference's output layout)
#include <math.h>
#include <string.h>

#include <map>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/dust3r_hip.h"
#include "kernels.hpp"

using namespace d3r;

namespace {

enum PackKind { PK_VEC, PK_MAT, PK_CONV, PK_CONVT, PK_CONVT_BIAS, PK_IGNORE };

struct Slot {
    PackKind kind = PK_IGNORE;
    void* dst = nullptr;      // device destination (matrix in dtype or fp32 vector)
    int rows = 0, cols = 0;   // expected logical (N, K) / vector length in rows
    int row_off = 0;          // first destination row (concatenated matrices / biases)
    int dst_cols = 0;         // destination row length (K, possibly padded)
    int cin = 0, cin_pad = 0, ksize = 1, cout_pad = 0;
    int dt = -1;              // layout of a packed matrix (-1: the model's dtype; the transformer blocks' matrices may be fp16 + fp8 rows)
    bool loaded = false, explicit_loaded = false;
    std::string mirror;       // dec_blocks.* -> dec_blocks2.* duplication
    struct Lin* fold = nullptr;   // PK_MAT: this matrix has the LayerNorm in front of it folded in (ln_fold engines): staged in fp32, packed by finalize_fold
    bool refold = false;          // PK_VEC: a LayerNorm weight / bias or the bias of a folded nn.Linear -- a new value makes the fold stale
    std::vector<struct Lin*> refold_lins;   // ... of these matrices (only THEY are re-folded: round 6)
    unsigned fold_bit = 0;        // PK_MAT with a fold: this slot's bit in Lin::want_mask (a Lin fed by several tensors -- projk | projv -- is complete when all were staged)
};

struct LNp { float* g = nullptr; float* b = nullptr; };
// dt: operand layout of this GEMM. ln != nullptr (ln_fold engines): W is packed as W diag(gamma), b_fold = b + W beta, ln_s[n] = sum_k of the packed row n
struct Lin { void* w = nullptr; float* b = nullptr; int N = 0, K = 0, n_pad = 0, n_rows = 0, dt = 0;
             const LNp* ln = nullptr; float* ln_s = nullptr; float* b_fold = nullptr; float* w32 = nullptr;
             bool fold_dirty = false; unsigned want_mask = 0, have_mask = 0; };      // fold bookkeeping per matrix: stale? which of its weight tensors sit in w32?
struct EncBlk { LNp n1, n2; Lin qkv, proj, fc1, fc2; };
struct DecBlk { LNp n1, n2, n3, ny; Lin qkv, proj, cq, ckv, cproj, fc1, fc2; };
struct ConvW { void* w = nullptr; float* b = nullptr; int Cout = 0, Cin = 0, cin_pad = 0, k = 1, n_pad = 0, n_rows = 0, K = 0; };
struct Refine { ConvW r1c1, r1c2, r2c1, r2c2; Lin outc; };
struct DptHead {
    Lin act1x1[4];
    Lin convt[2];      // ConvTranspose k=4 / k=2 as GEMM; N = k*k*cout_pad
    int convt_k[2] = {4, 2}, convt_coutp[2] = {0, 0};
    ConvW act3conv;    // Conv2d(768,768,3,s2,p1)
    ConvW layer_rn[4];
    Refine rn[4];      // rn[0] = refinenet1 ... rn[3] = refinenet4
    ConvW head0, head2;
    float* head4_w = nullptr; float* head4_b = nullptr;
    int cstride[4] = {0, 0, 0, 0};  // channel stride of the 4 reassembled maps
};

}  // namespace

// The engines of a process share their helper streams (per device and role; never destroyed). A HIP stream is bound to one of a few hardware queues (4 by default,
// GPU_MAX_HW_QUEUES) in creation order: with a stream per engine, the n-th engine of a process could find its second stream on the caller's own hardware queue -- the
// two decoder sides then run one after the other (measured on MI355X: the THIRD engine created in a process took 13.1 ms per one-pair call against 10.1 ms for the
// first, second and fourth; profiles/r05_y/ln_inline3.log). One process-wide stream per role keeps every engine on the placement the first one got. Stream order only
// adds dependencies; what it costs: engines on one device are NOT independent any more -- their side-stream halves serialise, and the enqueue of a forward is a
// process-wide critical section (run_phases: a capture of one engine must not see another engine's launches). Documented in include/dust3r_hip.h (d3r_model_create).
static hipStream_t shared_stream(int role) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, hipStream_t> pool;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    auto it = pool.find({dev, role});
    if (it != pool.end()) return it->second;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    pool[{dev, role}] = s;
    return s;
}

struct d3r_model {
    d3r_model_config cfg;
    int dt = 0, ktile = 64;
    int bdt = 0;              // operand layout of the transformer blocks' linears (= dt, or D3R_F16F8 on top of dt = D3R_F16X3)
    // LayerNorm folded into the GEMMs around it (round 5; split-fp16 engines; kernels.hpp GemmParams::ln_*): norm1 / norm2 of the encoder blocks
    // and norm1 / norm2 / norm3 / norm_y of the decoder blocks are not launched -- the fp32-residual epilogue in front of them also stores the RAW
    // typed rows and per-row partial sums, the nn.Linear behind them is packed as W diag(gamma) and applies rstd / mean in its epilogue.
    // enc_norm / dec_norm (their outputs leave the engine or feed the heads) stay kernels. D3R_LN_FOLD=0|1 at model creation.
    int ln_inline_rows = 3072; // folded LayerNorms of at most this many rows (calls of one or two pairs; the decoder sides of four) get their statistics in the consumer GEMM's prologue
                              // (GemmParams::ln_part_in; kernels.hpp ln_row_stats = ln_finalize_kernel's arithmetic with four adjacent lanes per row) instead of by an ln_finalize
                              // launch: bit-identical, one pair 10.32 -> 10.10 ms, two 15.27 -> 15.09, four and eight equal (profiles/r05_y/ln_inline3.log; the first version, 32
                              // lanes per row with five fp64 exchange levels in front of every tile, was SLOWER: r05_v). D3R_LN_INLINE_ROWS=n at creation; 0 = always launch.
    bool ln_fold = false, fold_dirty = false;
    std::vector<Lin*> fold_lins;
    std::unordered_map<std::string, Slot> slots;
    std::vector<void*> allocs;
    size_t weight_bytes = 0;
    Lin patch;
    std::vector<EncBlk> enc;
    LNp enc_norm, dec_norm;
    Lin dec_embed;
    std::vector<DecBlk> dec[2];
    DptHead dpt[2];
    Lin lin_head[2];
    float* rope_table = nullptr;
    void* zero_page = nullptr;
    // split-K of the small-batch forwards (kernels.hpp GemmParams::splitk): partial-tile slabs and arrival counters, one set per stream of the forward (main, side)
    static constexpr size_t SK_SLAB_FLOATS = (size_t)8 << 20; static constexpr int SK_CNT = 1024;
    float* sk_slab[2] = {nullptr, nullptr}; unsigned* sk_cnt[2] = {nullptr, nullptr};
    bool splitk_on = true;       // D3R_SPLITK=0 at creation: never (every launch then sums K in one block: a batch is bit-identical to its one-pair calls)
    void* ws = nullptr; size_t ws_bytes = 0;
    void* stage = nullptr; size_t stage_bytes = 0;   // load-time staging of host tensors
    // the two decoder sides (and the two heads) are independent inside a layer: side 1 runs on this second stream
    hipStream_t side = nullptr;
    hipEvent_t ev_main = nullptr, ev_side = nullptr;
    bool two_streams = true;
    PostMode post;                          // depth_mode / conf_mode of the heads (d3r_model_set_postprocess; default = the released checkpoints')
    // ---- hipGraph replay of small-batch forwards (d3r_model_forward* with B <= graph_max_pairs) ------------------------------------
    // One pair per call (dust3r/demo.py:156 batch_size=1, visloc.py:88) is ~700 launches of kernels that each fill a fraction of the
    // chip: the host-side enqueue and the two-stream event traffic, not the GPU, set the pace. The second call with the same
    // (entry point, B, image sizes, output layout, stream plan) is stream-captured on an engine-owned stream into a graph that works on
    // engine-owned input / output staging buffers; every later call is [copy inputs -> staging] + hipGraphLaunch + [copy staging ->
    // outputs] on the caller's stream. Same kernels, same order: bit-identical to the eager call.
    struct GraphKey {
        int B, H1, W1, H2, W2, pstride, two;
        bool operator==(const GraphKey& o) const { return B == o.B && H1 == o.H1 && W1 == o.W1 && H2 == o.H2 && W2 == o.W2 && pstride == o.pstride && two == o.two; }
    };
    struct GraphEntry { GraphKey key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; int seen = 0; float* io = nullptr; size_t io_bytes = 0; };
    std::vector<GraphEntry> graphs;
    hipStream_t cap = nullptr;              // capture origin (the legacy default stream cannot be captured)
    int graph_max_pairs = 0;                // D3R_MODEL_OPT_GRAPH_MAX_PAIRS; 0 = off (default: measured no latency gain on MI355X, see the header)
    long graph_replays = 0;                 // statistics (tests)
    void drop_graphs() {
        for (auto& g : graphs) {
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
            if (g.graph) (void)hipGraphDestroy(g.graph);
            if (g.io) (void)hipFree(g.io);
        }
        graphs.clear();
    }
    // last forward (debug hook)
    const void* last_encn = nullptr; size_t last_encn_elems = 0;
    // optional per-launch HIP-event timing (d3r_model_set_option(D3R_MODEL_OPT_PROFILE)); off in timed runs
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;
    struct ProfRec { int kind; double work; int M, N, K; };
    std::vector<ProfRec> prof_rec;

    void* dalloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
        (void)hipMemset(p, 0, bytes ? bytes : 16);
        allocs.push_back(p);
        weight_bytes += bytes;
        return p;
    }
};

namespace {

// ---- slot registration ---------------------------------------------------------------------------------
bool reg_vec(d3r_model* m, const std::string& key, float** dst, int n, int n_alloc = 0) {
    if (!*dst) {
        *dst = (float*)m->dalloc((size_t)(n_alloc ? n_alloc : n) * sizeof(float));
        if (!*dst) return false;
    }
    Slot s; s.kind = PK_VEC; s.dst = *dst; s.rows = n;
    m->slots[key] = s;
    return true;
}
bool reg_vec_at(d3r_model* m, const std::string& key, float* base, int off, int n) {
    Slot s; s.kind = PK_VEC; s.dst = base + off; s.rows = n;
    m->slots[key] = s;
    return true;
}
bool alloc_lin(d3r_model* m, Lin& L, int N, int K, bool bias = true, int dt = -1) {
    L.N = N; L.K = K; L.n_pad = gemm_n_pad(N); L.n_rows = gemm_n_rows(N);
    L.dt = dt < 0 ? m->dt : dt;
    L.w = m->dalloc((size_t)L.n_rows * K * wgt_bytes(L.dt));      // 2.5-unit rows: five bytes per element
    L.b = bias ? (float*)m->dalloc((size_t)L.n_rows * sizeof(float)) : nullptr;
    return L.w && (!bias || L.b);
}
void reg_mat(d3r_model* m, const std::string& key, const Lin& L, int rows, int row_off) {
    Slot s; s.kind = PK_MAT; s.dst = L.w; s.rows = rows; s.cols = L.K; s.row_off = row_off; s.dst_cols = L.K; s.dt = L.dt;
    m->slots[key] = s;
}
bool reg_linear(d3r_model* m, const std::string& prefix, Lin& L, int N, int K, int dt = -1) {
    if (!alloc_lin(m, L, N, K, true, dt)) return false;
    reg_mat(m, prefix + ".weight", L, N, 0);
    reg_vec_at(m, prefix + ".bias", L.b, 0, N);
    return true;
}
bool reg_ln(d3r_model* m, const std::string& prefix, LNp& p, int C) {
    return reg_vec(m, prefix + ".weight", &p.g, C) && reg_vec(m, prefix + ".bias", &p.b, C);
}
bool reg_conv(d3r_model* m, const std::string& prefix, ConvW& c, int Cout, int Cin, int k, bool bias) {
    c.Cout = Cout; c.Cin = Cin; c.k = k; c.cin_pad = rup(Cin, m->ktile); c.n_pad = gemm_n_pad(Cout); c.n_rows = gemm_n_rows(Cout); c.K = k * k * c.cin_pad;
    c.w = m->dalloc((size_t)c.n_rows * c.K * dt_bytes(m->dt));
    if (!c.w) return false;
    Slot s; s.kind = PK_CONV; s.dst = c.w; s.rows = Cout; s.cin = Cin; s.cin_pad = c.cin_pad; s.ksize = k; s.dst_cols = c.K;
    m->slots[prefix + ".weight"] = s;
    if (bias) {
        c.b = (float*)m->dalloc((size_t)c.n_rows * sizeof(float));
        if (!c.b) return false;
        reg_vec_at(m, prefix + ".bias", c.b, 0, Cout);
    }
    return true;
}
bool reg_convt(d3r_model* m, const std::string& prefix, Lin& L, int Cin, int Cout, int k, int cin_pad, int cout_pad) {
    L.N = k * k * cout_pad; L.K = cin_pad; L.n_pad = gemm_n_pad(L.N); L.n_rows = gemm_n_rows(L.N); L.dt = m->dt;
    L.w = m->dalloc((size_t)L.n_rows * L.K * dt_bytes(m->dt));
    L.b = (float*)m->dalloc((size_t)L.n_rows * sizeof(float));
    if (!L.w || !L.b) return false;
    Slot s; s.kind = PK_CONVT; s.dst = L.w; s.rows = Cin; s.cols = Cout; s.ksize = k; s.cin_pad = cin_pad; s.cout_pad = cout_pad; s.dst_cols = L.K;
    m->slots[prefix + ".weight"] = s;
    Slot b; b.kind = PK_CONVT_BIAS; b.dst = L.b; b.rows = Cout; b.ksize = k; b.cout_pad = cout_pad;
    m->slots[prefix + ".bias"] = b;
    return true;
}
// the nn.Linear `L` (weight slots `wkeys`, bias slots `bkeys`) consumes LayerNorm `ln` (slots prefix `lnkey`): fold it (ln_fold engines)
bool reg_fold(d3r_model* m, Lin& L, const LNp& ln, const std::string& lnkey, std::initializer_list<std::string> wkeys, std::initializer_list<std::string> bkeys) {
    if (!m->ln_fold) return true;
    L.ln = &ln;
    L.ln_s = (float*)m->dalloc((size_t)L.n_rows * sizeof(float));
    L.b_fold = (float*)m->dalloc((size_t)L.n_rows * sizeof(float));
    if (!L.ln_s || !L.b_fold) return false;
    unsigned bit = 1;
    for (auto& k : wkeys) { m->slots[k].fold = &L; m->slots[k].fold_bit = bit; L.want_mask |= bit; bit <<= 1; }
    for (auto& k : bkeys) { m->slots[k].refold = true; m->slots[k].refold_lins.push_back(&L); }
    for (const char* sfx : {".weight", ".bias"}) { Slot& ls = m->slots[lnkey + sfx]; ls.refold = true; ls.refold_lins.push_back(&L); }
    m->fold_lins.push_back(&L);
    return true;
}
void reg_ignore(d3r_model* m, const std::string& key) { Slot s; s.kind = PK_IGNORE; s.loaded = true; m->slots[key] = s; }

bool build_slots(d3r_model* m) {
    const d3r_model_config& c = m->cfg;
    const int Ce = c.enc_embed_dim, Cd = c.dec_embed_dim, ps = c.patch_size;
    const int bd = m->bdt;    // the 24 + 2 x 12 transformer blocks' matrices; patch embedding, decoder_embed and the heads keep m->dt
    if (!reg_linear(m, "patch_embed.proj", m->patch, Ce, 3 * ps * ps)) return false;
    reg_ignore(m, "mask_token");
    m->enc.resize(c.enc_depth);
    for (int l = 0; l < c.enc_depth; ++l) {
        const std::string p = "enc_blocks." + std::to_string(l);
        EncBlk& b = m->enc[l];
        if (!reg_ln(m, p + ".norm1", b.n1, Ce) || !reg_ln(m, p + ".norm2", b.n2, Ce) || !reg_linear(m, p + ".attn.qkv", b.qkv, 3 * Ce, Ce, bd) ||
            !reg_linear(m, p + ".attn.proj", b.proj, Ce, Ce, bd) || !reg_linear(m, p + ".mlp.fc1", b.fc1, 4 * Ce, Ce, bd) ||
            !reg_linear(m, p + ".mlp.fc2", b.fc2, Ce, 4 * Ce, bd))
            return false;
        if (!reg_fold(m, b.qkv, b.n1, p + ".norm1", {p + ".attn.qkv.weight"}, {p + ".attn.qkv.bias"}) ||
            !reg_fold(m, b.fc1, b.n2, p + ".norm2", {p + ".mlp.fc1.weight"}, {p + ".mlp.fc1.bias"}))
            return false;
    }
    if (!reg_ln(m, "enc_norm", m->enc_norm, Ce) || !reg_ln(m, "dec_norm", m->dec_norm, Cd) || !reg_linear(m, "decoder_embed", m->dec_embed, Cd, Ce))
        return false;
    for (int side = 0; side < 2; ++side) {
        m->dec[side].resize(c.dec_depth);
        for (int l = 0; l < c.dec_depth; ++l) {
            const std::string p = std::string(side ? "dec_blocks2." : "dec_blocks.") + std::to_string(l);
            DecBlk& b = m->dec[side][l];
            if (!reg_ln(m, p + ".norm1", b.n1, Cd) || !reg_ln(m, p + ".norm2", b.n2, Cd) || !reg_ln(m, p + ".norm3", b.n3, Cd) ||
                !reg_ln(m, p + ".norm_y", b.ny, Cd) || !reg_linear(m, p + ".attn.qkv", b.qkv, 3 * Cd, Cd, bd) ||
                !reg_linear(m, p + ".attn.proj", b.proj, Cd, Cd, bd) || !reg_linear(m, p + ".cross_attn.projq", b.cq, Cd, Cd, bd) ||
                !reg_linear(m, p + ".cross_attn.proj", b.cproj, Cd, Cd, bd) || !reg_linear(m, p + ".mlp.fc1", b.fc1, 4 * Cd, Cd, bd) ||
                !reg_linear(m, p + ".mlp.fc2", b.fc2, Cd, 4 * Cd, bd))
                return false;
            // projk and projv share their input: packed as one (2 Cd, Cd) matrix
            if (!alloc_lin(m, b.ckv, 2 * Cd, Cd, true, bd)) return false;
            reg_mat(m, p + ".cross_attn.projk.weight", b.ckv, Cd, 0);
            reg_mat(m, p + ".cross_attn.projv.weight", b.ckv, Cd, Cd);
            reg_vec_at(m, p + ".cross_attn.projk.bias", b.ckv.b, 0, Cd);
            reg_vec_at(m, p + ".cross_attn.projv.bias", b.ckv.b, Cd, Cd);
            if (!reg_fold(m, b.qkv, b.n1, p + ".norm1", {p + ".attn.qkv.weight"}, {p + ".attn.qkv.bias"}) ||
                !reg_fold(m, b.cq, b.n2, p + ".norm2", {p + ".cross_attn.projq.weight"}, {p + ".cross_attn.projq.bias"}) ||
                !reg_fold(m, b.ckv, b.ny, p + ".norm_y", {p + ".cross_attn.projk.weight", p + ".cross_attn.projv.weight"}, {p + ".cross_attn.projk.bias", p + ".cross_attn.projv.bias"}) ||
                !reg_fold(m, b.fc1, b.n3, p + ".norm3", {p + ".mlp.fc1.weight"}, {p + ".mlp.fc1.bias"}))
                return false;
        }
    }
    // dec_blocks.* duplicates into dec_blocks2.* until an explicit dec_blocks2 key arrives (model.py:91-98)
    {
        std::vector<std::string> keys;
        for (auto& kv : m->slots)
            if (kv.first.rfind("dec_blocks.", 0) == 0) keys.push_back(kv.first);
        for (auto& k : keys) m->slots[k].mirror = "dec_blocks2." + k.substr(strlen("dec_blocks."));
    }
    for (int hd = 0; hd < 2; ++hd) {
        const std::string hp = "downstream_head" + std::to_string(hd + 1);
        if (c.head_type == 0) {
            if (!reg_linear(m, hp + ".proj", m->lin_head[hd], 4 * ps * ps, Cd)) return false;
            continue;
        }
        DptHead& D = m->dpt[hd];
        const std::string dp = hp + ".dpt";
        const int ld[4] = {96, 192, 384, 768};
        const int din[4] = {Ce, Cd, Cd, Cd};
        for (int i = 0; i < 4; ++i) {
            D.cstride[i] = rup(ld[i], m->ktile);
            if (!alloc_lin(m, D.act1x1[i], ld[i], din[i])) return false;
            reg_mat(m, dp + ".act_postprocess." + std::to_string(i) + ".0.weight", D.act1x1[i], ld[i], 0);
            reg_vec_at(m, dp + ".act_postprocess." + std::to_string(i) + ".0.bias", D.act1x1[i].b, 0, ld[i]);
        }
        D.convt_coutp[0] = D.cstride[0]; D.convt_coutp[1] = D.cstride[1];
        if (!reg_convt(m, dp + ".act_postprocess.0.1", D.convt[0], ld[0], ld[0], 4, D.cstride[0], D.cstride[0])) return false;
        if (!reg_convt(m, dp + ".act_postprocess.1.1", D.convt[1], ld[1], ld[1], 2, D.cstride[1], D.cstride[1])) return false;
        if (!reg_conv(m, dp + ".act_postprocess.3.1", D.act3conv, ld[3], ld[3], 3, true)) return false;
        for (int i = 0; i < 4; ++i) {
            if (!reg_conv(m, dp + ".scratch.layer_rn." + std::to_string(i), D.layer_rn[i], 256, ld[i], 3, false)) return false;
            reg_ignore(m, dp + ".scratch.layer" + std::to_string(i + 1) + "_rn.weight");  // alias of layer_rn.i
            const std::string rp = dp + ".scratch.refinenet" + std::to_string(i + 1);
            Refine& R = D.rn[i];
            if (!reg_conv(m, rp + ".resConfUnit1.conv1", R.r1c1, 256, 256, 3, true) || !reg_conv(m, rp + ".resConfUnit1.conv2", R.r1c2, 256, 256, 3, true) ||
                !reg_conv(m, rp + ".resConfUnit2.conv1", R.r2c1, 256, 256, 3, true) || !reg_conv(m, rp + ".resConfUnit2.conv2", R.r2c2, 256, 256, 3, true))
                return false;
            if (!alloc_lin(m, R.outc, 256, 256)) return false;
            reg_mat(m, rp + ".out_conv.weight", R.outc, 256, 0);
            reg_vec_at(m, rp + ".out_conv.bias", R.outc.b, 0, 256);
        }
        // refinenet4.resConfUnit1 exists in the checkpoint but is never evaluated (single input): still required keys
        if (!reg_conv(m, dp + ".head.0", D.head0, 128, 256, 3, true) || !reg_conv(m, dp + ".head.2", D.head2, 128, 128, 3, true)) return false;
        if (!reg_vec(m, dp + ".head.4.weight", &D.head4_w, 4 * 128) || !reg_vec(m, dp + ".head.4.bias", &D.head4_b, 4)) return false;
    }
    return true;
}

// `data` is a DEVICE fp32 tensor in the checkpoint's (PyTorch) layout; the conversion to the engine's dtype and
// layout runs on the GPU (elementwise.hip: pack_weight_kernel), ordered on the default stream.
int pack_slot(d3r_model* m, Slot& s, const float* data, int ndim, const int64_t* shape) {
    size_t numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
    PackParams pp;
    pp.src = data; pp.numel = numel; pp.dst = s.dst; pp.dst_cols = s.dst_cols;
    switch (s.kind) {
        case PK_IGNORE: return D3R_OK;
        case PK_VEC:
            if (numel != (size_t)s.rows) return D3R_ERR_SHAPE;
            if (s.refold) { m->fold_dirty = true; for (Lin* L : s.refold_lins) L->fold_dirty = true; }
            return hipMemcpyAsync(s.dst, data, numel * sizeof(float), hipMemcpyDeviceToDevice, nullptr) == hipSuccess ? D3R_OK : D3R_ERR_ALLOC;
        case PK_MAT:
            if (ndim < 2 || shape[0] != s.rows || numel != (size_t)s.rows * s.cols) return D3R_ERR_SHAPE;
            pp.kind = PACK_MAT; pp.cols = s.cols; pp.row_off = s.row_off;
            if (s.fold) {       // the LayerNorm in front of this matrix is folded into it: keep the fp32 rows until finalize_fold packs W diag(gamma)
                Lin& L = *s.fold;
                if (!L.w32) {
                    if (hipMalloc((void**)&L.w32, (size_t)L.N * L.K * sizeof(float)) != hipSuccess) { L.w32 = nullptr; return D3R_ERR_ALLOC; }
                    L.have_mask = 0;            // a fresh staging copy holds nothing yet
                }
                L.have_mask |= s.fold_bit;
                L.fold_dirty = true;
                m->fold_dirty = true;
                return hipMemcpyAsync(L.w32 + (size_t)s.row_off * L.K, data, numel * sizeof(float), hipMemcpyDeviceToDevice, nullptr) == hipSuccess ? D3R_OK : D3R_ERR_ALLOC;
            }
            break;
        case PK_CONV:
            if (ndim != 4 || shape[0] != s.rows || shape[1] != s.cin || shape[2] != s.ksize || shape[3] != s.ksize) return D3R_ERR_SHAPE;
            pp = conv_pack_params(data, s.dst, false, s.rows, s.cin, s.ksize, s.cin_pad, 0);
            break;
        case PK_CONVT:
            if (ndim != 4 || shape[0] != s.rows || shape[1] != s.cols || shape[2] != s.ksize || shape[3] != s.ksize) return D3R_ERR_SHAPE;
            pp = conv_pack_params(data, s.dst, true, s.cols, s.rows, s.ksize, s.cin_pad, s.cout_pad);
            break;
        case PK_CONVT_BIAS:
            if (numel != (size_t)s.rows) return D3R_ERR_SHAPE;
            return launch_pack_convt_bias(data, (float*)s.dst, s.rows, s.cout_pad, s.ksize * s.ksize, nullptr) == hipSuccess ? D3R_OK : D3R_ERR_LAUNCH;
    }
    return launch_pack_weight(s.dt < 0 ? m->dt : s.dt, pp, nullptr) == hipSuccess ? D3R_OK : D3R_ERR_LAUNCH;
}

// ---- launch helpers ------------------------------------------------------------------------------------------
struct Ctx {
    d3r_model* m;
    hipStream_t st;
    int rc = D3R_OK;
    hipStream_t st0 = nullptr;    // the caller's stream (st moves between it and the engine's helper streams)
    void chk(hipError_t e) { if (e != hipSuccess && rc == D3R_OK) rc = 1000 + (int)e; }
    // profiling: one event BEFORE every launch; a launch's duration is event[i+1] - event[i]
    void mark(int kind, double work, int M = 0, int N = 0, int K = 0) {
        if (!m->prof_on) return;
        const size_t i = m->prof_rec.size();
        if (i >= m->prof_ev.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            m->prof_ev.push_back(e);
        }
        (void)hipEventRecord(m->prof_ev[i], st);
        m->prof_rec.push_back({kind, work, M, N, K});
    }
};
// profile record kinds: GEMM-kernel launches carry their tile configuration: kind = cfg (0..7) + 8 for implicit-GEMM convolution
enum { PRF_GEMM = 0, PRF_CONV = 8, PRF_ATTN = 16, PRF_OTHER = 17, PRF_GEMM_64 = 18, PRF_CONV_64 = 19, PRF_END = 20, PRF_GEMM_384 = 21, PRF_GEMM_P4 = 22, PRF_GEMM_F8 = 24 };   // 24..31: fp16 + fp8 linear launches by tile configuration
// tile configuration 8 (the 64 x 64 tile of the small-batch forwards, split-fp16 only) has its own two kinds behind the 0..7 ranges
static inline int prf_kind(int base, int cfg) { return cfg == GEMM_CFG_P4 ? PRF_GEMM_P4 : cfg == GEMM_CFG_384x192 ? PRF_GEMM_384 : (cfg == GEMM_CFG_64 || cfg == GEMM_CFG_96x64) ? (base == PRF_CONV ? PRF_CONV_64 : PRF_GEMM_64) : base + cfg; }
#define D3R_OTHER(call) do { c.mark(PRF_OTHER, 0.0); c.chk(call); } while (0)

// The two views of a pair may have different sizes (dust3r/model.py:148-150: the reference then encodes them separately): every
// per-side quantity of the decoder / heads is indexed by side -- token grid (th, tw), tokens per image N, rows M = B N, V^T row
// stride -- and cross attention runs Nq != Nk. With equal sizes this is the old schedule bit for bit.
struct SideDim { int H, W, th, tw, N, ldv; };
SideDim side_dim(int H, int W, int ps) {
    SideDim d;
    d.H = H; d.W = W; d.th = H / ps; d.tw = W / ps; d.N = d.th * d.tw; d.ldv = rup(d.N, 64);
    return d;
}

// folded LayerNorm (kernels.hpp GemmParams::ln_*): `stats` = the consumer side (rstd, -mean rstd of the input rows; the Lin carries column sums and
// folded bias), GemmParams::ln_part = the producer side (partial sums of the rows this launch stores, next to their raw typed copy out2)
struct LnStats { const float* rstd = nullptr; const float* nmr = nullptr; const float* part_in = nullptr; };   // part_in: small problem, the consumer forms rstd / nmr itself (no ln_finalize launch)

// EVERY GEMM-kernel launch of the forward: lend the split-K buffers, plan, mark the profile with the plan's tile and the logical problem (M, N, K), launch that plan.
// lend_sk: the buffers of this launch's stream go with it and gemm_plan decides whether it splits (never while profiling: one event per launch). Only gemm_linear lends
// them: gemm_plan would split an attention-projection launch too. planned: the caller's own plan (conv_head4).
void launch(Ctx& c, int dt, GemmParams& p, int base, int N, int K, bool lend_sk = false, const GemmPlan* planned = nullptr) {
    const int sset = c.st == c.st0 ? 0 : (c.st == c.m->side ? 1 : -1);
    if (lend_sk && c.m->splitk_on && sset >= 0 && c.m->sk_slab[sset] && !c.m->prof_on) {
        p.splitk = 0; p.sk_slab = c.m->sk_slab[sset]; p.sk_cnt = c.m->sk_cnt[sset]; p.sk_slab_floats = d3r_model::SK_SLAB_FLOATS; p.sk_cnt_n = d3r_model::SK_CNT;
    }
    const GemmPlan plan = planned ? *planned : gemm_plan_for(p, dt);
    if (base == PRF_GEMM && (dt == D3R_F16F8 || dt == D3R_F16X2F8)) base = PRF_GEMM_F8;
    c.mark(prf_kind(base, plan.cfg), 2.0 * p.M * (double)N * K, p.M, N, K);
    c.chk(launch_gemm(dt, p, plan, c.st));
}

// operands of the nn.Linear `L` on M rows of `act`, with the statistics of a folded LayerNorm in front of it; the caller names epilogue, outputs, residual and flags
GemmParams lin_params(const Lin& L, const void* act, int lda, int M, const LnStats& stats = LnStats()) {
    GemmParams p = linear_gemm_params(act, lda, L.w, L.b, M, L.N, L.K);
    if (stats.rstd) { p.bias = L.b_fold; ln_consumer(p, stats.rstd, stats.nmr, L.ln_s, stats.part_in, 1e-6f); }
    return p;
}
void gemm_linear(Ctx& c, const Lin& L, GemmParams& p) {
    p.ldr = p.ldo;      // residual rows have the output's stride
    launch(c, L.dt, p, PRF_GEMM, L.N, L.K, true);
}

// the input rows of an nn.Linear behind a LayerNorm: normalised rows, or (folded) the raw rows with their statistics -- norm_in() below
struct NormIn { const void* rows; LnStats stats; };
// q | k | v projection (EPI_HEADS): up to three regions of C columns each, stored per head in the attention kernel's layouts for the token grid `d`
struct Region { int kind = 0; void* dst = nullptr; };
void gemm_heads(Ctx& c, const Lin& L, const NormIn& in, int M, int C, int heads, const SideDim& d, Region r0, Region r1 = Region(), Region r2 = Region()) {
    GemmParams p = lin_params(L, in.rows, C, M, in.stats);
    const int kinds[3] = {r0.kind, r1.kind, r2.kind};
    void* const dsts[3] = {r0.dst, r1.dst, r2.dst};
    epi_heads(p, C, 3, kinds, dsts, heads, d.N, d.tw, d.ldv, c.m->rope_table);
    // q | k | v whose q | k prefix the plan puts on the persistent kernel (gemm_p4.hip: its drain rotates, it has no V^T): two launches on the same rows and statistics,
    // q | k there and V -- weight rows, bias and column sums from row 2 C on -- where a [vt] launch goes. Every element is computed as in the single launch.
    if (r0.kind == HEAD_ROPE && r1.kind == HEAD_ROPE && r2.kind == HEAD_VT && L.N == 3 * C && L.dt == D3R_F16X3) {
        GemmParams qk = p;
        qk.n_store = qk.n_pad = 2 * C; qk.head_kind[2] = 0; qk.head_dst[2] = nullptr;
        const GemmPlan plan = gemm_plan_for(qk, L.dt);
        if (plan.cfg == GEMM_CFG_P4) {        // (C % 128 == 0 there)
            launch(c, L.dt, qk, PRF_GEMM, 2 * C, L.K, false, &plan);
            GemmParams v = p;
            v.wgt = reinterpret_cast<const char*>(p.wgt) + (size_t)2 * C * L.K * dt_bytes(L.dt);
            if (v.bias) v.bias += 2 * C;
            if (v.ln_colsum) v.ln_colsum += 2 * C;
            v.n_store = v.n_pad = C; v.n_rows = p.n_rows - 2 * C;
            v.head_kind[0] = HEAD_VT; v.head_dst[0] = r2.dst;
            for (int i = 1; i < 3; ++i) { v.head_kind[i] = 0; v.head_dst[i] = nullptr; }
            launch(c, L.dt, v, PRF_GEMM, C, L.K);
            return;
        }
    }
    launch(c, L.dt, p, PRF_GEMM, L.N, L.K);
}

void conv(Ctx& c, const void* in, int B, int Hin, int Win, int cstride, const ConvW& w, int stride, int pad, void* out, int ldo,
          int flags, const void* res1 = nullptr, const void* res2 = nullptr, void* out2 = nullptr) {
    GemmParams p = conv_gemm_params(in, B, Hin, Win, cstride, w.w, w.b, w.cin_pad, w.Cout, w.k, stride, pad, c.m->zero_page);   // K, n_pad, n_rows: reg_conv's
    epi_typed_store(p, out, ldo, flags, res1, res2, out2);
    launch(c, c.m->dt, p, PRF_CONV, w.Cout, w.k * w.k * w.Cin);
}

// 3x3 convolution (stride 1, pad 1) + ReLU + Conv2d(Cout, 4, 1) + postprocess in one launch (EPI_HEAD4); false (nothing launched) when
// the problem does not get a tile shape whose waves hold all output channels
bool conv_head4(Ctx& c, const void* in, int B, int Hin, int Win, int cstride, const ConvW& w, const float* w4, const float* b4,
                float* pts, float* conf, int pstride, int cstride_conf) {
    GemmParams p = conv_gemm_params(in, B, Hin, Win, cstride, w.w, w.b, w.cin_pad, w.Cout, w.k, 1, 1, c.m->zero_page);
    epi_head_tail(p, w4, b4, pts, pstride, conf, cstride_conf, c.m->post);
    GemmPlan plan;
    if (!head4_tile(p, c.m->dt, plan)) return false;      // 512 x 128, else the forced 256 x 128 R (kernels.hpp)
    launch(c, c.m->dt, p, PRF_CONV, w.Cout, w.k * w.k * w.Cin, false, &plan);
    return true;
}

// The same launch reading the x2 bilinear map of `src` (B, Hi, Wi) without the map in memory (AMODE_CONV_UP2, gemm_up2.hip). up2_head4_params with null
// operands is what head_upfused asks the plan about: the layout (which then takes no map from the arena) and the launch decide by the same predicate.
GemmParams up2_head4_params(const d3r_model* m, const void* src, int B, int Hi, int Wi, int cstride, const ConvW& w, const float* w4, const float* b4,
                            float* pts, float* conf, int pstride, int cstride_conf) {
    GemmParams p = conv_up2_gemm_params(src, B, Hi, Wi, cstride, w.w, w.b, w.cin_pad, w.Cout, m->zero_page);
    epi_head_tail(p, w4, b4, pts, pstride, conf, cstride_conf, m->post);
    return p;
}
// The typed-store form (head.0 on the x2 map of refinenet-0's output): conv() without residuals
GemmParams up2_conv_params(const d3r_model* m, const void* src, int B, int Hi, int Wi, int cstride, const ConvW& w, void* out, int ldo, int flags) {
    GemmParams p = conv_up2_gemm_params(src, B, Hi, Wi, cstride, w.w, w.b, w.cin_pad, w.Cout, m->zero_page);
    epi_typed_store(p, out, ldo, flags);
    return p;
}
// The head's tail (1x1 convolution + postprocess) runs in the epilogue of the last 3x3 convolution: split-fp16 engines. D3R_HEAD_FUSE=0: the two-kernel route (test A/B)
bool head_fuse_on(const d3r_model* m) {
    const char* e = getenv("D3R_HEAD_FUSE");
    return m->dt == D3R_F16X3 && !(e && e[0] == '0');
}
// Which of the head's two x2 maps are interpolated inside the convolution that reads them. D3R_HEAD_UPFUSE=0: neither (the two-kernel routes: test A/B);
// the last convolution's route also needs its fused tail (head_fuse_on).
bool up2_switch_on(const d3r_model* m) {
    const char* u = getenv("D3R_HEAD_UPFUSE");
    return m->dt == D3R_F16X3 && !(u && u[0] == '0');
}
bool head_upfused(const d3r_model* m, const ConvW& w, int B, int Hi, int Wi, int cstride) {      // head.2 + tail on the x2 map of head.0's output
    if (!up2_switch_on(m) || w.k != 3 || !head_fuse_on(m)) return false;
    return gemm_plan_for(up2_head4_params(m, nullptr, B, Hi, Wi, cstride, w, nullptr, nullptr, nullptr, nullptr, 3, 1), m->dt).up2;
}
bool head0_upfused(const d3r_model* m, const ConvW& w, int B, int Hi, int Wi, int cstride, int ldo) {      // head.0 on the x2 map of refinenet-0's output
    if (!up2_switch_on(m) || w.k != 3) return false;
    return gemm_plan_for(up2_conv_params(m, nullptr, B, Hi, Wi, cstride, w, nullptr, ldo, 0), m->dt).up2;
}
void conv_up2(Ctx& c, const void* src, int B, int Hi, int Wi, int cstride, const ConvW& w, void* out, int ldo, int flags) {
    GemmParams p = up2_conv_params(c.m, src, B, Hi, Wi, cstride, w, out, ldo, flags);
    const GemmPlan plan = gemm_plan_for(p, c.m->dt);
    launch(c, c.m->dt, p, PRF_CONV, w.Cout, w.k * w.k * w.Cin, false, &plan);
}
void conv_up2_head4(Ctx& c, const void* src, int B, int Hi, int Wi, int cstride, const ConvW& w, const float* w4, const float* b4,
                    float* pts, float* conf, int pstride, int cstride_conf) {
    GemmParams p = up2_head4_params(c.m, src, B, Hi, Wi, cstride, w, w4, b4, pts, conf, pstride, cstride_conf);
    const GemmPlan plan = gemm_plan_for(p, c.m->dt);
    launch(c, c.m->dt, p, PRF_CONV, w.Cout, w.k * w.k * w.Cin, false, &plan);
}

struct Arena {
    char* base; size_t off = 0, cap;
    Arena(void* b, size_t c) : base((char*)b), cap(c) {}
    void* take(size_t bytes) {
        off = (off + 255) & ~(size_t)255;
        void* p = base ? base + off : nullptr;
        off += bytes;
        return p;
    }
};

}  // namespace

// =========================================================================================================
extern "C" const char* d3r_version(void) { return "dust3r_amd 0.1 (gfx950)"; }

extern "C" int d3r_device_check(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return D3R_ERR_STATE;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return D3R_ERR_STATE;     // the CURRENT device is the one the engine will run on
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return D3R_ERR_STATE;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? D3R_OK : D3R_ERR_STATE;
}

extern "C" int d3r_model_create(d3r_model** out, const d3r_model_config* cfg) {
    if (!out || !cfg) return D3R_ERR_INVALID;
    if (cfg->dtype < 0 || cfg->dtype > D3R_F16X2F8 || cfg->patch_size % 4 != 0) return D3R_ERR_INVALID;
    if (cfg->dtype == D3R_F16X2F8 && (cfg->enc_embed_dim % 128 || cfg->dec_embed_dim % 128)) return D3R_ERR_INVALID;   // whole 128-k blocks of five weight chunks
    if (cfg->enc_embed_dim != cfg->enc_num_heads * 64 || cfg->dec_embed_dim != cfg->dec_num_heads * 64) return D3R_ERR_INVALID;  // head dim 64
    d3r_model* m = new (std::nothrow) d3r_model();
    if (!m) return D3R_ERR_ALLOC;
    // D3R_DTYPE_F16F8: the transformer blocks' linears on fp16 + fp8 operand rows, everything else (patch embedding, decoder_embed,
    // attention operands, DPT / linear heads) in split-fp16
    // D3R_DTYPE_F16X2F8: the same split of the network, the blocks' linears on the 2.5-unit arithmetic (activation rows as above, five-chunk weight rows)
    const bool f8blocks = cfg->dtype == D3R_F16F8 || cfg->dtype == D3R_F16X2F8;
    m->cfg = *cfg; m->dt = f8blocks ? D3R_F16X3 : cfg->dtype; m->bdt = f8blocks ? cfg->dtype : m->dt;
    m->ktile = 128 / (int)dt_bytes(m->dt);
    {   // LayerNorm folded into the neighbouring GEMMs (see d3r_model::ln_fold): split-fp16 engines, every channel count a multiple of 32
        // default ON since round 5 (same-box A/B of two engines in one process, tools/fold_probe.py, profiles/r05_d: 168.8 -> 164.9 ms per 32-pair forward,
        // "other" kernels 11.9 -> 5.3 ms, nn.Linear launches +1.8 ms); D3R_LN_FOLD=0: LayerNorm kernels and an fp32 residual stream (rounds 1-4)
        const char* e = getenv("D3R_LN_FOLD");
        const bool want = e ? e[0] != '0' : true;
        m->ln_fold = want && m->dt == D3R_F16X3 && m->bdt == D3R_F16X3 && cfg->enc_embed_dim % 32 == 0 && cfg->dec_embed_dim % 32 == 0;
    }
    if (cfg->enc_embed_dim % m->ktile || cfg->dec_embed_dim % m->ktile || (3 * cfg->patch_size * cfg->patch_size) % m->ktile ||
        (cfg->head_type == 1 && (cfg->dec_depth <= 9 || cfg->patch_size != 16))) { delete m; return D3R_ERR_INVALID; }   // run_dpt assumes 16 x th == H
    if (!build_slots(m)) { d3r_model_destroy(m); return D3R_ERR_ALLOC; }
    m->rope_table = (float*)m->dalloc(512 * 16 * 2 * sizeof(float));
    m->zero_page = m->dalloc(4096);
    // split-K of the small-batch forwards: implemented, deterministic, and measured a LOSS on MI355X (profiles/r06_c: one pair 9.86 ms without, 9.99 ms with it on
    // the 64 x 64 tile, 12.5-13.7 ms on 128 x 128 tiles split 4-8 ways) -- opt-in (D3R_SPLITK=1 at create, D3R_MODEL_OPT_SPLIT_K), off by default
    { const char* e = getenv("D3R_SPLITK"); m->splitk_on = e && e[0] == '1'; }
    for (int i = 0; i < 2 && m->dt == D3R_F16X3; ++i) {
        m->sk_slab[i] = (float*)m->dalloc(d3r_model::SK_SLAB_FLOATS * sizeof(float));
        m->sk_cnt[i] = (unsigned*)m->dalloc(d3r_model::SK_CNT * sizeof(unsigned));
        if (!m->sk_slab[i] || !m->sk_cnt[i] || hipMemset(m->sk_cnt[i], 0, d3r_model::SK_CNT * sizeof(unsigned)) != hipSuccess) { m->sk_slab[i] = nullptr; m->sk_cnt[i] = nullptr; }
    }
    if (!m->rope_table || !m->zero_page) { d3r_model_destroy(m); return D3R_ERR_ALLOC; }
    if (launch_rope_table(m->rope_table, 512, cfg->rope_freq, 1.0f, nullptr) != hipSuccess) { d3r_model_destroy(m); return D3R_ERR_LAUNCH; }
    m->side = shared_stream(0);
    if (!m->side || hipEventCreateWithFlags(&m->ev_main, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_side, hipEventDisableTiming) != hipSuccess) { d3r_model_destroy(m); return D3R_ERR_ALLOC; }
    if (const char* e = getenv("D3R_GRAPH_MAX_PAIRS")) m->graph_max_pairs = atoi(e) > 0 ? atoi(e) : 0;
    if (const char* e = getenv("D3R_LN_INLINE_ROWS")) m->ln_inline_rows = atoi(e) > 0 ? atoi(e) : 0;
    (void)hipDeviceSynchronize();
    *out = m;
    return D3R_OK;
}

extern "C" int d3r_model_destroy(d3r_model* m) {
    if (!m) return D3R_OK;
    for (void* p : m->allocs) (void)hipFree(p);
    for (Lin* L : m->fold_lins) if (L->w32) (void)hipFree(L->w32);
    for (hipEvent_t e : m->prof_ev) (void)hipEventDestroy(e);
    if (m->ev_main) (void)hipEventDestroy(m->ev_main);
    if (m->ev_side) (void)hipEventDestroy(m->ev_side);
    if (m->side) (void)hipStreamSynchronize(m->side);      // shared with the process' other engines (shared_stream): drained, never destroyed
    m->drop_graphs();
    if (m->cap) (void)hipStreamDestroy(m->cap);
    if (m->ws) (void)hipFree(m->ws);
    if (m->stage) (void)hipFree(m->stage);
    delete m;
    return D3R_OK;
}

static int load_tensor_dev(d3r_model* m, const char* key, const float* data_dev, int ndim, const int64_t* shape) {
    auto it = m->slots.find(key);
    if (it == m->slots.end()) {
        const std::string k(key);
        if (k.find("pos_embed") != std::string::npos || k.rfind("prediction_head", 0) == 0) return D3R_OK;
        return D3R_ERR_UNKNOWN_KEY;
    }
    Slot& s = it->second;
    int rc = pack_slot(m, s, data_dev, ndim, shape);
    if (rc != D3R_OK) return rc;
    s.loaded = true;
    if (std::string(key).rfind("dec_blocks2.", 0) == 0) s.explicit_loaded = true;
    if (!s.mirror.empty()) {
        Slot& t = m->slots[s.mirror];
        if (!t.explicit_loaded) {
            rc = pack_slot(m, t, data_dev, ndim, shape);
            if (rc != D3R_OK) return rc;
            t.loaded = true;
        }
    }
    return D3R_OK;
}

extern "C" int d3r_model_load_tensor_device(d3r_model* m, const char* key, const float* data_dev, int ndim, const int64_t* shape) {
    if (!m || !key || !data_dev || ndim < 0 || ndim > 8) return D3R_ERR_INVALID;
    return load_tensor_dev(m, key, data_dev, ndim, shape);
}

extern "C" int d3r_model_load_tensor(d3r_model* m, const char* key, const float* data, int ndim, const int64_t* shape) {
    if (!m || !key || !data || ndim < 0 || ndim > 8) return D3R_ERR_INVALID;
    size_t numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
    const size_t bytes = (numel ? numel : 1) * sizeof(float);
    if (bytes > m->stage_bytes) {                 // host tensors are staged through one device buffer, packed on the GPU
        (void)hipDeviceSynchronize();
        if (m->stage) (void)hipFree(m->stage);
        m->stage = nullptr; m->stage_bytes = 0;
        if (hipMalloc(&m->stage, bytes) != hipSuccess) return D3R_ERR_ALLOC;
        m->stage_bytes = bytes;
    }
    // synchronous copy on the default stream: ordered after the previous tensor's pack kernels
    if (hipMemcpy(m->stage, data, numel * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return D3R_ERR_ALLOC;
    const int rc = load_tensor_dev(m, key, (const float*)m->stage, ndim, shape);
    if (hipStreamSynchronize(nullptr) != hipSuccess) return D3R_ERR_LAUNCH;   // the staging buffer is reused by the next call
    return rc;
}

extern "C" int d3r_model_missing(const d3r_model* m) {
    if (!m) return -1;
    int n = 0;
    for (auto& kv : m->slots)
        if (!kv.second.loaded) ++n;
    return n;
}

extern "C" size_t d3r_model_device_bytes(const d3r_model* m) { return m ? m->weight_bytes + m->ws_bytes : 0; }

extern "C" int d3r_model_debug_read(d3r_model* m, int what, float* out, size_t max_elems, void* stream) {
    if (!m || what != 0 || !m->last_encn) return D3R_ERR_INVALID;
    const size_t n = m->last_encn_elems < max_elems ? m->last_encn_elems : max_elems;
    if (m->dt == D3R_F32) return hipMemcpyAsync(out, m->last_encn, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? D3R_OK : D3R_ERR_LAUNCH;
    return D3R_ERR_INVALID;  // 16-bit modes: read through the Python side (torch view of the raw buffer is not exposed)
}

extern "C" int d3r_model_set_option(d3r_model* m, int option, int value) {
    if (!m) return D3R_ERR_INVALID;
    if (option == D3R_MODEL_OPT_PROFILE) { m->prof_on = value != 0; m->prof_rec.clear(); return D3R_OK; }
    if (option == D3R_MODEL_OPT_TWO_STREAMS) { m->two_streams = value != 0; return D3R_OK; }
    if (option == D3R_MODEL_OPT_SPLIT_K) { hipDeviceSynchronize(); m->drop_graphs(); m->splitk_on = value != 0; return D3R_OK; }
    if (option == D3R_MODEL_OPT_GRAPH_MAX_PAIRS) {
        m->graph_max_pairs = value > 0 ? value : 0;
        if (value <= 0) { hipDeviceSynchronize(); m->drop_graphs(); }     // a replay of the previous call may still be in flight
        return D3R_OK;
    }
    return D3R_ERR_INVALID;
}

// depth_mode / conf_mode of the heads' postprocess (dust3r/heads/postprocess.py:23-58; model.py:58-62 constructor keywords)
extern "C" int d3r_model_set_postprocess(d3r_model* m, int depth_mode, int conf_mode, float conf_vmin, float conf_vmax) {
    PostMode pm;
    if (!m || !post_mode(pm, depth_mode, conf_mode, conf_vmin, conf_vmax)) return D3R_ERR_INVALID;
    hipDeviceSynchronize();     // a captured graph carries the old mode in its kernel arguments
    m->drop_graphs();
    m->post = pm;
    return D3R_OK;
}

// Per-class totals of the LAST forward run with profiling on (kinds: include/dust3r_hip.h). Synchronises on the recorded events.
extern "C" int d3r_model_profile_read(d3r_model* m, int kind, int* launches, double* ms, double* work) {
    if (!m || kind < 0 || kind > 31 || m->prof_rec.size() < 2) return D3R_ERR_STATE;
    int n = 0; double t = 0.0, w = 0.0;
    if (hipEventSynchronize(m->prof_ev[m->prof_rec.size() - 1]) != hipSuccess) return D3R_ERR_LAUNCH;
    for (size_t i = 0; i + 1 < m->prof_rec.size(); ++i) {
        if (m->prof_rec[i].kind != kind) continue;
        float dt = 0.f;
        if (hipEventElapsedTime(&dt, m->prof_ev[i], m->prof_ev[i + 1]) != hipSuccess) return D3R_ERR_LAUNCH;
        ++n; t += dt; w += m->prof_rec[i].work;
    }
    if (launches) *launches = n;
    if (ms) *ms = t;
    if (work) *work = w;
    return D3R_OK;
}

// One launch of the LAST profiled forward: its class (as above), GEMM shape (M, N, K; attention: batch*heads, queries, keys; 0 for
// other kernels), duration and algorithmic work. Returns D3R_ERR_STATE past the last launch.
extern "C" int d3r_model_profile_launch(d3r_model* m, int index, int* kind, int* M, int* N, int* K, double* ms, double* work) {
    if (!m || index < 0 || (size_t)index + 1 >= m->prof_rec.size()) return D3R_ERR_STATE;
    if (hipEventSynchronize(m->prof_ev[m->prof_rec.size() - 1]) != hipSuccess) return D3R_ERR_LAUNCH;
    float dt = 0.f;
    if (hipEventElapsedTime(&dt, m->prof_ev[index], m->prof_ev[index + 1]) != hipSuccess) return D3R_ERR_LAUNCH;
    const auto& r = m->prof_rec[index];
    if (kind) *kind = r.kind;
    if (M) *M = r.M;
    if (N) *N = r.N;
    if (K) *K = r.K;
    if (ms) *ms = dt;
    if (work) *work = r.work;
    return D3R_OK;
}

// ---- the forward ---------------------------------------------------------------------------------------------
namespace {

// Phases: the encoder runs over `nimg` images (img1 holds the first nimg1 of them, img2 the rest: forward passes B + B,
// d3r_model_encode passes everything in img1) and leaves the normalised features [nimg][N][Ce] in `feat`; the decoder +
// heads run over B pairs whose features are feat[0..B) (view 1) and feat[B..2B) (view 2). forward = both phases with
// feat inside the workspace; encode / decode run one phase with a caller-owned feature buffer.
enum { PH_ENCODE = 1, PH_DECODE = 2 };
// one call of the engine, as its entry point describes it
struct Call {
    int phases = 0;
    const float* img1 = nullptr; const float* img2 = nullptr; int nimg1 = 0, nimg = 0;
    void* feat = nullptr;                   // caller-owned feature buffer (encode / decode); null: inside the workspace
    int B = 0;
    SideDim d[2];
    float* pts[2] = {nullptr, nullptr}; float* conf[2] = {nullptr, nullptr};
    int pstride = 3, cstride = 1;           // output element strides between pixels (8, 8: the packed entry points)
};

// row counts of a call. Shared scratch is sized for the wider of encoder / decoder (Cmax, Hmax); Ge, Gd: 32-column groups of a folded LayerNorm's partial sums
struct Dims { int Ce, Cd, He, Hd, Cmax, Hmax, Ge, Gd, Me, Ms[2], Roff[2], M2d, Mmax, M2, ldv_max, nvt, chunk; bool same, do_enc, do_dec; size_t eb; };
Dims dims_of(const d3r_model* m, const Call& k) {
    const d3r_model_config& cf = m->cfg;
    const SideDim &d0 = k.d[0], &d1 = k.d[1];
    Dims d;
    d.Ce = cf.enc_embed_dim; d.Cd = cf.dec_embed_dim; d.He = cf.enc_num_heads; d.Hd = cf.dec_num_heads;
    d.Cmax = d.Ce > d.Cd ? d.Ce : d.Cd; d.Hmax = d.He > d.Hd ? d.He : d.Hd; d.Ge = d.Ce / 32; d.Gd = d.Cd / 32;
    d.same = d0.H == d1.H && d0.W == d1.W; d.do_enc = (k.phases & PH_ENCODE) != 0; d.do_dec = (k.phases & PH_DECODE) != 0;
    // encoder rows: one pass over all images when the views share a size, else one pass per view (view 1 rows first)
    d.Me = !d.do_enc ? 0 : (d.same ? k.nimg * d0.N : k.nimg1 * d0.N + (k.nimg - k.nimg1) * d1.N);
    d.Ms[0] = d.do_dec ? k.B * d0.N : 0; d.Ms[1] = d.do_dec ? k.B * d1.N : 0;     // decoder rows per side
    d.Roff[0] = 0; d.Roff[1] = d.Ms[0];                                           // first row of a side in the two-sided buffers
    d.M2d = d.Ms[0] + d.Ms[1];
    d.Mmax = d.Ms[0] > d.Ms[1] ? d.Ms[0] : d.Ms[1];                               // a side's scratch part holds its own rows OR the other view's (cross attention)
    d.M2 = d.Me > 2 * d.Mmax ? d.Me : 2 * d.Mmax;                                 // rows of the shared scratch buffers
    d.ldv_max = d0.ldv > d1.ldv ? d0.ldv : d1.ldv;
    d.nvt = (d.do_enc ? k.nimg : 0) > 2 * (d.do_dec ? k.B : 0) ? k.nimg : 2 * k.B;   // images the v^T buffer must hold
    d.chunk = k.B < 32 ? k.B : 32;   // 288 GB of HBM: batch the head as wide as the encoder (low-resolution stages need the rows)
    d.eb = dt_bytes(m->dt);
    return d;
}

// ---- workspace layouts: ONE sequence of takes per arena. On Arena(nullptr, 0) it sizes the arena, on the real base it yields the pointers. ----
struct DptGrid { int H[4], W[4]; };       // the four reassembled maps of a th x tw token grid
DptGrid dpt_grid(int th, int tw) { return DptGrid{{4 * th, 2 * th, th, (th - 1) / 2 + 1}, {4 * tw, 2 * tw, tw, (tw - 1) / 2 + 1}}; }
struct DptBufs { void *cmap[4], *t1, *r[4], *rr[4], *tA, *tB, *tC, *up[4], *h0, *h1, *h2; bool fuse_up0, fuse_h1; };      // fuse_*: that x2 map is interpolated inside its consumer and has no buffer      // up[lvl]: refinenet lvl's upsampled output
DptBufs dpt_layout(const d3r_model* m, const DptHead& D, Arena& ar, int B, int th, int tw) {
    const size_t eb = dt_bytes(m->dt), px8 = (size_t)B * 8 * th * 8 * tw;
    const DptGrid g = dpt_grid(th, tw);
    DptBufs b;
    for (int i = 0; i < 4; ++i) b.cmap[i] = ar.take((size_t)B * g.H[i] * g.W[i] * D.cstride[i] * eb);
    b.t1 = ar.take((size_t)B * th * tw * 768 * eb);
    for (int i = 0; i < 4; ++i) { b.r[i] = ar.take((size_t)B * g.H[i] * g.W[i] * 256 * eb); b.rr[i] = ar.take((size_t)B * g.H[i] * g.W[i] * 256 * eb); }
    for (void** t : {&b.tA, &b.tB, &b.tC}) *t = ar.take((size_t)B * g.H[0] * g.W[0] * 256 * eb);
    // the two large x2 maps (refinenet-0's output: 1.6 GB per head at 32 pairs; head.0's: 3.2 GB) only where their consumers do not interpolate them themselves
    b.fuse_up0 = head0_upfused(m, D.head0, B, g.H[0], g.W[0], 256, 128);
    b.fuse_h1 = head_upfused(m, D.head2, B, 8 * th, 8 * tw, 128);
    for (int lvl = 3; lvl >= 0; --lvl)      // dpt_head.py:57 crops refinenet4's output to layer 3's size
        b.up[lvl] = lvl == 0 && b.fuse_up0 ? nullptr : ar.take((size_t)B * (lvl == 3 ? g.H[2] : 2 * g.H[lvl]) * (lvl == 3 ? g.W[2] : 2 * g.W[lvl]) * 256 * eb);
    b.h0 = ar.take(px8 * 128 * eb); b.h1 = b.fuse_h1 ? nullptr : ar.take(4 * px8 * 128 * eb); b.h2 = ar.take(4 * px8 * 128 * eb);
    return b;
}

// folded LayerNorm (d3r_model::ln_fold): partial sums [rows][C / 32][2], rstd / -mean rstd per row
struct FoldSet { float *part = nullptr, *rs = nullptr, *nm = nullptr; };
FoldSet take_fold(Arena& ar, int rows, int groups) {
    FoldSet s;
    s.part = (float*)ar.take((size_t)rows * groups * 8); s.rs = (float*)ar.take((size_t)rows * 4 + 16); s.nm = (float*)ar.take((size_t)rows * 4 + 16);
    return s;
}
struct Workspace {
    float* x; void *xn, *q, *k, *vt, *ao, *hb, *encn; float* f[2]; void* yn; void* hook[2][3]; float* lin_out;
    // fold sets: one for the encoder (e), one per decoder LAYER OUTPUT and buffer (l: both sides' rows, read by the own side's norm1 and the other side's norm_y) with
    // the raw typed copy fr of that output, one per side for the block-internal norm2 / norm3 (s)
    FoldSet e, l[2], s[2]; void* fr[2] = {nullptr, nullptr};
    void* head_arena[2]; size_t head_bytes = 0;     // the DPT head's arena of each side
    size_t bytes = 0;                               // the whole workspace
};
Workspace ws_layout(const d3r_model* m, const Call& k, const Dims& d, Arena& ar) {
    const size_t eb = d.eb, scratch = (size_t)d.M2 * d.Cmax * eb;
    const int ps = m->cfg.patch_size;
    Workspace w;
    w.x = (float*)ar.take((size_t)d.Me * d.Ce * 4);
    w.xn = ar.take(scratch); w.q = ar.take(scratch); w.k = ar.take(scratch);
    w.vt = ar.take((size_t)d.nvt * d.Hmax * 64 * d.ldv_max * eb);
    w.ao = ar.take(scratch);
    w.hb = ar.take(4 * scratch);   // MLP hidden; also holds the gathered patches
    w.encn = k.feat ? k.feat : ar.take((size_t)(d.Me > d.M2d ? d.Me : d.M2d) * d.Ce * eb);
    for (int b = 0; b < 2; ++b) w.f[b] = (float*)ar.take((size_t)d.M2d * d.Cd * 4);
    w.yn = ar.take((size_t)2 * d.Mmax * d.Cd * eb);
    for (int s = 0; s < 2; ++s)
        for (int j = 0; j < 3; ++j) w.hook[s][j] = ar.take((size_t)d.Ms[s] * d.Cd * eb);
    w.lin_out = m->cfg.head_type == 0 ? (float*)ar.take((size_t)d.M2d * 4 * ps * ps * 4) : nullptr;
    if (m->ln_fold) {
        w.e = take_fold(ar, d.Me, d.Ge);
        for (int b = 0; b < 2; ++b) { w.fr[b] = ar.take((size_t)d.M2d * d.Cd * eb); w.l[b] = take_fold(ar, d.M2d, d.Gd); w.s[b] = take_fold(ar, d.Mmax, d.Gd); }
    }
    // both sides' arenas hold a chunk of the larger view -- a full chunk or the call's last, smaller one: with fewer pixel tiles the head may keep the x2 map
    // that a full chunk does not take (head_upfused), so the smaller chunk is laid out too
    for (int s = 0; s < 2 && m->cfg.head_type == 1 && d.do_dec; ++s)
        for (int nb : {d.chunk, d.chunk > 0 ? k.B % d.chunk : 0}) {
            if (nb <= 0) continue;
            Arena sub(nullptr, 0);
            dpt_layout(m, m->dpt[0], sub, nb, k.d[s].th, k.d[s].tw);
            const size_t a = ((sub.off + 255) & ~(size_t)255) + 256;
            w.head_bytes = a > w.head_bytes ? a : w.head_bytes;
        }
    for (int s = 0; s < 2; ++s) w.head_arena[s] = ar.take(w.head_bytes);
    w.bytes = ar.off + 256;
    return w;
}

// ---- the residual stream of a transformer block in its two representations -------------------------------------------------------------------
// M rows of the stream at one point of a block. LayerNorm-kernel engines: fp32 rows `f32` (`raw`: a typed copy where one is wanted -- the DPT hooks).
// ln_fold engines: the typed rows `raw` ARE the stream (GF_X3RES) and carry a statistics set: `part` is written by the GEMM that stores the rows (null: none
// wanted, a LayerNorm kernel follows), rs / nm by an ln_finalize launch behind it or, up to ln_inline_rows rows (`inl`), by the consumer GEMM's prologue.
struct Res { int M = 0; float* f32 = nullptr; void* raw = nullptr; float* part = nullptr; float* rs = nullptr; float* nm = nullptr; bool inl = false; };
Res rows_of(const d3r_model* m, int M, float* f32, void* raw, const FoldSet& s, int first = 0, int groups = 0) {
    Res r; r.M = M; r.f32 = f32; r.raw = raw; r.inl = M <= m->ln_inline_rows;
    if (s.part) { r.part = s.part + (size_t)first * groups * 2; r.rs = s.rs + first; r.nm = s.nm + first; }
    return r;
}
// normalised input of the nn.Linear behind LayerNorm `ln`: the LayerNorm kernel into `scratch`, or (folded) nothing -- the raw rows and their statistics
NormIn norm_in(Ctx& c, const Res& r, const LNp& ln, void* scratch, int C) {
    if (c.m->ln_fold) return NormIn{r.raw, LnStats{r.rs, r.nm, r.inl ? r.part : nullptr}};
    D3R_OTHER(launch_layernorm(c.m->bdt, r.f32, ln.g, ln.b, scratch, r.M, C, 1e-6f, c.st));
    return NormIn{scratch, LnStats()};
}
// out = in + Linear(act) (`in` may be empty): fp32 rows, or (folded) typed rows + partial sums and the ln_finalize launch directly behind their producer
void residual_linear(Ctx& c, const Lin& L, const void* act, int lda, const Res& in, const Res& out, int C, bool typed_copy = false) {
    const bool fold = c.m->ln_fold;
    GemmParams p = lin_params(L, act, lda, out.M);
    if (fold) epi_typed_residual(p, in.raw, out.raw, C, out.part);
    else { p.epi = EPI_F32; p.ldo = C; p.out = out.f32; p.res1 = in.f32; if (typed_copy) { p.out2 = out.raw; p.ldo2 = C; } }
    gemm_linear(c, L, p);
    if (fold && out.part && !out.inl) D3R_OTHER(launch_ln_finalize(out.part, out.M, C, 1e-6f, out.rs, out.nm, c.st));
}
// a LayerNorm whose output leaves the blocks (enc_norm, dec_norm): always a kernel
void final_norm(Ctx& c, const Res& r, const LNp& ln, void* dst, int C) {
    if (c.m->ln_fold) D3R_OTHER(launch_layernorm_x3in(r.raw, ln.g, ln.b, dst, r.M, C, 1e-6f, c.st));
    else D3R_OTHER(launch_layernorm(c.m->dt, r.f32, ln.g, ln.b, dst, r.M, C, 1e-6f, c.st));
}
// a Linear with nothing but an epilogue and one output (n_store: columns written when not L.N)
void plain_linear(Ctx& c, const Lin& L, const NormIn& in, int lda, int M, int epi, void* out, int ldo, int n_store = -1) {
    GemmParams p = lin_params(L, in.rows, lda, M, in.stats);
    p.epi = epi; p.out = out; p.ldo = ldo;
    if (n_store >= 0) p.n_store = n_store;
    gemm_linear(c, L, p);
}
// softmax(q k^T / 8) v over nimg x heads problems: qd = the queries' token grid, kd = the keys' (self attention: the same)
struct AttnBufs { void *q, *k, *vt, *ao; };
void attention(Ctx& c, const AttnBufs& b, int nimg, int heads, const SideDim& qd, const SideDim& kd) {
    AttnParams a;
    a.q = b.q; a.k = b.k; a.vt = b.vt; a.out = b.ao; a.B = nimg; a.H = heads; a.Nq = qd.N; a.Nk = kd.N; a.ldv = kd.ldv; a.scale = 0.125f;
    a.out_dt = c.m->bdt;      // rows for the proj GEMM
    c.mark(PRF_ATTN, 4.0 * nimg * heads * (double)qd.N * kd.N * 64, nimg * heads, qd.N, kd.N);
    c.chk(launch_attention(c.m->dt, a, c.st));
}

// ---- the DPT head of one side for B images of a th x tw token grid, in its arena `ar` ------------------------------------------------------------
void run_dpt(Ctx& c, const DptHead& D, Arena ar, const Call& k, const void* const hooks[4], const int hook_c[4], int B, int th, int tw, float* pts, float* conf) {
    d3r_model* m = c.m;
    const DptGrid g = dpt_grid(th, tw);
    const DptBufs b = dpt_layout(m, D, ar, B, th, tw);
    // reassemble: 1x1 conv (+ ConvTranspose / strided conv)
    for (int i = 0; i < 4; ++i) {
        plain_linear(c, D.act1x1[i], NormIn{hooks[i]}, hook_c[i], B * th * tw, EPI_T, i == 2 ? b.cmap[2] : b.t1, D.cstride[i], D.cstride[i]);
        if (i < 2) {
            const int ldi[2] = {96, 192}, kk = D.convt_k[i] * D.convt_k[i];
            GemmParams p = lin_params(D.convt[i], b.t1, D.cstride[i], B * th * tw);
            epi_convt(p, D.convt_k[i], D.convt_coutp[i], th, tw, b.cmap[i], D.cstride[i]);
            launch(c, m->dt, p, PRF_CONV, kk * ldi[i], ldi[i]);
        } else if (i == 3) {
            conv(c, b.t1, B, th, tw, D.cstride[3], D.act3conv, 2, 1, b.cmap[3], D.cstride[3], 0);
        }
    }
    // layer_rn: 3x3 -> 256 (no bias), plus ReLU copy for the residual units' pre-activation
    for (int i = 0; i < 4; ++i) conv(c, b.cmap[i], B, g.H[i], g.W[i], D.cstride[i], D.layer_rn[i], 1, 1, b.r[i], 256, 0, nullptr, nullptr, b.rr[i]);
    void* path = nullptr;  // output of the previous refinenet (already upsampled)
    for (int lvl = 3; lvl >= 0; --lvl) {
        const Refine& R = D.rn[lvl];
        const int H = g.H[lvl], W = g.W[lvl];
        const void* skip = b.r[3];         // input of resConfUnit2 (un-activated) ...
        const void* skip_relu = b.rr[3];   // ... and its ReLU
        if (lvl != 3) {
            conv(c, b.rr[lvl], B, H, W, 256, R.r1c1, 1, 1, b.tA, 256, GF_RELU);
            conv(c, b.tA, B, H, W, 256, R.r1c2, 1, 1, b.tB, 256, 0, m->cfg.dpt_skip_relu_inplace ? b.rr[lvl] : b.r[lvl], path, b.tC);
            skip = b.tB; skip_relu = b.tC;
        }
        conv(c, skip_relu, B, H, W, 256, R.r2c1, 1, 1, b.tA, 256, GF_RELU);
        void* o = (lvl == 3) ? b.tB : b.tC;
        conv(c, b.tA, B, H, W, 256, R.r2c2, 1, 1, o, 256, 0, m->cfg.dpt_skip_relu_inplace ? skip_relu : skip);
        // out_conv (1x1) commutes with the bilinear upsampling (both linear, weights sum to 1): run it at low resolution
        plain_linear(c, R.outc, NormIn{o}, 256, B * H * W, EPI_T, b.tA, 256);
        if (lvl == 0 && b.fuse_up0) break;      // head.0 below interpolates this level's x2 map itself
        D3R_OTHER(launch_upsample2x(m->dt, b.tA, b.up[lvl], nullptr, B, H, W, 256, 256, lvl == 3 ? g.H[2] : 2 * H, lvl == 3 ? g.W[2] : 2 * W, c.st));
        path = b.up[lvl];
    }
    // head: 3x3 256->128, x2, 3x3 128->128 + ReLU, 1x1 128->4 + postprocess
    const int H8 = 8 * th, W8 = 8 * tw;
    if (b.fuse_up0) conv_up2(c, b.tA, B, g.H[0], g.W[0], 256, D.head0, b.h0, 128, 0);
    else conv(c, path, B, H8, W8, 256, D.head0, 1, 1, b.h0, 128, 0);
    // Split-fp16, whole 16 x 32 tiles of output pixels, a tile per CU: the x2 map is interpolated inside the last convolution (with the fused tail below), never stored
    if (b.fuse_h1) { conv_up2_head4(c, b.h0, B, H8, W8, 128, D.head2, D.head4_w, D.head4_b, pts, conf, k.pstride, k.cstride); return; }
    D3R_OTHER(launch_upsample2x(m->dt, b.h0, b.h1, nullptr, B, H8, W8, 128, 128, 2 * H8, 2 * W8, c.st));
    // Split-fp16, enough pixels for the 512 x 128 tile (every wave then holds all 128 channels of its 64 pixels): the 1x1 convolution and
    // the postprocess run in the epilogue of the last 3x3 convolution, on its fp32 accumulators -- the 128-channel full-resolution map
    // (3.2 GB per head at 32 pairs) is neither written nor read back.
    if (head_fuse_on(m) && conv_head4(c, b.h1, B, 2 * H8, 2 * W8, 128, D.head2, D.head4_w, D.head4_b, pts, conf, k.pstride, k.cstride)) return;
    conv(c, b.h1, B, 2 * H8, 2 * W8, 128, D.head2, 1, 1, b.h2, 128, GF_RELU);
    D3R_OTHER(launch_head_final(m->dt, b.h2, 128, D.head4_w, D.head4_b, pts, conf, (size_t)B * 4 * H8 * W8, k.pstride, k.cstride, m->post, c.st));
}

// ---- one forward -------------------------------------------------------------------------------------------------------------------------------
// Stream plan: encoder on the caller's stream; then side 0 stays there and side 1 runs on the model's second stream, re-joined at every layer boundary (each
// side reads the other's previous-layer output) and at the end. Each side has its own part of every scratch buffer and its own head arena.
struct EncGroup { const float* im[2]; int n[2]; const SideDim* dd; size_t row0; };
struct Fwd {
    d3r_model* m; const Call& k; const Dims d; const Workspace w; Ctx c;
    bool two; hipStream_t S[2];
    int cur = 0;                                                  // decoder: the buffer (f / fr / l) that holds the layers' input
    void* typed[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}; // typed rows of a layer's output [buffer][side]: folded, the stream itself (fr, or a DPT hook buffer at the hook layers); else the hook copy or null

    // fork: side 1 waits for what side 0 has enqueued; join: side 0 for side 1; both: a layer boundary
    void sync(bool fork, bool join) {
        if (!two) return;
        if (fork) c.chk(hipEventRecord(m->ev_main, S[0]));
        if (join) c.chk(hipEventRecord(m->ev_side, S[1]));
        if (join) c.chk(hipStreamWaitEvent(S[0], m->ev_side, 0));
        if (fork) c.chk(hipStreamWaitEvent(S[1], m->ev_main, 0));
    }
    // side sd's rows of the decoder's layer boundary `buf`: the statistics set of side t has Ms[t] rows whoever consumes it
    Res boundary(int buf, int sd) const { return rows_of(m, d.Ms[sd], w.f[buf] + (size_t)d.Roff[sd] * d.Cd, typed[buf][sd], w.l[buf], d.Roff[sd], d.Gd); }

    // Encoder: the images of one size in one pass, in the scratch buffers from row 0. Fold: every residual epilogue stores the typed rows (the residual stream
    // itself, GF_X3RES) and their partial sums; the LayerNorm is two fmas in the epilogue of the nn.Linear behind it (weights packed as W diag(gamma)) -- DESIGN 4.0
    void encode_group(const EncGroup& g) {
        const SideDim& dd = *g.dd;
        const int Ce = d.Ce, ps = m->cfg.patch_size, depth = m->cfg.enc_depth, n_img = g.n[0] + g.n[1], Mp = n_img * dd.N;
        const size_t pk = 3 * (size_t)ps * ps;
        const Res x = rows_of(m, Mp, w.x + g.row0 * Ce, w.xn, w.e);
        if (g.n[0] > 0) D3R_OTHER(launch_patchify(m->dt, g.im[0], w.hb, g.n[0], dd.H, dd.W, ps, c.st));     // the patches start where the hidden rows do
        if (g.n[1] > 0) D3R_OTHER(launch_patchify(m->dt, g.im[1], (char*)w.hb + (size_t)g.n[0] * dd.N * pk * d.eb, g.n[1], dd.H, dd.W, ps, c.st));
        residual_linear(c, m->patch, w.hb, (int)pk, Res(), x, Ce);
        for (int l = 0; l < depth; ++l) {
            const EncBlk& b = m->enc[l];
            gemm_heads(c, b.qkv, norm_in(c, x, b.n1, w.xn, Ce), Mp, Ce, d.He, dd, {HEAD_ROPE, w.q}, {HEAD_ROPE, w.k}, {HEAD_VT, w.vt});
            attention(c, AttnBufs{w.q, w.k, w.vt, w.ao}, n_img, d.He, dd, dd);
            residual_linear(c, b.proj, w.ao, Ce, x, x, Ce);
            plain_linear(c, b.fc1, norm_in(c, x, b.n2, w.xn, Ce), Ce, Mp, EPI_GELU, w.hb, 4 * Ce);
            Res y = x;
            if (l + 1 == depth) y.part = nullptr;        // enc_norm (a kernel) follows: no sums
            residual_linear(c, b.fc2, w.hb, 4 * Ce, x, y, Ce);
        }
        final_norm(c, x, m->enc_norm, (char*)w.encn + g.row0 * Ce * d.eb, Ce);
    }
    // all images of the call as one group when the views share a size (model.py:142-151 concatenates the two views), else view 1's images, then view 2's (model.py:148-150)
    void encoder() {
        if (d.same) encode_group(EncGroup{{k.img1, k.img2}, {k.nimg1, k.nimg - k.nimg1}, &k.d[0], 0});
        if (!d.same && k.nimg1 > 0) encode_group(EncGroup{{k.img1, nullptr}, {k.nimg1, 0}, &k.d[0], 0});
        if (!d.same && k.nimg > k.nimg1) encode_group(EncGroup{{k.img2, nullptr}, {k.nimg - k.nimg1, 0}, &k.d[1], (size_t)k.nimg1 * k.d[0].N});
        m->last_encn = w.encn; m->last_encn_elems = (size_t)d.Me * d.Ce;
    }

    // Decoder block l of side s (model.py:172-191) on the stream c.st: reads the PREVIOUS layer's output of both sides (buffer cur), writes its own into cur ^ 1.
    // The stream: layer input `in` -> `mid` (after self attention, then in place after cross attention) -> `out`, the next layer's input.
    void decoder_block(int l, int s) {
        const int Cd = d.Cd, M = d.Ms[s], layer_no = l + 1, hk6 = m->cfg.dec_depth * 2 / 4, hk9 = m->cfg.dec_depth * 3 / 4;
        const SideDim &own = k.d[s], &oth = k.d[1 - s];
        const DecBlk& b = m->dec[s][l];
        // this side's part of the scratch buffers (the encoder used them whole)
        const size_t part = (size_t)s * d.Mmax * d.Cmax * d.eb;
        void *sxn = (char*)w.xn + part, *shb = (char*)w.hb + 4 * part;
        void* syn = (char*)w.yn + (size_t)s * d.Mmax * Cd * d.eb;         // norm_y of the OTHER view's tokens (Ms[1 - s] <= Mmax rows)
        const AttnBufs ab{(char*)w.q + part, (char*)w.k + part, (char*)w.vt + (size_t)s * k.B * d.Hmax * 64 * d.ldv_max * d.eb, (char*)w.ao + part};
        // fc2 also stores the typed rows of its output: at the hook layers into the DPT hook buffer (folded: the typed layer output IS the hook), else (folded) into fr
        void* hook = (m->cfg.head_type == 1 && (layer_no == hk6 || layer_no == hk9)) ? w.hook[s][layer_no == hk6 ? 0 : 1] : nullptr;
        typed[cur ^ 1][s] = hook || !m->ln_fold ? hook : (void*)((char*)w.fr[cur ^ 1] + (size_t)d.Roff[s] * Cd * d.eb);
        const Res in = boundary(cur, s), other = boundary(cur, 1 - s), mid = rows_of(m, M, w.f[cur ^ 1] + (size_t)d.Roff[s] * Cd, sxn, w.s[s]);
        Res out = boundary(cur ^ 1, s);
        if (layer_no == m->cfg.dec_depth) out.part = nullptr;          // dec_norm (a kernel) follows: no sums
        gemm_heads(c, b.qkv, norm_in(c, in, b.n1, sxn, Cd), M, Cd, d.Hd, own, {HEAD_ROPE, ab.q}, {HEAD_ROPE, ab.k}, {HEAD_VT, ab.vt});
        attention(c, ab, k.B, d.Hd, own, own);
        residual_linear(c, b.proj, ab.ao, Cd, in, mid, Cd);
        // cross attention: q from norm2(x), k / v from norm_y(y) -- the other side's rows (and statistics); Nk = the other view's token count
        const NormIn y = norm_in(c, other, b.ny, syn, Cd);
        gemm_heads(c, b.cq, norm_in(c, mid, b.n2, sxn, Cd), M, Cd, d.Hd, own, {HEAD_ROPE, ab.q});
        gemm_heads(c, b.ckv, y, other.M, Cd, d.Hd, oth, {HEAD_ROPE, ab.k}, {HEAD_VT, ab.vt});
        attention(c, ab, k.B, d.Hd, own, oth);
        residual_linear(c, b.cproj, ab.ao, Cd, mid, mid, Cd);
        plain_linear(c, b.fc1, norm_in(c, mid, b.n3, sxn, Cd), Cd, M, EPI_GELU, shb, 4 * Cd);
        residual_linear(c, b.fc2, shb, 4 * Cd, mid, out, Cd, true);
    }
    // decoder_embed over both sides' rows in one launch, then the layers
    void decoder() {
        for (int sd = 0; sd < 2 && m->ln_fold; ++sd) typed[0][sd] = (char*)w.fr[0] + (size_t)d.Roff[sd] * d.Cd * d.eb;
        Res e = rows_of(m, d.M2d, w.f[0], w.fr[0], w.l[0]);
        e.inl = d.Ms[0] <= m->ln_inline_rows && d.Ms[1] <= m->ln_inline_rows;      // the consumers are per side
        residual_linear(c, m->dec_embed, w.encn, d.Ce, Res(), e, d.Cd);
        sync(true, false);
        for (int l = 0; l < m->cfg.dec_depth; ++l, cur ^= 1) {
            for (int s = 0; s < 2; ++s) { c.st = S[s]; decoder_block(l, s); }
            sync(true, true);
        }
    }
    // dec_norm + heads, each side on its own stream; the caller's stream continues only after side 1 has finished
    void heads() {
        const int Ce = d.Ce, Cd = d.Cd, ps = m->cfg.patch_size, B = k.B;
        for (int s = 0; s < 2; ++s) {
            c.st = S[s];
            const SideDim& own = k.d[s];
            final_norm(c, boundary(cur, s), m->dec_norm, w.hook[s][2], Cd);
            if (m->cfg.head_type == 0) {
                float* lo = w.lin_out + (size_t)d.Roff[s] * 4 * ps * ps;
                plain_linear(c, m->lin_head[s], NormIn{w.hook[s][2]}, Cd, d.Ms[s], EPI_F32, lo, 4 * ps * ps);
                D3R_OTHER(launch_linear_head_post(lo, k.pts[s], k.conf[s], B, own.th, own.tw, ps, k.pstride, k.cstride, m->post, c.st));
            }
            for (int b0 = 0; b0 < B && m->cfg.head_type == 1; b0 += d.chunk) {
                const size_t r0 = (size_t)b0 * own.N, px0 = (size_t)b0 * own.H * own.W;
                const void* hooks[4] = {(const char*)w.encn + ((size_t)d.Roff[s] + r0) * Ce * d.eb, (const char*)w.hook[s][0] + r0 * Cd * d.eb,
                                        (const char*)w.hook[s][1] + r0 * Cd * d.eb, (const char*)w.hook[s][2] + r0 * Cd * d.eb};
                const int hc[4] = {Ce, Cd, Cd, Cd};
                run_dpt(c, m->dpt[s], Arena(w.head_arena[s], w.head_bytes), k, hooks, hc, (B - b0) < d.chunk ? (B - b0) : d.chunk, own.th, own.tw,
                        k.pts[s] + px0 * k.pstride, k.conf[s] + px0 * k.cstride);
            }
        }
        c.st = S[0];
        sync(false, true);
    }
};

// bytes of the workspace a call needs: its layout on no base
size_t workspace_bytes(const d3r_model* m, const Call& k) {
    Arena ar(nullptr, 0);
    return ws_layout(m, k, dims_of(m, k), ar).bytes;
}

// enqueues the call on `st`, in the model's workspace; refuses it before the first launch when a layout does not fit its arena
int forward(d3r_model* m, const Call& k, hipStream_t st) {
    Arena ar(m->ws, m->ws_bytes);
    const Dims d = dims_of(m, k);
    Fwd F{m, k, d, ws_layout(m, k, d, ar), Ctx{m, st, D3R_OK, st}};
    if (!m->ws || F.w.bytes > ar.cap) return D3R_ERR_ALLOC;
    for (int s = 0; s < 2 && F.w.head_bytes; ++s)
        for (int nb : {d.chunk, d.chunk > 0 ? k.B % d.chunk : 0}) {
            if (nb <= 0) continue;
            Arena sub(F.w.head_arena[s], F.w.head_bytes);
            dpt_layout(m, m->dpt[s], sub, nb, k.d[s].th, k.d[s].tw);
            if (sub.off > sub.cap) return D3R_ERR_ALLOC;
        }
    Ctx& c = F.c;
    F.two = m->two_streams && !m->prof_on && m->side != nullptr;
    F.S[0] = st; F.S[1] = F.two ? m->side : st;
    if (k.d[0].ldv != k.d[0].N || k.d[1].ldv != k.d[1].N) D3R_OTHER(hipMemsetAsync(F.w.vt, 0, (size_t)d.nvt * d.Hmax * 64 * d.ldv_max * d.eb, st));
    if (d.do_enc) F.encoder();
    if (d.do_dec) { F.decoder(); F.heads(); }
    c.mark(PRF_END, 0.0);
    return c.rc;
}

}  // namespace

// ln_fold engines: (re)pack the nn.Linear matrices behind a folded LayerNorm whose inputs changed as W diag(gamma) and form their column sums / folded bias,
// from the fp32 rows staged by pack_slot. Runs at the first forward after a load; the staging copies are released afterwards. Bookkeeping is PER MATRIX
// (round 6; before, one stale vector made every one of the ~100 folded matrices demand a reload): a matrix is re-folded when one of its weight tensors, its
// bias or its LayerNorm's vectors were loaded, and it needs ALL of its weight tensors staged for that (projk | projv: both). A vector-only update of a
// matrix whose staging copy is gone cannot be folded: D3R_ERR_STATE until that matrix's weights are loaded again (include/dust3r_hip.h, d3r_model_load_tensor);
// the other matrices are unaffected.
// The two launches of one matrix (kernels.hpp launch_ln_fold_pack): here so that the kernel tests (capi.hip d3r_ln_fold_pack) run what finalize_fold runs.
hipError_t d3r::launch_ln_fold_pack(int dt, const float* W, const float* gamma, const float* beta, const float* bias_in, void* dst, float* colsum, float* bias_out, int N, int K,
                                    hipStream_t s) {
    PackParams pp;
    pp.src = W; pp.numel = (size_t)N * K; pp.dst = dst; pp.dst_cols = K; pp.kind = PACK_MAT; pp.cols = K; pp.row_off = 0;
    pp.kscale = gamma;
    const hipError_t e = launch_pack_weight(dt, pp, s);
    return e != hipSuccess ? e : launch_ln_fold_vectors(dt, W, gamma, beta, bias_in, colsum, bias_out, N, K, s);
}

static int finalize_fold(d3r_model* m) {
    if (!m->ln_fold || !m->fold_dirty) return D3R_OK;
    for (Lin* L : m->fold_lins) if (L->fold_dirty && (!L->w32 || L->have_mask != L->want_mask)) return D3R_ERR_STATE;
    for (Lin* L : m->fold_lins) {
        if (!L->fold_dirty) continue;
        if (launch_ln_fold_pack(L->dt, L->w32, L->ln->g, L->ln->b, L->b, L->w, L->ln_s, L->b_fold, L->N, L->K, nullptr) != hipSuccess) return D3R_ERR_LAUNCH;
    }
    if (hipDeviceSynchronize() != hipSuccess) return D3R_ERR_LAUNCH;
    for (Lin* L : m->fold_lins) {
        if (!L->fold_dirty) continue;
        (void)hipFree(L->w32);
        L->w32 = nullptr;
        L->have_mask = 0;
        L->fold_dirty = false;
    }
    m->fold_dirty = false;
    return D3R_OK;
}

// ---- small whole forwards: replay a captured graph (see d3r_model::GraphEntry). True: the call was served by a replay (or failed trying), *rc is its result;
// false: the caller enqueues it eagerly ----------------------------------------------------------------------------------------------------------
static bool graph_forward(d3r_model* m, const Call& k, hipStream_t st, int* rc) {
    const int B = k.B, H1 = k.d[0].H, W1 = k.d[0].W, H2 = k.d[1].H, W2 = k.d[1].W;
    const bool graphable = k.phases == (PH_ENCODE | PH_DECODE) && m->graph_max_pairs > 0 && B <= m->graph_max_pairs && !m->prof_on && k.nimg1 == B && k.nimg == 2 * B;
    if (!graphable) return false;
    const d3r_model::GraphKey key{B, H1, W1, H2, W2, k.pstride, (m->two_streams && m->side) ? 1 : 0};
    d3r_model::GraphEntry* ge = nullptr;
    for (auto& g : m->graphs)
        if (g.key == key) { ge = &g; break; }
    if (!ge) {
        if (m->graphs.size() >= 16) {                       // a handful of (batch, size) combinations is the expected use
            (void)hipStreamSynchronize(st);                 // a replay enqueued by the previous call (and its staging copies) may still be in flight
            if (m->side) (void)hipStreamSynchronize(m->side);
            if (m->cap) (void)hipStreamSynchronize(m->cap);
            m->drop_graphs();
        }
        m->graphs.push_back(d3r_model::GraphEntry());
        ge = &m->graphs.back();
        ge->key = key;
    }
    const size_t n_in1 = (size_t)B * 3 * H1 * W1, n_in2 = (size_t)B * 3 * H2 * W2;
    const size_t a1 = (size_t)B * H1 * W1, a2 = (size_t)B * H2 * W2;
    const bool packed = k.pstride == 8;                      // one [B][H][W][8] payload (H1 == H2, W1 == W2)
    const size_t n_out = packed ? a1 * 8 : 4 * (a1 + a2);
    // staging layout (floats): img1 | img2 | pts1 conf1 pts2 conf2 (or the packed payload)
    if (ge->seen >= 1 && !ge->exec && ge->seen < 1000) {     // second call: capture
        bool ok = true;
        if (!m->cap) ok = hipStreamCreateWithFlags(&m->cap, hipStreamNonBlocking) == hipSuccess;
        const size_t bytes = (n_in1 + n_in2 + n_out) * sizeof(float);
        if (ok && !ge->io) { ok = hipMalloc((void**)&ge->io, bytes) == hipSuccess; ge->io_bytes = bytes; }
        if (ok) {
            Call staged = k;
            staged.img1 = ge->io; staged.img2 = ge->io + n_in1;
            float* o1 = ge->io + n_in1 + n_in2;
            staged.pts[0] = o1;
            if (packed) { staged.conf[0] = o1 + 3; staged.pts[1] = o1 + 4; staged.conf[1] = o1 + 7; }
            else { staged.conf[0] = o1 + 3 * a1; staged.pts[1] = staged.conf[0] + a1; staged.conf[1] = staged.pts[1] + 3 * a2; }
            ok = hipStreamBeginCapture(m->cap, hipStreamCaptureModeRelaxed) == hipSuccess;
            if (ok) {
                const int crc = forward(m, staged, m->cap);
                hipGraph_t g = nullptr;
                const bool ended = hipStreamEndCapture(m->cap, &g) == hipSuccess && g != nullptr;
                ok = ended && crc == D3R_OK && hipGraphInstantiate(&ge->exec, g, nullptr, nullptr, 0) == hipSuccess;
                if (ok) ge->graph = g;
                else if (g) (void)hipGraphDestroy(g);
            }
        }
        if (!ok) {                        // this shape stays eager
            (void)hipGetLastError();
            ge->exec = nullptr;
            ge->seen = 1000;
        }
    }
    if (!ge->exec) {
        if (ge->seen < 1000) ++ge->seen;
        return false;
    }
    float* io = ge->io;
    const float* o1 = io + n_in1 + n_in2;
    bool ok = hipMemcpyAsync(io, k.img1, n_in1 * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess &&
              hipMemcpyAsync(io + n_in1, k.img2, n_in2 * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess &&
              hipGraphLaunch(ge->exec, st) == hipSuccess;
    if (ok && packed) ok = hipMemcpyAsync(k.pts[0], o1, n_out * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess;
    else if (ok)
        ok = hipMemcpyAsync(k.pts[0], o1, 3 * a1 * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipMemcpyAsync(k.conf[0], o1 + 3 * a1, a1 * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipMemcpyAsync(k.pts[1], o1 + 4 * a1, 3 * a2 * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipMemcpyAsync(k.conf[1], o1 + 4 * a1 + 3 * a2, a2 * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (ok) ++m->graph_replays;
    *rc = ok ? D3R_OK : D3R_ERR_LAUNCH;
    return true;
}

static int run_phases(d3r_model* m, const Call& k, hipStream_t st) {
    // The engines of a process share their helper streams (shared_stream above): the ENQUEUE of a forward -- host side only, the device work stays asynchronous --
    // is therefore one critical section per process. Engines driven from different host threads stay correct (one engine's stream capture cannot swallow another
    // engine's launches on the shared side stream; fork / join events of two forwards do not interleave); their side-stream halves run in enqueue order.
    static std::mutex enqueue_mu;
    std::lock_guard<std::mutex> enqueue_lock(enqueue_mu);
    const int ps = m->cfg.patch_size;
    for (const SideDim& v : k.d)
        if (v.H % ps || v.W % ps || v.H <= 0 || v.W <= 0 || v.H / ps > 511 || v.W / ps > 511) return D3R_ERR_SHAPE;
    if (d3r_model_missing(m) != 0) return D3R_ERR_STATE;
    { const int frc = finalize_fold(m); if (frc != D3R_OK) return frc; }
    const size_t need = workspace_bytes(m, k);
    if (need > m->ws_bytes) {
        (void)hipStreamSynchronize(st);
        if (m->side) (void)hipStreamSynchronize(m->side);
        m->drop_graphs();                         // captured launches point into the old workspace
        if (m->ws) (void)hipFree(m->ws);
        m->ws = nullptr; m->ws_bytes = 0;
        if (hipMalloc(&m->ws, need) != hipSuccess) return D3R_ERR_ALLOC;
        m->ws_bytes = need;
    }
    m->prof_rec.clear();
    int rc = D3R_OK;
    if (graph_forward(m, k, st, &rc)) return rc;
    return forward(m, k, st);
}

extern "C" long d3r_model_graph_replays(const d3r_model* m) { return m ? m->graph_replays : -1; }

// B pairs of two image sizes with their outputs; packed: one [B][H][W][8] payload (pts1 xyz, conf1, pts2 xyz, conf2 per pixel)
static Call pair_call(const d3r_model* m, int phases, int B, int H1, int W1, int H2, int W2, float* pts1, float* conf1, float* pts2, float* conf2, bool packed = false) {
    Call k;
    k.phases = phases; k.B = B; k.d[0] = side_dim(H1, W1, m->cfg.patch_size); k.d[1] = side_dim(H2, W2, m->cfg.patch_size);
    k.pts[0] = pts1; k.conf[0] = conf1; k.pts[1] = pts2; k.conf[1] = conf2;
    if (packed) k.pstride = k.cstride = 8;
    return k;
}
static int run_forward(d3r_model* m, Call k, const float* img1, const float* img2, void* stream) {
    k.img1 = img1; k.img2 = img2; k.nimg1 = k.B; k.nimg = 2 * k.B;
    return run_phases(m, k, (hipStream_t)stream);
}
static int run_decode(d3r_model* m, Call k, const void* feat, void* stream) {
    k.feat = const_cast<void*>(feat);
    return run_phases(m, k, (hipStream_t)stream);
}

extern "C" int d3r_model_forward(d3r_model* m, const float* img1, const float* img2, int B, int H, int W, float* pts1, float* conf1,
                                 float* pts2, float* conf2, void* stream) {
    if (!m || !img1 || !img2 || B <= 0 || !pts1 || !conf1 || !pts2 || !conf2) return D3R_ERR_INVALID;
    return run_forward(m, pair_call(m, PH_ENCODE | PH_DECODE, B, H, W, H, W, pts1, conf1, pts2, conf2), img1, img2, stream);
}

extern "C" int d3r_model_forward_mixed(d3r_model* m, const float* img1, int H1, int W1, const float* img2, int H2, int W2, int B, float* pts1,
                                       float* conf1, float* pts2, float* conf2, void* stream) {
    if (!m || !img1 || !img2 || B <= 0 || !pts1 || !conf1 || !pts2 || !conf2) return D3R_ERR_INVALID;
    return run_forward(m, pair_call(m, PH_ENCODE | PH_DECODE, B, H1, W1, H2, W2, pts1, conf1, pts2, conf2), img1, img2, stream);
}

extern "C" int d3r_model_forward_packed(d3r_model* m, const float* img1, const float* img2, int B, int H, int W, float* out8, void* stream) {
    if (!m || !img1 || !img2 || B <= 0 || !out8) return D3R_ERR_INVALID;
    return run_forward(m, pair_call(m, PH_ENCODE | PH_DECODE, B, H, W, H, W, out8, out8 + 3, out8 + 4, out8 + 7, true), img1, img2, stream);
}

extern "C" size_t d3r_model_feature_bytes(const d3r_model* m, int H, int W) {
    if (!m || H <= 0 || W <= 0) return 0;
    const int ps = m->cfg.patch_size;
    return (size_t)(H / ps) * (W / ps) * m->cfg.enc_embed_dim * dt_bytes(m->dt);
}

extern "C" int d3r_model_encode(d3r_model* m, const float* img, int n, int H, int W, void* feat_out, void* stream) {
    if (!m || !img || n <= 0 || !feat_out) return D3R_ERR_INVALID;
    Call k = pair_call(m, PH_ENCODE, 0, H, W, H, W, nullptr, nullptr, nullptr, nullptr);
    k.img1 = img; k.nimg1 = k.nimg = n; k.feat = feat_out;
    return run_phases(m, k, (hipStream_t)stream);
}

extern "C" int d3r_model_decode(d3r_model* m, const void* feat, int B, int H, int W, float* pts1, float* conf1, float* pts2, float* conf2,
                                void* stream) {
    if (!m || !feat || B <= 0 || !pts1 || !conf1 || !pts2 || !conf2) return D3R_ERR_INVALID;
    return run_decode(m, pair_call(m, PH_DECODE, B, H, W, H, W, pts1, conf1, pts2, conf2), feat, stream);
}

extern "C" int d3r_model_decode_packed(d3r_model* m, const void* feat, int B, int H, int W, float* out8, void* stream) {
    if (!m || !feat || B <= 0 || !out8) return D3R_ERR_INVALID;
    return run_decode(m, pair_call(m, PH_DECODE, B, H, W, H, W, out8, out8 + 3, out8 + 4, out8 + 7, true), feat, stream);
}
