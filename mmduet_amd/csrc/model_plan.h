// model_plan.h -- what a context is built from, and nothing else: the configuration checks and derived dimensions (model_dims), the checkpoint tensors and the fused
// layouts they become (weight_plan), every workspace and pinned buffer (workspace_plan).  Pure host functions: no GPU header, no runtime call, no environment; it compiles with
// the host C++17 compiler alone (tests/test_model_plan_host.py walks tests/model_plan_cases.py through it without a GPU).  mmd_create copies model_dims(),
// mmd_finalize_weights checks and then executes weight_plan() entry by entry, alloc_workspaces allocates workspace_plan(); model.hip keeps the launches and one
// name-to-field map.
#pragma once
#include <stdio.h>
#include <string>
#include <vector>
#include "step_plan.h"          // STEP_MULTI_ATTN_MAX_RUN; through gemm_plan.h: round_up, GEMV_CHAIN_ROWS / GEMV_SSQ_STRIDE, the MMD_ codes

// ---- configuration ----------------------------------------------------------------------------------------------------
struct ModelDims {
    int rc = MMD_OK; const char* error = "";          // rc != MMD_OK: mmd_create refuses with this message (the first failing check)
    int vit_grid = 0, vit_tokens = 0, vit_seq = 0;    // patches per side, grid^2, tower sequence length (+ 1 with a class token)
    int vit_kpad = 0, vit_ipad = 0;                   // patch-embedding columns 3 P^2 and fc1 rows / fc2 columns, padded to 64
    int qkv_w = 0;                                    // rows of the fused q|k|v projection (0: no decoder)
};
static inline ModelDims model_dims(const mmd_config* cfg) {
    ModelDims d;
    auto no = [&](const char* why) { d.rc = MMD_EINVAL; d.error = why; return d; };
    if (!cfg) return no("null argument");
    if (cfg->struct_size != (int32_t)sizeof(mmd_config)) return no("mmd_config size mismatch (ABI)");
    if (cfg->dtype != MMD_F32 && cfg->dtype != MMD_BF16) return no("unsupported dtype");
    if (cfg->weight_dtype != MMD_W_DTYPE && (cfg->weight_dtype != MMD_W_FP8_E4M3 || cfg->dtype != MMD_BF16)) return no("weight_dtype fp8_e4m3 needs a bf16 context");
    if (!cfg->vision_only && (cfg->num_heads % cfg->num_kv_heads != 0 || cfg->head_dim % 2 != 0 || cfg->head_dim > 128)) return no("unsupported head configuration");
    if (cfg->vit_hidden % cfg->vit_heads != 0 || cfg->vit_hidden / cfg->vit_heads > 128) return no("unsupported ViT head configuration");
    if (cfg->tower_f16 && (cfg->dtype != MMD_BF16 || cfg->vision_only || cfg->vit_class_token || cfg->vit_pre_layernorm || cfg->vit_act != 0 || cfg->vit_pool_head ||
                           (cfg->vit_hidden % 64) != 0 || ((cfg->vit_hidden / cfg->vit_heads) % 8) != 0))
        return no("tower_f16 needs a bf16 context and the LLaVA SigLIP tower form (no class token / pre-LN / pooling head, hidden % 64 == 0, head_dim % 8 == 0)");
    if (cfg->tower_f16 < 0 || cfg->tower_f16 > 2 || (cfg->tower_f16 == 1 && (cfg->vit_post_layernorm || cfg->vit_hidden > 2048)))
        return no("tower_f16: 0 | 1 (autocast: fp32 residual stream; no post_layernorm, hidden <= 2048) | 2 (fp16 residual stream)");
    d.vit_grid = cfg->vit_image / cfg->vit_patch;
    d.vit_tokens = d.vit_grid * d.vit_grid;
    d.vit_seq = d.vit_tokens + (cfg->vit_class_token ? 1 : 0);
    d.vit_kpad = (int)round_up(3 * cfg->vit_patch * cfg->vit_patch, 64);
    d.vit_ipad = (int)round_up(cfg->vit_intermediate, 64);
    d.qkv_w = cfg->vision_only ? 0 : (cfg->num_heads + 2 * cfg->num_kv_heads) * cfg->head_dim;
    return d;
}
static inline size_t model_elem_size(const mmd_config& g) { return g.dtype == MMD_F32 ? 4 : 2; }

// ---- weights ------------------------------------------------------------------------------------------------------------
// a checkpoint name as the plan spells it: the LLaVA tower's two prefixes become "vit."
static inline std::string canon_name(const char* name) {
    std::string n(name);
    const std::string a = "model.vision_tower.vision_tower.vision_model.", b = "model.vision_tower.vision_tower.";
    if (n.compare(0, a.size(), a) == 0) return "vit." + n.substr(a.size());
    if (n.compare(0, b.size(), b) == 0) return "vit." + n.substr(b.size());
    return n;
}
// MFMA-fragment-major copies (weight-streaming GEMMs): one exists in a bf16 context when the shape tiles; the row-major original is dropped when every GEMM regime can run
// from the packed copy alone (gemv16 / skinny / big kernels) -- one copy of the weights in HBM (15.8 GB instead of 31 GB for the 7B model)
static inline bool weight_packs(int dtype, int64_t N, int64_t K) { return dtype == MMD_BF16 && (N % 16) == 0 && (K % 32) == 0; }
static inline bool weight_releases(int dtype, int64_t N, int64_t K) { return weight_packs(dtype, N, K) && (N % 64) == 0 && (K % 64) == 0; }

enum { W_ALIAS = 0,             // the loaded tensor itself becomes the destination
       W_CAT_ROWS = 1,          // the sources one after the other (q | k | v, the two video heads)
       W_INTERLEAVE16 = 2,      // gate and up in alternating blocks of 16 rows: [2 I, H]
       W_PAD_COLS = 3,          // [N, numel / N] -> [N, K], zero columns behind (patch embedding, fc2: K tile-aligned)
       W_PAD_ROWS = 4,          // the source, then zero rows up to N (fc1 and its bias: gelu(0) = 0 keeps the result exact)
       W_SPLIT_QKV = 5 };       // nn.MultiheadAttention's in_proj: rows [0, N) -> field, rows [N, N + N2) -> field2
enum { PACK_NONE = 0, PACK_KEEP = 1, PACK_RELEASE = 2 };          // the packed copy goes to <field>_p; PACK_RELEASE drops the original when weight_releases()
enum { IN_CTX = 0, IN_LLM_LAYER = 1, IN_VIT_LAYER = 2 };          // whose member `field` names: mmd_ctx, LlmLayer[layer], VitLayer[layer]
struct WeightSrc { std::string name; int64_t numel; };          // element count only, as take() always checked: not per dimension
struct WeightEntry {
    int scope = IN_CTX, layer = 0; const char* field = ""; const char* field2 = nullptr;
    int op = W_ALIAS; std::vector<WeightSrc> src;
    int64_t N = 0, K = 1, N2 = 0;          // destination [N, K] (vectors: K = 1)
    bool zero = false;                     // zero-filled before it is written
    int pack = PACK_NONE;
    bool fp8 = false;                      // quantised in place per output channel; e4m3 fragment-major copy in <field>_8, scales in s<field without its w>
    bool counted = false;                  // a matrix of mmd_weight_bytes
    bool release = false;                  // release point: behind this entry the sources consumed since the last one (aliases apart) are freed
    std::string refusal;                   // not empty: finalize refuses (MMD_EINVAL) once this entry's sources were found
};
struct WeightPlan {
    std::vector<WeightEntry> entries;
    // mmd_weight_bytes has always counted a projector (H C + H H elements) for a vision-only context too, which has none: the number is reported, never used for sizing
    int64_t phantom_elems = 0;
    int64_t weight_bytes(const mmd_config& g) const {
        int64_t n = phantom_elems * (int64_t)model_elem_size(g);
        for (const WeightEntry& w : entries) if (w.counted) n += w.N * w.K * ((int64_t)model_elem_size(g) + (w.fp8 ? 1 : 0));          // (fp8: plus the 1-byte copy)
        return n;
    }
};
// Dropped by finalize, not named here: whatever else was loaded -- vit.post_layernorm.* without vit_post_layernorm, vit.head.* without vit_pool_head, encoder layers
// beyond vit_layers, a checkpoint's other modules.
static inline WeightPlan weight_plan(const mmd_config& g, const ModelDims& m) {
    WeightPlan p;
    const int64_t H = g.hidden_size, I = g.intermediate_size, V = g.vocab_size, q = (int64_t)g.num_heads * g.head_dim, kv = (int64_t)g.num_kv_heads * g.head_dim;
    const int64_t C = g.vit_hidden, CI = g.vit_intermediate, KP = 3 * g.vit_patch * g.vit_patch;
    const bool fp8 = g.weight_dtype == MMD_W_FP8_E4M3;
    int scope = IN_CTX, layer = 0; std::string pre;          // where add() puts an entry and what its source names start with
    auto add = [&](const char* field, int op, std::vector<WeightSrc> src, int64_t N, int64_t K = 1, int pack = PACK_NONE, bool counted = false) -> WeightEntry& {
        WeightEntry w; w.scope = scope; w.layer = layer; w.field = field; w.op = op; w.N = N; w.K = K; w.pack = pack; w.counted = counted;
        for (WeightSrc& s : src) s.name = pre + s.name;
        w.src = std::move(src); p.entries.push_back(std::move(w)); return p.entries.back();
    };
    auto vec = [&](const char* field, const char* name, int64_t n) -> WeightEntry& { return add(field, W_ALIAS, {{name, n}}, n); };
    if (!g.vision_only) {
        add("embed", W_ALIAS, {{"model.embed_tokens.weight", V * H}}, V, H, PACK_NONE, true);
        vec("fnorm", "model.norm.weight", H);
        add("lm_head", W_ALIAS, {{"lm_head.weight", V * H}}, V, H, PACK_KEEP, true);
        WeightEntry& h4 = add("heads4", W_CAT_ROWS, {{"informative_head.weight", 2 * H}, {"relevance_head.weight", 2 * H}}, 4, H); h4.zero = h4.release = true;
        scope = IN_LLM_LAYER;
        for (layer = 0; layer < g.num_layers; ++layer) {          // one decoder layer
            pre = "model.layers." + std::to_string(layer) + ".";
            std::string bad8;          // the first matrix fp8 cannot take: refused where the layer's last matrix is, as the quantisation ran behind the layer's takes
            auto mat = [&](const char* field, int op, std::vector<WeightSrc> src, int64_t N, int64_t K) -> WeightEntry& {
                WeightEntry& w = add(field, op, std::move(src), N, K, PACK_RELEASE, true); w.fp8 = fp8;
                if (fp8 && bad8.empty() && ((N % 16) != 0 || (K % 64) != 0)) {
                    char b[96]; snprintf(b, sizeof(b), "fp8 weights need N %% 16 == 0 and K %% 64 == 0 (got %d x %d)", (int)N, (int)K); bad8 = b; }
                return w;
            };
            vec("ln1", "input_layernorm.weight", H); vec("ln2", "post_attention_layernorm.weight", H);
            mat("wqkv", W_CAT_ROWS, {{"self_attn.q_proj.weight", q * H}, {"self_attn.k_proj.weight", kv * H}, {"self_attn.v_proj.weight", kv * H}}, m.qkv_w, H);
            add("bqkv", W_CAT_ROWS, {{"self_attn.q_proj.bias", q}, {"self_attn.k_proj.bias", kv}, {"self_attn.v_proj.bias", kv}}, m.qkv_w);
            mat("wo", W_ALIAS, {{"self_attn.o_proj.weight", H * q}}, H, q);
            WeightEntry& gu = mat("wgu", W_INTERLEAVE16, {{"mlp.gate_proj.weight", I * H}, {"mlp.up_proj.weight", I * H}}, 2 * I, H);
            if (I % 16) { char b[96]; snprintf(b, sizeof(b), "intermediate_size must be a multiple of 16 (got %d)", (int)I); gu.refusal = b; }
            WeightEntry& dn = mat("wdown", W_ALIAS, {{"mlp.down_proj.weight", H * I}}, H, I); dn.release = true; dn.refusal = bad8;
        }
    }
    scope = IN_CTX; layer = 0; pre = "vit.";
    { WeightEntry& w = add("patch_w", W_PAD_COLS, {{"embeddings.patch_embedding.weight", C * KP}}, C, m.vit_kpad, PACK_KEEP, true); w.release = true; }
    vec("patch_b", "embeddings.patch_embedding.bias", C);
    add("pos_emb", W_ALIAS, {{"embeddings.position_embedding.weight", m.vit_seq * C}}, m.vit_seq, C);
    if (g.vit_class_token) vec("cls_emb", "embeddings.class_embedding", C);
    if (g.vit_pre_layernorm) { vec("pre_w", "pre_layrnorm.weight", C); vec("pre_b", "pre_layrnorm.bias", C); }
    scope = IN_VIT_LAYER;
    for (layer = 0; layer < g.vit_layers; ++layer) {          // one tower layer
        pre = "vit.encoder.layers." + std::to_string(layer) + ".";
        vec("ln1w", "layer_norm1.weight", C); vec("ln1b", "layer_norm1.bias", C); vec("ln2w", "layer_norm2.weight", C); vec("ln2b", "layer_norm2.bias", C);
        add("wqkv", W_CAT_ROWS, {{"self_attn.q_proj.weight", C * C}, {"self_attn.k_proj.weight", C * C}, {"self_attn.v_proj.weight", C * C}}, 3 * C, C, PACK_RELEASE, true);
        add("bqkv", W_CAT_ROWS, {{"self_attn.q_proj.bias", C}, {"self_attn.k_proj.bias", C}, {"self_attn.v_proj.bias", C}}, 3 * C);
        add("wo", W_ALIAS, {{"self_attn.out_proj.weight", C * C}}, C, C, PACK_RELEASE, true); vec("bo", "self_attn.out_proj.bias", C);
        add("w1", W_PAD_ROWS, {{"mlp.fc1.weight", CI * C}}, m.vit_ipad, C, PACK_RELEASE, true).zero = true;
        add("b1", W_PAD_ROWS, {{"mlp.fc1.bias", CI}}, m.vit_ipad).zero = true;
        add("w2", W_PAD_COLS, {{"mlp.fc2.weight", C * CI}}, C, m.vit_ipad, PACK_RELEASE, true);
        vec("b2", "mlp.fc2.bias", C).release = true;
    }
    scope = IN_CTX; layer = 0; pre = "vit.";
    if (g.vit_post_layernorm) { vec("post_w", "post_layernorm.weight", C); vec("post_b", "post_layernorm.bias", C); }
    if (!g.vision_only) {
        pre = "model.mm_projector.";
        add("p0w", W_ALIAS, {{"0.weight", H * C}}, H, C, PACK_KEEP, true); vec("p0b", "0.bias", H);
        add("p2w", W_ALIAS, {{"2.weight", H * H}}, H, H, PACK_KEEP, true); vec("p2b", "2.bias", H);
    } else p.phantom_elems = H * C + H * H;
    if (g.vit_pool_head) {          // SiglipMultiheadAttentionPoolingHead: nn.MultiheadAttention keeps q/k/v stacked in in_proj_weight [3C, C]
        pre = "vit.head.";
        vec("hd_probe", "probe", C);
        { WeightEntry& w = add("hd_wq", W_SPLIT_QKV, {{"attention.in_proj_weight", 3 * C * C}}, C, C); w.field2 = "hd_wkv"; w.N2 = 2 * C; }
        { WeightEntry& w = add("hd_bq", W_SPLIT_QKV, {{"attention.in_proj_bias", 3 * C}}, C); w.field2 = "hd_bkv"; w.N2 = 2 * C; w.release = true; }
        add("hd_wo", W_ALIAS, {{"attention.out_proj.weight", C * C}}, C, C); vec("hd_bo", "attention.out_proj.bias", C);
        vec("hd_lnw", "layernorm.weight", C); vec("hd_lnb", "layernorm.bias", C);
        add("hd_w1", W_ALIAS, {{"mlp.fc1.weight", CI * C}}, CI, C); vec("hd_b1", "mlp.fc1.bias", CI);
        add("hd_w2", W_ALIAS, {{"mlp.fc2.weight", C * CI}}, C, CI); vec("hd_b2", "mlp.fc2.bias", C);
    }
    return p;
}
// The check finalize makes before it consumes anything, in plan order.  numel_of(name): elements of the loaded tensor, < 0 when there is none.
struct WeightRefusal { int rc = MMD_OK; std::string error; };
template <class F> static inline WeightRefusal weight_plan_check(const WeightPlan& p, F numel_of) {
    WeightRefusal r; char b[256];
    for (const WeightEntry& w : p.entries) {
        for (const WeightSrc& s : w.src) {
            const long long n = numel_of(s.name);
            if (n < 0) { r.rc = MMD_ENOENT; snprintf(b, sizeof(b), "missing weight tensor '%s'", s.name.c_str()); r.error = b; return r; }
            if (n != s.numel) { r.rc = MMD_EINVAL; snprintf(b, sizeof(b), "weight '%s' has %lld elements, expected %lld", s.name.c_str(), n, (long long)s.numel); r.error = b; return r; }
        }
        if (!w.refusal.empty()) { r.rc = MMD_EINVAL; r.error = w.refusal; return r; }
    }
    return r;
}

// ---- workspaces -----------------------------------------------------------------------------------------------------------
// fp32 split-K slab workspace of the LLM side: 64 MB; 192 MB for a model built for several streams' merged chunks (three slabs of a 2548-row down_proj are 110 MB)
static inline size_t model_splitk_bytes(const mmd_config& g) { return (size_t)(g.max_step_tokens > 2048 ? 192 : 64) << 20; }
constexpr size_t MODEL_ATTN_WS_BYTES = (size_t)128 << 20;          // split-KV partials of the LLM side
constexpr size_t MODEL_TOWER_WS_BYTES = (size_t)32 << 20;          // the tower runs on a side stream next to LLM steps: its own split-K and split-KV scratch, each this size
constexpr int MODEL_PREV_CAP = 16384;                              // ids of the repetition-penalty list at first (it grows)
struct WorkspaceEntry { const char* field; size_t bytes; bool pinned; };          // device buffers are zero-filled, pinned host buffers are not
struct WorkspacePlan {
    std::vector<WorkspaceEntry> entries;
    size_t splitk_bytes = 0, attn_bytes = 0, v_splitk_bytes = 0, v_attn_bytes = 0;          // the capacities the GEMM and attention planners are handed
    int64_t v_h32_rows = 0; int prev_cap = 0;
};
// step_state_bytes: sizeof(StepState) (common.h)
static inline WorkspacePlan workspace_plan(const mmd_config& g, const ModelDims& m, size_t step_state_bytes) {
    WorkspacePlan p;
    const size_t e = model_elem_size(g), C = g.vit_hidden, H = g.hidden_size, Bm = g.max_vit_batch;
    const size_t Mv = (size_t)round_up((int64_t)g.max_vit_batch * m.vit_seq, 128);
    auto dev = [&](const char* field, size_t bytes) { p.entries.push_back({field, bytes, false}); };
    auto pin = [&](const char* field, size_t bytes) { p.entries.push_back({field, bytes, true}); };
    dev("v_col", Mv * m.vit_kpad * e); dev("v_h", Mv * C * e); dev("v_xn", Mv * C * e);
    if (g.tower_f16 == 1) {          // the autocast tower's fp32 residual stream: Mv rows + the compact rows of the sparse last layer
        const size_t pout = (m.vit_grid + g.pool_stride - 1) / g.pool_stride;
        p.v_h32_rows = (int64_t)Mv; dev("v_h32", (Mv + Bm * 4 * pout * pout) * C * sizeof(float));
    }
    dev("v_qkv", Mv * 3 * C * e); dev("v_attn", Mv * C * e); dev("v_mlp", (size_t)round_up(Mv, 16) * m.vit_ipad * e);          // (rows padded to 16: the piece-major form of fc1's output holds whole 16-row pieces)
    if (g.vit_class_token) dev("v_patch", Mv * C * e);
    p.v_splitk_bytes = p.v_attn_bytes = MODEL_TOWER_WS_BYTES; dev("v_splitk_ws", p.v_splitk_bytes); dev("v_attn_ws", p.v_attn_bytes);
    if (g.vit_pool_head) {
        dev("hd_q", C * e); dev("hd_kv", Mv * 2 * C * e); dev("hd_a", Bm * C * e); dev("hd_h", Bm * C * e); dev("hd_n", Bm * C * e); dev("hd_m", Bm * g.vit_intermediate * e);
    }
    if (g.vision_only) return p;
    dev("v_p1", Mv * H * e); dev("v_p2", Mv * H * e);
    const size_t S = (size_t)round_up(g.max_step_tokens, 128), qw = (size_t)g.num_heads * g.head_dim, seg = 8 * STEP_MULTI_ATTN_MAX_RUN * step_state_bytes;
    dev("l_h", S * H * e); dev("l_xn", S * H * e); dev("l_qkv", S * m.qkv_w * e); dev("l_q", S * qw * e); dev("l_attn", S * qw * e);
    dev("l_act", (size_t)round_up(S, 16) * g.intermediate_size * e); dev("l_hid", S * H * e);          // (l_act rows padded to 16: whole pieces in its piece-major form)
    p.splitk_bytes = model_splitk_bytes(g); dev("splitk_ws", p.splitk_bytes);
    dev("chain_ssq", (size_t)GEMV_CHAIN_ROWS * GEMV_SSQ_STRIDE * sizeof(float)); dev("rope_tab", S * 64 * 2 * sizeof(float));          // (cos, sin) of a step's positions: decode steps and chunks
    p.attn_bytes = MODEL_ATTN_WS_BYTES; dev("attn_ws", p.attn_bytes);
    dev("logits_ws", (size_t)g.vocab_size * sizeof(float)); dev("heads_dev", S * 4 * sizeof(float)); dev("rows_dev", S * sizeof(int32_t));
    dev("tok_dev", 64); dev("argmax_scratch", 1024); p.prev_cap = MODEL_PREV_CAP; dev("prev_dev", (size_t)p.prev_cap * sizeof(int64_t)); dev("gen_embed", H * e);
    pin("heads_host", S * 4 * sizeof(float)); pin("rows_host", S * sizeof(int32_t)); pin("tok_host", 64); pin("step_host", step_state_bytes); pin("seg_host", seg);
    dev("seg_dev", seg); dev("step_dev", step_state_bytes);
    return p;
}
