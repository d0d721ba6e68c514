// model.hip -- context, weights, KV arena and the forward orchestration behind the C ABI (include/mmduet.h).
//
// Host-side control only: every arithmetic step is a HIP kernel from gemm.hip / attn.hip / ops.hip launched on the
// context's stream.  Reference call chain this file stands in for:
//   LiveMixin.visual_embed (models/modeling_live.py:26-33) -> mmd_vit_encode
//   VideoHeadLiveLlavaQwenForCausalLM.forward (models/live_llava/video_head_live_llava_qwen.py:121-205) -> mmd_llm_step +
//       mmd_video_heads + mmd_lm_head
//   fast_greedy_generate (models/modeling_live.py:51-77) -> mmd_greedy_generate
#include "common.h"
#include "step_plan.h"
#include "tower_plan.h"
#include "select_plan.h"
#include "kv_plan.h"
#include "pixel_taps.h"
#include "model_plan.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

static thread_local std::string g_create_error;

struct RawTensor { void* p = nullptr; std::vector<int64_t> shape; int64_t numel = 0; };

struct Prof {
    unsigned on = 0;                   // bitmask over MMD_K_* classes
    int stride = 1;                    // bracket every stride-th launch of an enabled class (event records are not free)
    int64_t seen[MMD_K_COUNT] = {0};
    std::vector<hipEvent_t> pool;
    struct Pending { hipEvent_t a, b; int kind; };
    std::vector<Pending> pending;
    double ms[MMD_K_COUNT] = {0}; int64_t n[MMD_K_COUNT] = {0}; double bytes[MMD_K_COUNT] = {0}; double flops[MMD_K_COUNT] = {0};
};

static_assert(SELECT_ROUND_MAX_ROWS == MMD_ROUND_MAX_SAMPLERS, "select_plan.h restates the rows of one launch");
enum { SELECT_OF_OP = 0, SELECT_OF_GENERATE = 1, SELECT_OF_ROUND = 2 };
constexpr int SELECT_LAST_FIELDS = SELECT_PLAN_FIELDS + 1 + GENERATE_PLAN_FIELDS;          // (a RoundBlocks is the shorter tail)
static_assert(ROUND_BLOCKS_FIELDS <= GENERATE_PLAN_FIELDS, "the tail of select_last holds either");

// The state of a response in progress (response_plan.h holds its rules, DESIGN.md "Response state" who owns what).  The context has one for its generate calls, every sampler
// one for its rounds; the helpers below (response_*) are the only code that sizes, fills or frees these buffers.
struct Response {
    int64_t* prev_dev = nullptr; int prev_cap = 0; float penalty = 0.f;          // repetition-penalty list (device), its capacity, the penalty (0: off)
    ConsSet cons; int32_t* cons_ids_dev = nullptr; float* cons_bias_dev = nullptr;          // the validated set and its table on the device (allocated with the first set that is on)
    int lp_top = -1, lp_cap = 0; LogprobRec* lp_rec = nullptr;          // log-probabilities: the setting (-1 off), the device records of the current response
    ResponseCount count;
    bool zero_fill = false;            // the context's buffers are zero-filled when they are (re)placed, as its workspaces are; a sampler's never were
};

// one captured decode step: the instantiated graph, its source, and the (penalty, EOS, filter selection) it was captured for
struct DecodeGraph {
    hipGraphExec_t exec = nullptr; hipGraph_t src = nullptr;
    float pen = 0.f; int64_t eos = 0; int sel = 0; int lp = -1;          // lp: log-probability recording of the step (-1 off, else its top_n)
    uint32_t cons = 0;          // constraints: 0 the step was captured without, 1 with (its sets are read from device memory)
    void drop() {
        if (exec) { hipGraphExecDestroy(exec); exec = nullptr; }
        if (src) { hipGraphDestroy(src); src = nullptr; }
    }
};

struct LlmLayer { void *ln1 = 0, *ln2 = 0, *wqkv = 0, *bqkv = 0, *wo = 0, *wgu = 0, *wdown = 0;
                  void *wqkv_p = 0, *wo_p = 0, *wgu_p = 0, *wdown_p = 0;       // *_p: MFMA-fragment-major copies (skinny GEMM)
                  void *wqkv_8 = 0, *wo_8 = 0, *wgu_8 = 0, *wdown_8 = 0;       // fp8 e4m3 fragment-major copies (weight_dtype = fp8: the streaming kernels read these)
                  float *sqkv = 0, *so = 0, *sgu = 0, *sdown = 0; };          // per-output-channel scales of the quantised matrices
struct VitLayer { void *ln1w = 0, *ln1b = 0, *wqkv = 0, *bqkv = 0, *wo = 0, *bo = 0, *ln2w = 0, *ln2b = 0, *w1 = 0, *b1 = 0, *w2 = 0, *b2 = 0;
                  void *wqkv_p = 0, *wo_p = 0, *w1_p = 0, *w2_p = 0; };

struct mmd_ctx {
    mmd_config cfg;
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::string err;
    std::unordered_map<std::string, RawTensor> raw;
    std::vector<void*> allocs, host_allocs;          // every device buffer (dev_alloc) and every pinned host buffer (host_alloc) of the context: mmd_destroy frees the lists
    int64_t weight_bytes = 0;
    bool finalized = false;
    // fused weights
    std::vector<LlmLayer> L;
    std::vector<VitLayer> VL;
    void *embed = 0, *fnorm = 0, *lm_head = 0, *heads4 = 0, *lm_head_p = 0;
    void *patch_w = 0, *patch_b = 0, *pos_emb = 0, *post_w = 0, *post_b = 0, *p0w = 0, *p0b = 0, *p2w = 0, *p2b = 0;
    void *patch_w_p = 0, *p0w_p = 0, *p2w_p = 0;
    int vit_kpad = 0, vit_ipad = 0, vit_tokens = 0, vit_grid = 0, qkv_w = 0;
    int vit_seq = 0;                    // tower sequence length = vit_tokens (+ 1 with a class token, CLIP)
    void *cls_emb = 0, *pre_w = 0, *pre_b = 0, *v_patch = 0;      // CLIP: class embedding, pre_layrnorm; patch rows before the class token is spliced in
    // SigLIP attention-pooling head (pooler_output): probe, MHA in_proj split into q | kv, out_proj, LayerNorm, MLP
    void *hd_probe = 0, *hd_wq = 0, *hd_bq = 0, *hd_wkv = 0, *hd_bkv = 0, *hd_wo = 0, *hd_bo = 0, *hd_lnw = 0, *hd_lnb = 0, *hd_w1 = 0, *hd_b1 = 0, *hd_w2 = 0, *hd_b2 = 0;
    void *hd_q = 0, *hd_kv = 0, *hd_a = 0, *hd_h = 0, *hd_n = 0, *hd_m = 0;
    float* inv_freq = nullptr; bool inv_freq_user = false;
    // workspaces
    void *v_col = 0, *v_h = 0, *v_xn = 0, *v_qkv = 0, *v_attn = 0, *v_mlp = 0, *v_p1 = 0, *v_p2 = 0;
    float* v_h32 = 0; int64_t v_h32_rows = 0;          // tower_f16 == 1: the autocast tower's fp32 residual stream [Mv + compact rows of the sparse last layer, C]
    void *l_h = 0, *l_xn = 0, *l_qkv = 0, *l_q = 0, *l_attn = 0, *l_act = 0, *l_hid = 0;
    float* splitk_ws = 0; size_t splitk_bytes = 0;
    float* attn_ws = 0; size_t attn_bytes = 0;
    float* v_splitk_ws = 0; size_t v_splitk_bytes = 0;   // the tower runs on a side stream next to LLM steps: its own split-K / split-KV scratch
    float* v_attn_ws = 0; size_t v_attn_bytes = 0;
    float* logits_ws = 0;              // [V] fp32 for generation
    float* heads_dev = 0;              // [max_step_tokens,4]
    int32_t* rows_dev = 0;
    int64_t* tok_dev = 0;              // sampled token id
    void* argmax_scratch = 0;          // candidates of the two-stage argmax
    Response resp;                     // of the generate calls; resp.prev_dev is the workspace entry "prev_dev" (model_plan.h)
    void* gen_embed = 0;               // [1,H]
    // pinned staging
    float* heads_host = 0; int32_t* rows_host = 0; int64_t* tok_host = 0;
    // preprocess tables
    int lb_W = 0, lb_H = 0, lb_R = 0; int32_t* lb_xtab = 0; int32_t* lb_ytab = 0;      // letterbox tap tables (mmd_letterbox_frames)
    int pp_R = 0; int32_t* pp_coef = 0; int32_t* pp_bounds = 0; int pp_ksize = 0; uint8_t* pp_tmp = 0; size_t pp_tmp_bytes = 0;
    int last_vit_B = 0;
    // graph-captured decode steps (generate_impl): the arg-max one, keyed by penalty value and EOS, and the sampled one, keyed by penalty on/off, EOS and which filters run;
    // per-call state lives in *step_dev.  dec_route: what the most recent generate call's decode steps did (mmd_op_decode_last_route)
    StepState* step_dev = nullptr; StepState* step_host = nullptr;
    DecodeGraph dec_greedy, dec_sampled; int dec_route = 0; bool no_graph = false;
    int last_form[2] = {0, 0};          // form / splits of the most recent LLM / raw-operator attention launch of THIS context (mmd_op_attention_last_form)
    int last_plan[4] = {-1, 0, 0, 0};   // kernel / tiles / splits / blocks of the most recent gemm() (mmd_op_gemm_last_plan)
    StepSwitches sw;                   // the A/B switches of the step schedule (step_plan.h), read from the environment in mmd_create
    int step_last[STEP_PLAN_FIELDS] = {0};          // the plan of the most recent LLM step of THIS context (mmd_op_step_last_plan)
    // the SelectPlan the most recent token selection launched from, then whose it was (SELECT_OF_*) and that caller's GeneratePlan / RoundBlocks (mmd_op_select_last_plan)
    int select_last[SELECT_LAST_FIELDS] = {0};
    int tower_ring_flags = -1, tower_ring_blocks = 0;   // mmd_set_tower_share: persistent-grid cap of the tower's ring GEMMs beside a response's decoding
    int hid_compact = 0;               // > 0: l_hid holds that many compact rows (in the order of the `need` list) instead of all S rows of the step
    bool full_tower = false;           // mmd_vit_set_full_tower(1): the last encoder layer runs on ALL tokens (feature extraction, debug taps); default: on the tokens the bilinear pool reads
    TowerPlan tower_last;              // the plan of the most recent tower run of THIS context (mmd_op_tower_last_plan): the projector behind it and the debug taps read it
    void* rope_tab = 0;                // (cos, sin) of a decode step's positions (launch_rope_table), read by the attention kernel's fused q/k/v preparation
    float* chain_ssq = 0;              // GemvChain scratch: per-row, per-n-tile sums of squares
    StepState* seg_dev = nullptr; StepState* seg_host = nullptr; int seg_slot = 0;          // per-stream (context, capacity, arena) of a step's batched decode attention: 8 slots of 64, rotated per step
    hipEvent_t seg_event[8] = {};      // recorded behind a slot's upload: the pinned host slot is rewritten only once that copy has run (steps without a synchronisation may queue up)
    // mmd_round_multi (allocated at its first use): logits of the sampling rows, their gathered hidden rows, the two-stage argmax candidates, the drawn tokens
    float* round_logits = 0; void* round_hidden = 0; void* round_scratch = 0; int64_t* round_toks_dev = 0; int64_t* round_toks_host = 0;
    // ... and, at the first round with a recording sampler: one record destination per logits row (device, pinned staging), the record kernels' scratch for a round's rows;
    // what the most recent round recorded (mmd_op_round_last_record)
    LogprobRow* round_lp_rows_dev = nullptr; LogprobRow* round_lp_rows_host = nullptr; void* round_lp_scratch = nullptr;
    int round_record_last[ROUND_RECORD_FIELDS] = {0, 0, 0, -1};
    // mmd_lm_nll (allocated at its first use): one fp32 logit chunk [rows, chunk columns], the rows' (max, sum exp, label logit) and the one-writer partials of a chunk's reduce
    float* nll_ws = 0; size_t nll_ws_bytes = 0; float* nll_state = 0; float* nll_part = 0; int nll_rows = 0;
    // sampled decoding (allocated at its first use): row descriptors on the device ([0] mmd_sample_generate's, [1..] a round's) with their pinned staging, the chain's scratch
    // for MMD_ROUND_MAX_SAMPLERS rows
    SampleRow* samp_rows_dev = nullptr; SampleRow* samp_rows_host = nullptr; void* samp_scratch = nullptr;
    uint32_t sample_lane = 0; uint32_t n_samplers = 0;
    // log-probabilities of generated tokens (mmd_set_generate_logprobs): resp.count.lp_n records of the most recent generate call are valid, with lp_call_top alternatives
    // each (resp.lp_top is the setting for the next call); the record kernels' scratch for one row (allocated at its first use)
    int lp_call_top = -1; void* lp_scratch = nullptr;
    // constrained decoding (allocated at its first use): the key the captured steps carry for resp.cons (0 off, 1 on: a call that sets, generates and clears finds its step
    // again), row descriptors on the device ([0] the generate calls', [1..] a round's) with their pinned staging
    uint32_t cons_gen = 0;
    ConstraintRow* cons_rows_dev = nullptr; ConstraintRow* cons_rows_host = nullptr;
    Prof prof;
};

struct mmd_stream {
    mmd_ctx* ctx;
    void* K = nullptr; void* V = nullptr;      // [layers][nkv][cap][d]   (cap = the row STRIDE in tokens)
    int64_t cap = 0, len = 0;
    int64_t pos_off = 0;                       // tokens dropped in front of the live ones (mmd_kv_drop): the RoPE position of slot t is t + pos_off for every token written from now on
    // virtual-memory arena (default): K / V are address ranges reserved for `cap` tokens per (layer, kv head) row; physical pages back only the
    // first `mapped` tokens of every row and are added chunk by chunk -- growth copies nothing and never needs a second arena
    bool vmm = false;
    int64_t mapped = 0, chunk_tokens = 0;
    size_t va_bytes = 0;
    std::vector<hipMemGenericAllocationHandle_t> handles;
    std::vector<std::pair<void*, size_t>> maps;
    // stash of a token range (mmd_kv_stash / mmd_kv_unstash)
    void* stash_k = nullptr; void* stash_v = nullptr; size_t stash_bytes = 0; int64_t stash_from = -1, stash_to = -1;
};

#define FAIL(ctx, code, ...) do { char _b[512]; snprintf(_b, sizeof(_b), __VA_ARGS__); (ctx)->err = _b; return (code); } while (0)
#define HIPCHK(ctx, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { FAIL(ctx, MMD_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); } } while (0)

static size_t es(const mmd_ctx* c) { return dtype_size(c->cfg.dtype); }

static int dev_alloc(mmd_ctx* c, void** out, size_t bytes, bool zero = true) {
    if (bytes == 0) bytes = 16;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) FAIL(c, MMD_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    if (zero) { e = hipMemsetAsync(p, 0, bytes, c->stream); if (e != hipSuccess) FAIL(c, MMD_EHIP, "memset failed"); }
    c->allocs.push_back(p);
    *out = p;
    return MMD_OK;
}
static int host_alloc(mmd_ctx* c, void** out, size_t bytes) {
    HIPCHK(c, hipHostMalloc(out, bytes));
    c->host_allocs.push_back(*out);
    return MMD_OK;
}
static void dev_free(mmd_ctx* c, void* p) {
    if (!p) return;
    for (size_t i = 0; i < c->allocs.size(); ++i) if (c->allocs[i] == p) { c->allocs[i] = c->allocs.back(); c->allocs.pop_back(); break; }
    hipFree(p);
}

// ---- a response's buffers (response_plan.h: the rules; struct Response: the fields) ----------------------------------------------------------------------------
// `buf` [cap entries of elem bytes] must hold `need`: grown by doubling behind a drained stream (a step or a round in flight may still read or write the old buffer).
// *moved is set when the old buffer is gone, whatever the answer -- the context drops its captured decode steps, which hold the pointer; a sampler has nothing to drop.
static int response_grow(mmd_ctx* c, const Response& r, void** buf, int* cap, int need, int first, size_t elem, bool* moved) {
    const int ncap = grow_capacity(*cap, need, first);
    if (ncap == *cap) return MMD_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (moved) *moved = true;
    dev_free(c, *buf); *buf = nullptr; *cap = 0;
    int rc = dev_alloc(c, buf, (size_t)ncap * elem, r.zero_fill); if (rc) return rc;
    *cap = ncap;
    return MMD_OK;
}
static int response_reserve_list(mmd_ctx* c, Response& r, int need, int first, bool* moved = nullptr) { return response_grow(c, r, (void**)&r.prev_dev, &r.prev_cap, need, first, sizeof(int64_t), moved); }
static int response_reserve_records(mmd_ctx* c, Response& r, int need, int first, bool* moved = nullptr) { return response_grow(c, r, (void**)&r.lp_rec, &r.lp_cap, need, first, sizeof(LogprobRec), moved); }
// a validated set becomes the response's: its table goes to the device first.  The stream is drained before the upload (a step in flight may read the old values), then the
// copy is synchronous -- no staging of pageable memory behind the caller's back
static int response_set_constraints(mmd_ctx* c, Response& r, const ConsSet& s) {
    if (s.on && !r.cons_bias_dev) {
        int rc = dev_alloc(c, (void**)&r.cons_ids_dev, CONS_MAX_TABLE * sizeof(int32_t), r.zero_fill); if (rc) return rc;
        rc = dev_alloc(c, (void**)&r.cons_bias_dev, CONS_MAX_TABLE * sizeof(float), r.zero_fill); if (rc) return rc;
    }
    if (s.on && s.n > 0) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(r.cons_ids_dev, s.ids, sizeof(int32_t) * s.n, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(r.cons_bias_dev, s.bias, sizeof(float) * s.n, hipMemcpyHostToDevice));
    }
    r.cons = s;
    return MMD_OK;
}
// the record option of a response: -1 off, else the alternatives of a record.  (When a switch takes hold is its owner's business: a sampler switches at a response boundary
// and reserves at once, the context's next generate call takes the setting.)
static int response_lp_top_checked(mmd_ctx* c, int top_n) {
    if (top_n < -1 || top_n > LP_MAX_TOP) FAIL(c, MMD_ERANGE, "log-probability alternatives: -1 (off) or 0..%d, got %d", LP_MAX_TOP, top_n);
    return MMD_OK;
}
static void unpack_logprobs(const LogprobRec* h, int n, int top_n, float* lp, float* slp, int64_t* top_ids, float* top_lp) {
    for (int i = 0; i < n; ++i) {
        if (lp) lp[i] = h[i].lp;
        if (slp) slp[i] = h[i].slp;
        for (int j = 0; j < top_n; ++j) { if (top_ids) top_ids[(size_t)i * top_n + j] = h[i].top_id[j]; if (top_lp) top_lp[(size_t)i * top_n + j] = h[i].top_lp[j]; }
    }
}
// the first n records, written with top_n alternatives each, into the caller's arrays (any of them may be null)
static int response_read_records(mmd_ctx* c, const Response& r, int n, int top_n, float* lp, float* slp, int64_t* top_ids, float* top_lp, int cap_tokens) {
    if (cap_tokens < n) FAIL(c, MMD_ERANGE, "%d records, room for %d", n, cap_tokens);
    std::vector<LogprobRec> h((size_t)n);
    HIPCHK(c, hipMemcpyAsync(h.data(), r.lp_rec, sizeof(LogprobRec) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unpack_logprobs(h.data(), n, top_n, lp, slp, top_ids, top_lp);
    return MMD_OK;
}
static void response_release(mmd_ctx* c, Response& r) {
    dev_free(c, r.prev_dev); dev_free(c, r.cons_ids_dev); dev_free(c, r.cons_bias_dev); dev_free(c, r.lp_rec);
    r = Response{};
}

// ---- profiling ---------------------------------------------------------------------------------------------------
struct ProfScope {
    mmd_ctx* c; int kind; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(mmd_ctx* c_, int kind_, double bytes, double flops) : c(c_), kind(kind_) {
        if (!((c->prof.on >> kind_) & 1u)) return;
        if ((c->prof.seen[kind_]++ % c->prof.stride) != 0) return;
        auto get = [&]() { hipEvent_t e; if (!c->prof.pool.empty()) { e = c->prof.pool.back(); c->prof.pool.pop_back(); } else hipEventCreate(&e); return e; };
        a = get(); b = get();
        c->prof.bytes[kind] += bytes; c->prof.flops[kind] += flops; c->prof.n[kind] += 1;
        hipEventRecord(a, c->stream);
    }
    ~ProfScope() {
        if (!a) return;
        hipEventRecord(b, c->stream);
        c->prof.pending.push_back({a, b, kind});
        // pairs that have completed are folded in as we go (hipEventQuery, no wait), so a long timed region does not pile up thousands of recorded, unread events.
        // (It does not make the sampling free: the runtime's event thread costs 0.4-0.5 CPU-s per 0.85 s step from ~5 steps on whatever the number of pending
        // pairs -- 8 steps, stride 31: 340-345 frames/s with, 343-345 without sampling; `bench.py --no-prof` is the line without it.)
        if (c->prof.pending.size() >= 32) {
            size_t done = 0;
            while (done + 8 < c->prof.pending.size() && hipEventQuery(c->prof.pending[done].b) == hipSuccess) {
                Prof::Pending& p = c->prof.pending[done];
                float ms = 0; hipEventElapsedTime(&ms, p.a, p.b);
                c->prof.ms[p.kind] += ms;
                c->prof.pool.push_back(p.a); c->prof.pool.push_back(p.b);
                ++done;
            }
            if (done) c->prof.pending.erase(c->prof.pending.begin(), c->prof.pending.begin() + done);
        }
    }
};
static void prof_drain(mmd_ctx* c) {
    if (c->prof.pending.empty()) return;
    hipStreamSynchronize(c->stream);
    for (auto& p : c->prof.pending) {
        float ms = 0; hipEventElapsedTime(&ms, p.a, p.b);
        c->prof.ms[p.kind] += ms;
        c->prof.pool.push_back(p.a); c->prof.pool.push_back(p.b);
    }
    c->prof.pending.clear();
}

// ---- GEMM wrapper --------------------------------------------------------------------------------------------------
// the GemmArgs of a GEMM in this context (tower: the side stream's split-K scratch and ring instantiation) -- the one place they are filled, for launches and for probes
static GemmArgs gemm_args(mmd_ctx* c, const void* X, int64_t ldx, const void* W, int64_t ldw, const void* bias, const void* R, int64_t ldr, void* Y, int64_t ldy, int M, int N, int K,
                          int epi, int out_f32, int variant, const void* Wp, bool tower, const void* Wp8 = nullptr, const float* wscale = nullptr) {
    GemmArgs a;
    a.X = X; a.ldx = ldx; a.W = W; a.ldw = ldw; a.Wp = Wp; a.bias = bias; a.R = R; a.ldr = ldr; a.Y = Y; a.ldy = ldy;
    a.M = M; a.N = N; a.K = K; a.epi = epi; a.out_f32 = out_f32; a.variant = variant; a.Wp8 = Wp8; a.wscale = wscale;
    a.splitk_ws = tower ? c->v_splitk_ws : c->splitk_ws; a.splitk_ws_bytes = tower ? c->v_splitk_bytes : c->splitk_bytes;
    a.plan_out = c->last_plan;
    if (tower && c->tower_ring_flags >= 0) { a.ring_flags = c->tower_ring_flags; a.ring_max_blocks = c->tower_ring_blocks; }
    return a;
}
// dt: the element type of the operands: the context's (< 0), or the tower plan's -- MMD_F16 inside the fp16 vision tower (tower_gemm)
static int gemm(mmd_ctx* c, const void* X, int64_t ldx, const void* W, int64_t ldw, const void* bias, const void* R, int64_t ldr, void* Y,
                int64_t ldy, int M, int N, int K, int epi, int out_f32 = 0, int variant = GEMM_AUTO, const void* Wp = nullptr, bool tower = false,
                const void* Wp8 = nullptr, const float* wscale = nullptr, const GemvChain* chain = nullptr, int* ring_slabs_out = nullptr, int pm = 0, int dt = -1) {
    GemmArgs a = gemm_args(c, X, ldx, W, ldw, bias, R, ldr, Y, ldy, M, N, K, epi, out_f32, variant, Wp, tower, Wp8, wscale);
    a.chain = chain; a.ring_slabs_out = ring_slabs_out; a.x_pm = pm & 1; a.y_pm = (pm >> 1) & 1;          // pm: 1 = X is piece-major, 2 = Y becomes piece-major (gemm_pair_pm, TowerPlan::mlp_pm)
    if (dt < 0) dt = c->cfg.dtype;
    const GemmPlan pl = gemm_plan_for(dt, a);          // the profiler class is that of the kernel that runs
    double e = (double)es(c);
    double bytes = (double)M * K * e + (double)N * K * ((Wp8 && M <= 64) ? 1.0 : e) + (double)M * (epi == EPI_SWIGLU ? N / 2 : N) * (out_f32 ? 4.0 : e);
    ProfScope ps(c, pl.prof_class, bytes, 2.0 * M * N * K);
    HIPCHK(c, launch_gemm(dt, a, c->stream, &pl));
    return MMD_OK;
}

// mmd_op_gemm_pair: may the intermediate between a producer GEMM (X1 [M,K1] -> T [M,N1], epilogue epi1) and its ONLY consumer (T -> [M,N2]) live in the ring kernel's
// piece-major layout?  Yes when the automatic dispatch runs BOTH on gemm_ringx_kernel (gemm_ring_auto asks the planner about the very arguments gemm() will launch with).
// (The LLM step and the tower ask the same of gemm_plan() inside their own plans: step_plan.h, tower_plan.h.)
static bool gemm_pair_pm(mmd_ctx* c, const void* X1, int64_t ldx1, const void* W1p, const void* b1, int N1w, int K1, int epi1, void* T, int64_t ldt,
                         const void* W2p, int N2, const void* R2, int64_t ldr2, void* Y2, int64_t ldy2, int epi2, int M) {
    if (c->sw.no_pm) return false;
    const GemmArgs a = gemm_args(c, X1, ldx1, nullptr, 0, b1, nullptr, 0, T, ldt, M, N1w, K1, epi1, 0, GEMM_AUTO, W1p, false);
    const GemmArgs b = gemm_args(c, T, ldt, nullptr, 0, nullptr, R2, ldr2, Y2, ldy2, M, N2, (int)ldt, epi2, 0, GEMM_AUTO, W2p, false);
    return gemm_ring_auto(c->cfg.dtype, a, true) && gemm_ring_auto(c->cfg.dtype, b);          // (the producer on the PLAIN ring: its split-K form writes row-major through splitk_reduce -- ADVICE r05)
}

// ---- create / destroy ------------------------------------------------------------------------------------------------
extern "C" int mmd_create(const mmd_config* cfg, int device, mmd_ctx** out) {
    const ModelDims dims = model_dims(out ? cfg : nullptr);
    if (dims.rc) { g_create_error = dims.error; return dims.rc; }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return MMD_EHIP; }
    mmd_ctx* c = new mmd_ctx();
    c->cfg = *cfg; c->device = device; c->resp.zero_fill = true;
    e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e); delete c; return MMD_EHIP; }
    c->stream = c->own_stream;
    c->vit_grid = dims.vit_grid; c->vit_tokens = dims.vit_tokens; c->vit_seq = dims.vit_seq; c->vit_kpad = dims.vit_kpad; c->vit_ipad = dims.vit_ipad; c->qkv_w = dims.qkv_w;
    auto is1 = [](const char* name) { const char* v = getenv(name); return v && v[0] == '1'; };
    StepSwitches& sw = c->sw;
    { const char* nf = getenv("MMDUET_NO_FUSE"); sw.no_fuse = nf && nf[0] == '1'; sw.no_pm = nf && (nf[0] == '1' || nf[0] == '2'); }          // (2: only the piece-major MLP intermediates off -- their A/B)
    sw.no_chain = is1("MMDUET_NO_CHAIN"); sw.no_slab_norm = is1("MMDUET_NO_SLAB_NORM"); sw.full_last_layer = is1("MMDUET_FULL_LAST_LAYER"); sw.no_rope_fuse = is1("MMDUET_NO_ROPE_FUSE");
    sw.no_multi_fuse = getenv("MMDUET_NO_MULTI_FUSE") != nullptr; sw.no_multi_attn = getenv("MMDUET_NO_MULTI_ATTN") != nullptr; sw.no_chunk_rope = getenv("MMDUET_NO_CHUNK_ROPE") != nullptr;
    // graph replay of the decode step is opt-in (MMDUET_GRAPH=1): measured on MI355X it is not faster than eager launches
    // from this C++ loop (458 vs 480-500 ms for 128 tokens) -- the step is bound by the ~1.5 us GPU-side kernel boundaries,
    // which a graph does not remove, not by host launch latency.
    { const char* ng = getenv("MMDUET_GRAPH"); c->no_graph = !(ng && ng[0] == '1'); }
    *out = c;
    return MMD_OK;
}

extern "C" void mmd_destroy(mmd_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    prof_drain(c);
    for (auto e : c->prof.pool) hipEventDestroy(e);
    for (void* p : c->allocs) hipFree(p);
    for (void* p : c->host_allocs) hipHostFree(p);
    for (auto& ev : c->seg_event) if (ev) hipEventDestroy(ev);
    c->dec_greedy.drop(); c->dec_sampled.drop();
    hipStreamDestroy(c->own_stream);
    delete c;
}

extern "C" const char* mmd_last_error(const mmd_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }
extern "C" int mmd_set_tower_share(mmd_ctx* c, int max_blocks) {
    if (!c || max_blocks < 0) return MMD_EINVAL;
    c->tower_ring_blocks = max_blocks; if (c->tower_ring_flags < 0) c->tower_ring_flags = 16;
    return MMD_OK;
}
extern "C" int mmd_set_stream(mmd_ctx* c, void* s) { if (!c) return MMD_EINVAL; c->stream = (hipStream_t)s; return MMD_OK; }   // 0 = the (legacy) null stream, as torch's default stream
extern "C" void* mmd_get_stream(mmd_ctx* c) { return c ? (void*)c->stream : nullptr; }
extern "C" int mmd_synchronize(mmd_ctx* c) { if (!c) return MMD_EINVAL; HIPCHK(c, hipStreamSynchronize(c->stream)); return MMD_OK; }
extern "C" int64_t mmd_weight_bytes(const mmd_ctx* c) { return c ? c->weight_bytes : 0; }

// ---- weights ---------------------------------------------------------------------------------------------------------
extern "C" int mmd_load_tensor(mmd_ctx* c, const char* name, const void* data, int src_dtype, const int64_t* shape, int rank, int on_device) {
    if (!c || !name || !data || rank < 1 || rank > 4) return MMD_EINVAL;
    if (c->finalized) FAIL(c, MMD_EINVAL, "weights already finalized");
    if (src_dtype != MMD_F32 && src_dtype != MMD_BF16) FAIL(c, MMD_EINVAL, "unsupported source dtype %d for %s", src_dtype, name);
    hipSetDevice(c->device);
    RawTensor t;
    t.numel = 1;
    for (int i = 0; i < rank; ++i) { t.shape.push_back(shape[i]); t.numel *= shape[i]; }
    int rc = dev_alloc(c, &t.p, (size_t)t.numel * es(c), false);
    if (rc) return rc;
    const void* src = data;
    void* staging = nullptr;
    if (!on_device) {
        size_t sb = (size_t)t.numel * dtype_size(src_dtype);
        if (src_dtype == c->cfg.dtype) {
            HIPCHK(c, hipMemcpyAsync(t.p, data, sb, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            src = nullptr;
        } else {
            HIPCHK(c, hipMalloc(&staging, sb));
            HIPCHK(c, hipMemcpyAsync(staging, data, sb, hipMemcpyHostToDevice, c->stream));
            src = staging;
        }
    }
    if (src) {
        HIPCHK(c, launch_convert(src, src_dtype, t.p, c->cfg.dtype, t.numel, c->stream));
        if (staging) { HIPCHK(c, hipStreamSynchronize(c->stream)); hipFree(staging); }
    }
    std::string key = canon_name(name);
    auto it = c->raw.find(key);
    if (it != c->raw.end()) dev_free(c, it->second.p);
    c->raw[key] = t;
    return MMD_OK;
}

extern "C" int mmd_merge_lora(mmd_ctx* c, const char* weight_name, const float* A_host, const float* B_host, int r, float scale) {
    if (!c || !weight_name || !A_host || !B_host || r <= 0) return MMD_EINVAL;
    auto it = c->raw.find(canon_name(weight_name));
    if (it == c->raw.end()) FAIL(c, MMD_ENOENT, "mmd_merge_lora: no tensor %s", weight_name);
    RawTensor& t = it->second;
    if (t.shape.size() != 2) FAIL(c, MMD_EINVAL, "mmd_merge_lora: %s is not a matrix", weight_name);
    int out_f = (int)t.shape[0], in_f = (int)t.shape[1];
    float *A = nullptr, *B = nullptr;
    HIPCHK(c, hipMalloc((void**)&A, sizeof(float) * r * in_f));
    HIPCHK(c, hipMalloc((void**)&B, sizeof(float) * out_f * r));
    HIPCHK(c, hipMemcpyAsync(A, A_host, sizeof(float) * r * in_f, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(B, B_host, sizeof(float) * out_f * r, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_lora_merge(c->cfg.dtype, t.p, A, B, out_f, in_f, r, scale, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(A); hipFree(B);
    return MMD_OK;
}

extern "C" int mmd_set_rope_inv_freq(mmd_ctx* c, const float* host, int n) {
    if (!c || !host || n != c->cfg.head_dim / 2) return MMD_EINVAL;
    if (!c->inv_freq) { int rc = dev_alloc(c, (void**)&c->inv_freq, sizeof(float) * n); if (rc) return rc; }
    HIPCHK(c, hipMemcpyAsync(c->inv_freq, host, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->inv_freq_user = true;
    return MMD_OK;
}

static int alloc_workspaces(mmd_ctx* c);

// MFMA-fragment-major copy of a bf16 weight matrix for the weight-streaming skinny GEMM (null if the shape does not tile)
static int make_packed(mmd_ctx* c, const void* W, int N, int K, void** out) {
    *out = nullptr;
    if (!weight_packs(c->cfg.dtype, N, K)) return MMD_OK;
    int rc = dev_alloc(c, out, (size_t)N * K * 2, false); if (rc) return rc;
    HIPCHK(c, launch_pack_w(W, K, N, K, *out, c->stream));
    return MMD_OK;
}
// pack and, where the plan says so (weight_releases, model_plan.h), drop the row-major original
static int pack_and_release(mmd_ctx* c, void** W, int N, int K, void** out) {
    int rc = make_packed(c, *W, N, K, out); if (rc) return rc;
    if (weight_releases(c->cfg.dtype, N, K)) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dev_free(c, *W); *W = nullptr;
    }
    return MMD_OK;
}

// fp8 e4m3 copy of a row-major bf16 matrix (W is replaced by bf16(q)); out8 = fragment-major bytes for the streaming kernels, scale = [N] fp32
// (the shape was checked with the plan: N % 16 == 0, K % 64 == 0)
static int quantize_fp8(mmd_ctx* c, void* W, int N, int K, void** out8, float** scale) {
    *out8 = nullptr; *scale = nullptr;
    uint8_t* q8 = nullptr;
    HIPCHK(c, hipMalloc((void**)&q8, (size_t)N * K));
    int rc = dev_alloc(c, (void**)scale, (size_t)N * sizeof(float), false); if (rc) { hipFree(q8); return rc; }
    rc = dev_alloc(c, out8, (size_t)N * K, false); if (rc) { hipFree(q8); return rc; }
    hipError_t e = launch_quantize_fp8_rows(W, N, K, q8, *scale, c->stream);
    if (e == hipSuccess) e = launch_pack_w8(q8, N, K, *out8, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(q8);
    HIPCHK(c, e);
    return MMD_OK;
}

// The one name-to-field map: the member a plan entry (model_plan.h) names, in the context, a decoder layer or a tower layer.
typedef void** (*FieldOf)(void*);
#define FIELD(T, m) {#m, [](void* o) -> void** { return (void**)&((T*)o)->m; }}
static void** field_of(mmd_ctx* c, int scope, int layer, const std::string& name) {
    static const std::unordered_map<std::string, FieldOf> ctx = {
        FIELD(mmd_ctx, embed), FIELD(mmd_ctx, fnorm), FIELD(mmd_ctx, lm_head), FIELD(mmd_ctx, lm_head_p), FIELD(mmd_ctx, heads4), FIELD(mmd_ctx, patch_w), FIELD(mmd_ctx, patch_w_p),
        FIELD(mmd_ctx, patch_b), FIELD(mmd_ctx, pos_emb), FIELD(mmd_ctx, cls_emb), FIELD(mmd_ctx, pre_w), FIELD(mmd_ctx, pre_b), FIELD(mmd_ctx, post_w), FIELD(mmd_ctx, post_b),
        FIELD(mmd_ctx, p0w), FIELD(mmd_ctx, p0w_p), FIELD(mmd_ctx, p0b), FIELD(mmd_ctx, p2w), FIELD(mmd_ctx, p2w_p), FIELD(mmd_ctx, p2b), FIELD(mmd_ctx, hd_probe), FIELD(mmd_ctx, hd_wq),
        FIELD(mmd_ctx, hd_bq), FIELD(mmd_ctx, hd_wkv), FIELD(mmd_ctx, hd_bkv), FIELD(mmd_ctx, hd_wo), FIELD(mmd_ctx, hd_bo), FIELD(mmd_ctx, hd_lnw), FIELD(mmd_ctx, hd_lnb),
        FIELD(mmd_ctx, hd_w1), FIELD(mmd_ctx, hd_b1), FIELD(mmd_ctx, hd_w2), FIELD(mmd_ctx, hd_b2),
        // workspaces
        FIELD(mmd_ctx, v_col), FIELD(mmd_ctx, v_h), FIELD(mmd_ctx, v_xn), FIELD(mmd_ctx, v_h32), FIELD(mmd_ctx, v_qkv), FIELD(mmd_ctx, v_attn), FIELD(mmd_ctx, v_mlp), FIELD(mmd_ctx, v_patch),
        FIELD(mmd_ctx, v_splitk_ws), FIELD(mmd_ctx, v_attn_ws), FIELD(mmd_ctx, hd_q), FIELD(mmd_ctx, hd_kv), FIELD(mmd_ctx, hd_a), FIELD(mmd_ctx, hd_h), FIELD(mmd_ctx, hd_n), FIELD(mmd_ctx, hd_m),
        FIELD(mmd_ctx, v_p1), FIELD(mmd_ctx, v_p2), FIELD(mmd_ctx, l_h), FIELD(mmd_ctx, l_xn), FIELD(mmd_ctx, l_qkv), FIELD(mmd_ctx, l_q), FIELD(mmd_ctx, l_attn), FIELD(mmd_ctx, l_act),
        FIELD(mmd_ctx, l_hid), FIELD(mmd_ctx, splitk_ws), FIELD(mmd_ctx, chain_ssq), FIELD(mmd_ctx, rope_tab), FIELD(mmd_ctx, attn_ws), FIELD(mmd_ctx, logits_ws), FIELD(mmd_ctx, heads_dev),
        FIELD(mmd_ctx, rows_dev), FIELD(mmd_ctx, tok_dev), FIELD(mmd_ctx, argmax_scratch), {"prev_dev", [](void* o) -> void** { return (void**)&((mmd_ctx*)o)->resp.prev_dev; }}, FIELD(mmd_ctx, gen_embed), FIELD(mmd_ctx, heads_host),
        FIELD(mmd_ctx, rows_host), FIELD(mmd_ctx, tok_host), FIELD(mmd_ctx, step_host), FIELD(mmd_ctx, seg_host), FIELD(mmd_ctx, seg_dev), FIELD(mmd_ctx, step_dev)};
    static const std::unordered_map<std::string, FieldOf> llm = {
        FIELD(LlmLayer, ln1), FIELD(LlmLayer, ln2), FIELD(LlmLayer, wqkv), FIELD(LlmLayer, bqkv), FIELD(LlmLayer, wo), FIELD(LlmLayer, wgu), FIELD(LlmLayer, wdown),
        FIELD(LlmLayer, wqkv_p), FIELD(LlmLayer, wo_p), FIELD(LlmLayer, wgu_p), FIELD(LlmLayer, wdown_p), FIELD(LlmLayer, wqkv_8), FIELD(LlmLayer, wo_8), FIELD(LlmLayer, wgu_8),
        FIELD(LlmLayer, wdown_8), FIELD(LlmLayer, sqkv), FIELD(LlmLayer, so), FIELD(LlmLayer, sgu), FIELD(LlmLayer, sdown)};
    static const std::unordered_map<std::string, FieldOf> vit = {
        FIELD(VitLayer, ln1w), FIELD(VitLayer, ln1b), FIELD(VitLayer, wqkv), FIELD(VitLayer, bqkv), FIELD(VitLayer, wo), FIELD(VitLayer, bo), FIELD(VitLayer, ln2w), FIELD(VitLayer, ln2b),
        FIELD(VitLayer, w1), FIELD(VitLayer, b1), FIELD(VitLayer, w2), FIELD(VitLayer, b2), FIELD(VitLayer, wqkv_p), FIELD(VitLayer, wo_p), FIELD(VitLayer, w1_p), FIELD(VitLayer, w2_p)};
    const auto& map = scope == IN_LLM_LAYER ? llm : scope == IN_VIT_LAYER ? vit : ctx;
    void* owner = scope == IN_LLM_LAYER ? (void*)&c->L[layer] : scope == IN_VIT_LAYER ? (void*)&c->VL[layer] : (void*)c;
    return map.at(name)(owner);
}
#undef FIELD

// the dimensions mmd_create copied from model_dims()
static ModelDims dims_of(const mmd_ctx* c) {
    ModelDims d; d.vit_grid = c->vit_grid; d.vit_tokens = c->vit_tokens; d.vit_seq = c->vit_seq; d.vit_kpad = c->vit_kpad; d.vit_ipad = c->vit_ipad; d.qkv_w = c->qkv_w;
    return d;
}

// Checks the whole weight plan against what was loaded, then executes it entry by entry.  A refusal consumes nothing: load the missing tensor and call again.
extern "C" int mmd_finalize_weights(mmd_ctx* c) {
    if (!c) return MMD_EINVAL;
    if (c->finalized) return MMD_OK;
    hipSetDevice(c->device);
    const mmd_config& g = c->cfg;
    const int dt = g.dtype; const size_t e = es(c);
    hipStream_t st = c->stream;
    const WeightPlan plan = weight_plan(g, dims_of(c));
    const WeightRefusal bad = weight_plan_check(plan, [&](const std::string& name) { auto it = c->raw.find(name); return it == c->raw.end() ? -1LL : (long long)it->second.numel; });
    if (bad.rc) FAIL(c, bad.rc, "%s", bad.error.c_str());
    if (g.tower_f16) {
        // the checkpoint's bf16 tower parameters become IEEE half, as autocast casts them per op (exact for every normal value: 8 mantissa bits into 11);
        // padding / fusing / fragment packing below only move 2-byte elements
        for (auto& kv : c->raw)
            if (kv.first.rfind("vit.", 0) == 0) HIPCHK(c, launch_convert(kv.second.p, MMD_BF16, kv.second.p, MMD_F16, kv.second.numel, st));
    }
    c->L.resize(g.vision_only ? 0 : g.num_layers); c->VL.resize(g.vit_layers);
    std::vector<void*> spent;          // sources copied from, freed at the next release point
    for (const WeightEntry& w : plan.entries) {
        std::vector<RawTensor> src;
        for (const WeightSrc& s : w.src) { auto it = c->raw.find(s.name); src.push_back(it->second); c->raw.erase(it); }
        void** dst = field_of(c, w.scope, w.layer, w.field);
        const size_t row = (size_t)w.K * e;
        int rc = MMD_OK;
        if (w.op == W_ALIAS) *dst = src[0].p;
        else {
            rc = dev_alloc(c, dst, (size_t)w.N * row, w.zero); if (rc) return rc;
            for (const RawTensor& t : src) spent.push_back(t.p);
        }
        if (w.op == W_CAT_ROWS || w.op == W_PAD_ROWS) {
            char* at = (char*)*dst;
            for (const RawTensor& t : src) { HIPCHK(c, hipMemcpyAsync(at, t.p, (size_t)t.numel * e, hipMemcpyDeviceToDevice, st)); at += (size_t)t.numel * e; }
        } else if (w.op == W_INTERLEAVE16) {
            HIPCHK(c, launch_interleave16(dt, src[0].p, src[1].p, *dst, (int)(w.N / 2), (int)w.K, st));
        } else if (w.op == W_PAD_COLS) {
            HIPCHK(c, launch_pad_cols(dt, src[0].p, (int)w.N, (int)(src[0].numel / w.N), *dst, (int)w.K, st));
        } else if (w.op == W_SPLIT_QKV) {
            void** dst2 = field_of(c, w.scope, w.layer, w.field2);
            rc = dev_alloc(c, dst2, (size_t)w.N2 * row, false); if (rc) return rc;
            HIPCHK(c, hipMemcpyAsync(*dst, src[0].p, (size_t)w.N * row, hipMemcpyDeviceToDevice, st));
            HIPCHK(c, hipMemcpyAsync(*dst2, (char*)src[0].p + (size_t)w.N * row, (size_t)w.N2 * row, hipMemcpyDeviceToDevice, st));
        }
        const std::string f = w.field;
        if (w.fp8) {      // quantise the fused matrix (one scale per output channel), then pack both copies
            rc = quantize_fp8(c, *dst, (int)w.N, (int)w.K, field_of(c, w.scope, w.layer, f + "_8"), (float**)field_of(c, w.scope, w.layer, "s" + f.substr(1))); if (rc) return rc;
        }
        if (w.pack == PACK_KEEP) rc = make_packed(c, *dst, (int)w.N, (int)w.K, field_of(c, w.scope, w.layer, f + "_p"));
        else if (w.pack == PACK_RELEASE) rc = pack_and_release(c, dst, (int)w.N, (int)w.K, field_of(c, w.scope, w.layer, f + "_p"));
        if (rc) return rc;
        if (w.release) {
            HIPCHK(c, hipStreamSynchronize(st));
            for (void* p : spent) dev_free(c, p);
            spent.clear();
        }
    }
    // tensors that are on the checkpoint but not on the path (post_layernorm when unused, pooling head, ...) are dropped
    for (auto& kv : c->raw) dev_free(c, kv.second.p);
    c->raw.clear();
    if (!c->inv_freq_user && !g.vision_only) {
        const int d = g.head_dim, n = d / 2;
        std::vector<float> t(n);
        for (int i = 0; i < n; ++i) t[i] = (float)(1.0 / std::pow((double)g.rope_theta, (double)(2 * i) / (double)d));
        if (!c->inv_freq) { int rc = dev_alloc(c, (void**)&c->inv_freq, sizeof(float) * n); if (rc) return rc; }
        HIPCHK(c, hipMemcpyAsync(c->inv_freq, t.data(), sizeof(float) * n, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    c->weight_bytes = plan.weight_bytes(g);
    int rc = alloc_workspaces(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    c->finalized = true;
    return MMD_OK;
}

static int alloc_workspaces(mmd_ctx* c) {
    const WorkspacePlan p = workspace_plan(c->cfg, dims_of(c), sizeof(StepState));
    for (const WorkspaceEntry& w : p.entries) {
        void** dst = field_of(c, IN_CTX, 0, w.field);
        int rc = w.pinned ? host_alloc(c, dst, w.bytes) : dev_alloc(c, dst, w.bytes); if (rc) return rc;
    }
    c->v_splitk_bytes = p.v_splitk_bytes; c->v_attn_bytes = p.v_attn_bytes; c->v_h32_rows = p.v_h32_rows;
    if (!c->cfg.vision_only) { c->splitk_bytes = p.splitk_bytes; c->attn_bytes = p.attn_bytes; c->resp.prev_cap = p.prev_cap; }
    return MMD_OK;
}

#define NEED_FINAL(c) do { if (!(c)) return MMD_EINVAL; if (!(c)->finalized) FAIL(c, MMD_EINVAL, "weights not finalized"); hipSetDevice((c)->device); } while (0)

// ---- vision ----------------------------------------------------------------------------------------------------------
static int connector_pool(mmd_ctx* c, const void* feats, int B, void* out, TowerProjectorPlan rows);
static int ensure_preprocess_tables(mmd_ctx* c, int T, int R);

// what tower_plan() (tower_plan.h) needs to know of this context
static TowerModel tower_model(const mmd_ctx* c) {
    const mmd_config& g = c->cfg; TowerModel m;
    m.dtype = g.dtype; m.tower_f16 = g.tower_f16; m.C = g.vit_hidden; m.heads = g.vit_heads; m.ipad = c->vit_ipad; m.grid = c->vit_grid; m.tokens = c->vit_tokens; m.seq = c->vit_seq;
    m.layers = g.vit_layers; m.pool_mode = g.pool_mode; m.pool_stride = g.pool_stride; m.class_token = g.vit_class_token != 0; m.pre_ln = g.vit_pre_layernorm != 0;
    m.post_ln = g.vit_post_layernorm != 0; m.act = g.vit_act; m.vision_only = g.vision_only != 0; m.max_batch = g.max_vit_batch; m.splitk_ws_bytes = c->v_splitk_bytes;
    m.fc1_p = !c->VL.empty() && c->VL[0].w1_p; m.fc2_p = !c->VL.empty() && c->VL[0].w2_p;
    return m;
}
// Validate the batch, evaluate the plan ONCE and store it: tower_run, the projector behind it and the debug taps launch (or refuse) what c->tower_last says.
static int tower_begin(mmd_ctx* c, int B, bool for_pool) {
    TowerShape s; s.B = B; s.for_pool = for_pool; s.full_tower = c->full_tower; s.ring_flags = c->tower_ring_flags; s.ring_max_blocks = c->tower_ring_blocks;
    const TowerPlan p = tower_plan(tower_model(c), s, c->sw.no_pm, gemm_tuning());
    if (p.rc) FAIL(c, p.rc, "%s", p.error);
    c->tower_last = p;
    return MMD_OK;
}
// a tower GEMM as every part launches it: X [M,K] -> Y [M,N] in the plan's element type (every tower tensor is IEEE half under tower_f16, the reference's autocast), weights [N,K]
// row-major (W; null where only the packed copy Wp was kept), the side stream's split-K scratch and ring cap; a residual R has Y's row stride
static int tower_gemm(mmd_ctx* c, const void* X, int64_t ldx, const void* W, const void* Wp, const void* bias, const void* R, void* Y, int64_t ldy, int M, int N, int K, int epi, int pm = 0) {
    return gemm(c, X, ldx, W, K, bias, R, R ? ldy : 0, Y, ldy, M, N, K, epi, 0, GEMM_AUTO, Wp, true, nullptr, nullptr, nullptr, nullptr, pm, c->tower_last.dt);
}

// patch embed and the stream's start, from the im2col matrix in v_col: patch GEMM, the embed form of the plan, CLIP's pre_layrnorm
static int tower_embed(mmd_ctx* c, const TowerPlan& p, int B) {
    const mmd_config& g = c->cfg; hipStream_t st = c->stream; const int C = g.vit_hidden, T = c->vit_tokens, M = B * c->vit_seq;
    void* patch_out = p.embed == TOWER_EMBED_CLS ? c->v_patch : (p.embed == TOWER_EMBED_F32 ? c->v_xn : c->v_h);
    int rc = tower_gemm(c, c->v_col, c->vit_kpad, c->patch_w, c->patch_w_p, c->patch_b, nullptr, patch_out, C, B * T, C, c->vit_kpad, EPI_NONE); if (rc) return rc;
    if (p.embed == TOWER_EMBED_F32) {          // h32 = float(patch fp16) + float(position table); layer 0's LayerNorm 1 in the same pass (no layer: the cast to the model dtype)
        const VitLayer* L0 = g.vit_layers > 0 ? &c->VL[0] : nullptr;
        ProfScope ps(c, MMD_K_NORM_ROPE, 12.0 * M * C, 0);
        HIPCHK(c, launch_resid32_layernorm(c->v_xn, c->v_h32, c->pos_emb, T, L0 ? L0->ln1w : nullptr, L0 ? L0->ln1b : nullptr, L0 ? c->v_xn : nullptr, L0 ? nullptr : c->v_h, M, C, g.vit_ln_eps, st));
    } else {
        ProfScope ps(c, MMD_K_OTHER, 0, 0);
        if (p.embed == TOWER_EMBED_CLS) { HIPCHK(c, launch_assemble_cls(p.dt, c->v_patch, c->cls_emb, c->pos_emb, B, T, C, c->v_h, st)); }
        else { HIPCHK(c, launch_add_rows(p.dt, c->v_h, c->pos_emb, M, C, T, st)); }
    }
    if (g.vit_pre_layernorm) { HIPCHK(c, launch_layernorm(p.dt, c->v_h, c->pre_w, c->pre_b, c->v_h, M, C, g.vit_ln_eps, st)); }
    return MMD_OK;
}

// one layer's attention: S query rows per frame at q (row stride ldq, a frame's rows contiguous) over all vit_seq keys of the frame in v_qkv -> v_attn [B * S, C].  Every token's
// own queries in place (q = v_qkv, ldq = 3 C, S = vit_seq) or the sparse last layer's compact block (ldq = C, S = U)
static int tower_attention(mmd_ctx* c, int dt, const void* q, int64_t ldq, int S, int B) {
    const mmd_config& g = c->cfg; const int C = g.vit_hidden, TS = c->vit_seq, hd = C / g.vit_heads;
    AttnArgs a; memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = ldq; a.K = (char*)c->v_qkv + (size_t)C * es(c); a.V = (char*)c->v_qkv + (size_t)2 * C * es(c);
    a.k_hs = hd; a.k_ts = 3 * C; a.v_hs = hd; a.v_ts = 3 * C; a.out = c->v_attn; a.ldo = C;
    a.S = S; a.nh = g.vit_heads; a.nkv = g.vit_heads; a.d = hd; a.n_ctx = TS - S; a.causal = 0;          // S query rows over all TS keys
    a.batch = B; a.q_bstride = (int64_t)S * ldq; a.kv_bstride = (int64_t)TS * 3 * C; a.o_bstride = (int64_t)S * C;
    a.ws = c->v_attn_ws; a.ws_bytes = c->v_attn_bytes; a.variant = 0;
    ProfScope ps(c, MMD_K_ATTN_VIT, 2.0 * (B * TS + B * S) * C * es(c), 4.0 * B * (double)S * TS * C);
    HIPCHK(c, launch_attention(dt, a, c->stream));
    return MMD_OK;
}

// One layer's tail -- o_proj, LayerNorm 2, fc1 + GELU, fc2, residual -- over `rows` rows of the residual stream: all tokens, or the compact block of the sparse last layer (their
// attention output is in v_attn).  pm: fc1's output is piece-major (its only reader is fc2).  One function per residual form (TowerPlan::resid).
// TOWER_RESID_EPI, and TOWER_RESID_F16 which is the same in half: o_proj and fc2 add the stream h in their epilogue
static int tower_tail_epi(mmd_ctx* c, const TowerPlan& p, const VitLayer& L, int rows, void* h, bool pm) {
    const mmd_config& g = c->cfg; const int C = g.vit_hidden, IP = c->vit_ipad; const bool quick = g.vit_act == 1;
    int rc = tower_gemm(c, c->v_attn, C, L.wo, L.wo_p, L.bo, h, h, C, rows, C, C, EPI_RESID); if (rc) return rc;
    { ProfScope ps(c, MMD_K_NORM_ROPE, 2.0 * rows * C * es(c), 0); HIPCHK(c, launch_layernorm(p.dt, h, L.ln2w, L.ln2b, c->v_xn, rows, C, g.vit_ln_eps, c->stream)); }
    // CLIP quick_gelu: plain fc1, then x * sigmoid(1.702 x) on the storage-rounded output (secondary path: not fused, never piece-major)
    rc = tower_gemm(c, c->v_xn, C, L.w1, L.w1_p, L.b1, nullptr, c->v_mlp, IP, rows, IP, C, quick ? EPI_NONE : EPI_GELU_TANH, pm ? 2 : 0); if (rc) return rc;
    if (quick) { HIPCHK(c, launch_quick_gelu(p.dt, c->v_mlp, (int64_t)rows * IP, c->stream)); }
    return tower_gemm(c, c->v_mlp, IP, L.w2, L.w2_p, L.b2, h, h, C, rows, C, IP, EPI_RESID, pm ? 1 : 0);
}
// TOWER_RESID_F32: the linears write their fp16 result to v_xn, resid32_layernorm folds it into the fp32 stream h32 and emits what follows: LayerNorm 2 behind o_proj; behind fc2 the
// NEXT layer's LayerNorm 1, or after the last layer the stream in the model dtype at cast_out (hidden_states[-1].to(bf16); cast_bytes: that pass's bytes per element, for the profiler)
static int tower_tail_f32(mmd_ctx* c, const VitLayer& L, int rows, float* h32, bool pm, const VitLayer* next, void* cast_out, double cast_bytes) {
    const mmd_config& g = c->cfg; hipStream_t st = c->stream; const int C = g.vit_hidden, IP = c->vit_ipad;
    int rc = tower_gemm(c, c->v_attn, C, L.wo, L.wo_p, L.bo, nullptr, c->v_xn, C, rows, C, C, EPI_NONE); if (rc) return rc;
    { ProfScope ps(c, MMD_K_NORM_ROPE, 12.0 * rows * C, 0); HIPCHK(c, launch_resid32_layernorm(c->v_xn, h32, nullptr, 1, L.ln2w, L.ln2b, c->v_xn, nullptr, rows, C, g.vit_ln_eps, st)); }
    rc = tower_gemm(c, c->v_xn, C, L.w1, L.w1_p, L.b1, nullptr, c->v_mlp, IP, rows, IP, C, EPI_GELU_TANH, pm ? 2 : 0); if (rc) return rc;
    rc = tower_gemm(c, c->v_mlp, IP, L.w2, L.w2_p, L.b2, nullptr, c->v_xn, C, rows, C, IP, EPI_NONE, pm ? 1 : 0); if (rc) return rc;
    ProfScope ps(c, MMD_K_NORM_ROPE, (next ? 12.0 : cast_bytes) * rows * C, 0);
    HIPCHK(c, launch_resid32_layernorm(c->v_xn, h32, nullptr, 1, next ? next->ln1w : nullptr, next ? next->ln1b : nullptr, next ? c->v_xn : nullptr, next ? nullptr : cast_out, rows, C, g.vit_ln_eps, st));
    return MMD_OK;
}

// the tower, as c->tower_last (tower_begin) says: patch-embed (+ class token, + pre-LN for CLIP) -> encoder layers -> optional post_layernorm.  Result in the model dtype:
// [B * vit_seq, C] in v_h, or with sparse_last the rows the pool reads, [B * U, C], in v_col.  px == null: the im2col matrix is in v_col already.
static int tower_run(mmd_ctx* c, const void* px, int B) {
    const mmd_config& g = c->cfg; hipStream_t st = c->stream; const TowerPlan& p = c->tower_last;
    const int dt = p.dt, C = g.vit_hidden, TS = c->vit_seq, M = B * TS, Mc = p.compact_rows;
    const bool r32 = p.resid == TOWER_RESID_F32;
    const int dt_copy = dt == MMD_F32 ? MMD_F32 : MMD_BF16;          // row gathers only move elements: 2-byte ones as bf16
    if (px) { ProfScope ps(c, MMD_K_OTHER, 0, 0); HIPCHK(c, launch_im2col(dt == MMD_F16 ? MMD_F16 + 1 : dt, px, B, g.vit_image, g.vit_patch, c->vit_grid, c->vit_kpad, c->v_col, st)); }
    int rc = tower_embed(c, p, B); if (rc) return rc;
    // the sparse last layer's compact blocks: queries in v_mlp (free until fc1), the residual stream -- then the tower's output -- in v_col (the im2col matrix is dead since the
    // patch GEMM), the fp32 stream behind the full one's rows in v_h32
    void* const qc = c->v_mlp; void* const hc = c->v_col; float* const hc32 = r32 ? c->v_h32 + c->v_h32_rows * C : nullptr;
    for (int i = 0; i < g.vit_layers; ++i) {
        const VitLayer& L = c->VL[i];
        const bool compact = p.sparse_last && i + 1 == g.vit_layers;
        if (!r32) { ProfScope ps(c, MMD_K_NORM_ROPE, 2.0 * M * C * es(c), 0); HIPCHK(c, launch_layernorm(dt, c->v_h, L.ln1w, L.ln1b, c->v_xn, M, C, g.vit_ln_eps, st)); }
        rc = tower_gemm(c, c->v_xn, C, L.wqkv, L.wqkv_p, L.bqkv, nullptr, c->v_qkv, 3 * C, M, 3 * C, C, EPI_NONE); if (rc) return rc;          // K and V always come from all tokens
        if (compact) {
            ProfScope ps(c, MMD_K_OTHER, 0, 0);
            HIPCHK(c, launch_gather_pool_rows(dt_copy, c->v_qkv, qc, B, c->vit_grid, C, p.pout, st, 3 * C));
            if (r32) { HIPCHK(c, launch_gather_pool_rows(MMD_F32, c->v_h32, hc32, B, c->vit_grid, C, p.pout, st, C)); }
            else { HIPCHK(c, launch_gather_pool_rows(dt_copy, c->v_h, hc, B, c->vit_grid, C, p.pout, st, C)); }
        }
        rc = compact ? tower_attention(c, dt, qc, C, p.U, B) : tower_attention(c, dt, c->v_qkv, 3 * C, TS, B); if (rc) return rc;
        const int rows = compact ? Mc : M; const bool pm = compact ? p.mlp_pm_last : p.mlp_pm;
        if (r32) rc = tower_tail_f32(c, L, rows, compact ? hc32 : c->v_h32, pm, i + 1 < g.vit_layers ? &c->VL[i + 1] : nullptr, compact ? hc : c->v_h, compact ? 8.0 : 12.0);
        else rc = tower_tail_epi(c, p, L, rows, compact ? hc : c->v_h, pm);
        if (rc) return rc;
    }
    if (g.vit_post_layernorm) { HIPCHK(c, launch_layernorm(dt, c->v_h, c->post_w, c->post_b, c->v_h, M, C, g.vit_ln_eps, st)); }          // (never with sparse_last)
    if (p.final_convert) {          // the tower's output is rounded to bf16 at the end (SigLipVisionTower returns hidden_states[-1].to(images.dtype) [3P-recalled]): in place, elementwise
        void* y = p.sparse_last ? hc : c->v_h;
        ProfScope ps(c, MMD_K_OTHER, 0, 0); HIPCHK(c, launch_convert(y, MMD_F16, y, MMD_BF16, (int64_t)(p.sparse_last ? Mc : M) * C, st));
    }
    c->last_vit_B = B;
    return MMD_OK;
}

// Both encode entry points: checks, the plan, the im2col matrix -- from pixel_values px inside tower_run, or here straight from uint8 frames [B,3,R,R] (SURVEY.md section 8 f1:
// image_processor.preprocess (test/inference.py:203) and the patch-embed load are one pass, the normalised pixels go from the Pillow-exact resampler directly into the im2col
// matrix of the patch GEMM; no pixel_values tensor exists; bit-identical to mmd_preprocess_frames + mmd_vit_encode) -- the tower, then projector + pool on the rows the plan says
static int vit_encode(mmd_ctx* c, const void* px, const uint8_t* frames, int B, int R, void* out) {
    NEED_FINAL(c);
    if (B <= 0) return MMD_OK;
    if (!px && (!frames || !out)) return MMD_EINVAL;
    if (c->cfg.vision_only) FAIL(c, MMD_EINVAL, "vision-only context: use mmd_vision_tower");
    int rc = tower_begin(c, B, true); if (rc) return rc;
    const TowerPlan& p = c->tower_last;
    if (!px) {
        rc = ensure_preprocess_tables(c, B, R); if (rc) return rc;
        ProfScope ps(c, MMD_K_OTHER, 0, 0);
        HIPCHK(c, launch_preprocess_im2col(p.dt, frames, B, R, c->cfg.vit_image, c->pp_coef, c->pp_bounds, c->pp_ksize, c->pp_tmp, c->cfg.vit_patch, c->vit_grid, c->vit_kpad, c->v_col, c->stream));
    }
    rc = tower_run(c, px, B); if (rc) return rc;
    return connector_pool(c, p.sparse_last ? c->v_col : c->v_h, B, out, TowerProjectorPlan{p.proj_compact, p.proj_gather, p.pout});
}
extern "C" int mmd_vit_encode(mmd_ctx* c, const void* px, int B, void* out) { return vit_encode(c, px, nullptr, B, 0, out); }
// frames uint8 [B,3,R,R] (device) -> out [B*frame_num_tokens, hidden]
extern "C" int mmd_vit_encode_frames(mmd_ctx* c, const uint8_t* frames, int B, int R, void* out) { return vit_encode(c, nullptr, frames, B, R, out); }

// ---- secondary encoder path (models/vision_live.py) -------------------------------------------------------------------------------------
extern "C" int mmd_normalize_frames(mmd_ctx* c, const void* frames, int src_kind, int B, int R, const float* mean, const float* sd, float rescale, void* out) {
    if (!c || !frames || !out || !mean || !sd || (src_kind != 0 && src_kind != 1)) return MMD_EINVAL;
    hipSetDevice(c->device);
    HIPCHK(c, launch_normalize_frames(c->cfg.dtype, frames, src_kind, B, R, rescale, mean, sd, out, c->stream));
    return MMD_OK;
}
extern "C" int mmd_vision_tower(mmd_ctx* c, const void* px, int B, void* out) {
    NEED_FINAL(c);
    if (B <= 0) return MMD_OK;
    if (!px || !out) return MMD_EINVAL;
    int rc = tower_begin(c, B, false); if (rc) return rc;          // (not for the pool: every token's output, never the sparse last layer)
    rc = tower_run(c, px, B); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(out, c->v_h, (size_t)B * c->vit_seq * c->cfg.vit_hidden * es(c), hipMemcpyDeviceToDevice, c->stream));
    return MMD_OK;
}
// adaptive_avg_pool2d of the spatial token grid (class token, if any, skipped) -- models/vision_live.py:17-24,40-47
extern "C" int mmd_vision_pool_tokens(mmd_ctx* c, const void* feats, int B, int out_h, int out_w, void* out) {
    NEED_FINAL(c);
    if (B <= 0) return MMD_OK;
    if (!feats || !out || out_h <= 0 || out_h != out_w) FAIL(c, MMD_EINVAL, "pool target must be square (frame_token_pooled = [%d, %d])", out_h, out_w);
    const int C = c->cfg.vit_hidden, T = c->vit_tokens, TS = c->vit_seq; const size_t e = es(c);
    for (int b = 0; b < B; ++b) {      // one frame at a time: with a class token the spatial rows of a frame are not contiguous with the next frame's
        const char* src = (const char*)feats + ((size_t)b * TS + (TS - T)) * C * e;
        HIPCHK(c, launch_pool(c->cfg.dtype, src, (char*)out + (size_t)b * out_h * out_w * C * e, 1, c->vit_grid, C, MMD_POOL_ADAPTIVE_AVG, out_h, c->stream));
    }
    return MMD_OK;
}
// SiglipMultiheadAttentionPoolingHead.forward (siglip/modeling_siglip.py [3P]): probe attends over the sequence (nn.MultiheadAttention), then
// residual + mlp(layernorm(.)); returns hidden_state[:, 0] -> [B, C]
extern "C" int mmd_vision_pool_head(mmd_ctx* c, const void* feats, int B, void* out) {
    NEED_FINAL(c);
    if (B <= 0) return MMD_OK;
    const mmd_config& g = c->cfg; const int dt = g.dtype; hipStream_t st = c->stream; const size_t e = es(c);
    if (!g.vit_pool_head) FAIL(c, MMD_EINVAL, "this tower has no pooling head");
    if (B > g.max_vit_batch) FAIL(c, MMD_ERANGE, "batch %d exceeds max_vit_batch %d", B, g.max_vit_batch);
    const int C = g.vit_hidden, CI = g.vit_intermediate, TS = c->vit_seq, hd = C / g.vit_heads;
    int rc = gemm(c, c->hd_probe, C, c->hd_wq, C, c->hd_bq, nullptr, 0, c->hd_q, C, 1, C, C, EPI_NONE, 0, GEMM_AUTO, nullptr, true); if (rc) return rc;
    rc = gemm(c, feats, C, c->hd_wkv, C, c->hd_bkv, nullptr, 0, c->hd_kv, 2 * C, B * TS, 2 * C, C, EPI_NONE, 0, GEMM_AUTO, nullptr, true); if (rc) return rc;
    {
        AttnArgs a; memset(&a, 0, sizeof(a));
        a.q = c->hd_q; a.ldq = C; a.K = c->hd_kv; a.V = (char*)c->hd_kv + (size_t)C * e;
        a.k_hs = hd; a.k_ts = 2 * C; a.v_hs = hd; a.v_ts = 2 * C; a.out = c->hd_a; a.ldo = C;
        a.S = 1; a.nh = g.vit_heads; a.nkv = g.vit_heads; a.d = hd; a.n_ctx = TS - 1; a.causal = 0;      // 1 query over n_ctx + S = TS keys
        a.batch = B; a.q_bstride = 0; a.kv_bstride = (int64_t)TS * 2 * C; a.o_bstride = C;
        a.ws = c->v_attn_ws; a.ws_bytes = c->v_attn_bytes; a.variant = 1;
        HIPCHK(c, launch_attention(dt, a, st));
    }
    rc = gemm(c, c->hd_a, C, c->hd_wo, C, c->hd_bo, nullptr, 0, c->hd_h, C, B, C, C, EPI_NONE, 0, GEMM_AUTO, nullptr, true); if (rc) return rc;
    HIPCHK(c, launch_layernorm(dt, c->hd_h, c->hd_lnw, c->hd_lnb, c->hd_n, B, C, g.vit_ln_eps, st));
    rc = gemm(c, c->hd_n, C, c->hd_w1, C, c->hd_b1, nullptr, 0, c->hd_m, CI, B, CI, C, EPI_GELU_TANH, 0, GEMM_AUTO, nullptr, true); if (rc) return rc;
    rc = gemm(c, c->hd_m, CI, c->hd_w2, CI, c->hd_b2, c->hd_h, C, out, C, B, C, CI, EPI_RESID, 0, GEMM_AUTO, nullptr, true); if (rc) return rc;
    return MMD_OK;
}

// second half of LiveMixin.visual_embed (models/modeling_live.py:30-33): mm_projector (Linear, GELU(erf), Linear) -> post_projector_pooling
// rows (tower_plan.h): `compact` -- the projector runs on the rows the bilinear pool reads alone; `gather` -- feats holds every token and those rows are gathered here (else the
// tower's sparse last layer already left exactly them in feats)
static int connector_pool(mmd_ctx* c, const void* feats, int B, void* out, TowerProjectorPlan rows) {
    const mmd_config& g = c->cfg; const int dt = g.dtype; hipStream_t st = c->stream;
    const int C = g.vit_hidden, H = g.hidden_size, pout = rows.pout, M = rows.compact ? B * TOWER_POOL_TAPS * pout * pout : B * c->vit_tokens;
    if (rows.gather) { ProfScope ps(c, MMD_K_OTHER, 0, 0); HIPCHK(c, launch_gather_pool_rows(dt, feats, c->v_xn, B, c->vit_grid, C, pout, st)); feats = c->v_xn; }
    int rc = gemm(c, feats, C, c->p0w, C, c->p0b, nullptr, 0, c->v_p1, H, M, H, C, EPI_GELU_ERF, 0, GEMM_AUTO, c->p0w_p, true); if (rc) return rc;
    rc = gemm(c, c->v_p1, H, c->p2w, H, c->p2b, nullptr, 0, c->v_p2, H, M, H, H, EPI_NONE, 0, GEMM_AUTO, c->p2w_p, true); if (rc) return rc;
    ProfScope ps(c, MMD_K_OTHER, 0, 0);
    if (rows.compact) { HIPCHK(c, launch_pool_compact_bilinear(dt, c->v_p2, out, B, c->vit_grid, H, pout, st)); }
    else { HIPCHK(c, launch_pool(dt, c->v_p2, out, B, c->vit_grid, H, g.pool_mode, g.pool_stride, st)); }
    return MMD_OK;
}

// the feature-file path (data/utils.py:99-117 writes what `vision_encode` returns, [T, tokens, C] per video; visual_embed then starts at the
// connector, models/modeling_live.py:26-33 without `vision_encode`): tower features [B, tokens, vit_hidden] -> [B*frame_num_tokens, hidden]
extern "C" int mmd_connector_pool(mmd_ctx* c, const void* tower_features, int B, void* out) {
    NEED_FINAL(c);
    if (B <= 0) return MMD_OK;
    if (B > c->cfg.max_vit_batch) FAIL(c, MMD_ERANGE, "feature batch %d exceeds max_vit_batch %d", B, c->cfg.max_vit_batch);
    if (!tower_features || !out) return MMD_EINVAL;
    return connector_pool(c, tower_features, B, out, tower_projector_plan(tower_model(c), false));
}

// feature extraction (vision_encode's [B, tokens, C]) and the debug taps need the tower's output for ALL tokens: on = the last layer is not restricted to the rows the pool reads
extern "C" int mmd_vit_set_full_tower(mmd_ctx* c, int on) {
    if (!c) return MMD_EINVAL;
    c->full_tower = on != 0;
    return MMD_OK;
}
extern "C" int mmd_vit_get_full_tower(const mmd_ctx* c) { return c ? (c->full_tower ? 1 : 0) : MMD_EINVAL; }

extern "C" int mmd_vit_debug_tap(mmd_ctx* c, int stage, void* out, int64_t out_elems) {
    NEED_FINAL(c);
    if (c->tower_last.sparse_last)          // only when the last encode really ran sparse (post_layernorm / class-token towers / U >= T never do): v_h holds no full output then
        FAIL(c, MMD_EINVAL, "mmd_vit_debug_tap needs mmd_vit_set_full_tower(ctx, 1) before the encode call (the default path computes the last layer for the pooled tokens only)");
    int64_t M = (int64_t)c->last_vit_B * c->vit_seq;
    int64_t n = M * (stage == 0 ? c->cfg.vit_hidden : c->cfg.hidden_size);
    if (stage < 0 || stage > 1 || out_elems < n) FAIL(c, MMD_EINVAL, "bad tap request");
    if (stage == 1 && c->last_vit_B > 0) {
        // the shipped path runs the projector on the tokens the bilinear pool reads; the tap wants connector() of ALL tokens: recompute it from the tower output
        // still sitting in v_h (debug entry point; the pooled result goes to a scratch row block of v_xn and is dropped)
        const int rc = connector_pool(c, c->v_h, c->last_vit_B, c->v_xn, tower_projector_plan(tower_model(c), true));
        if (rc) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(out, stage == 0 ? c->v_h : c->v_p2, (size_t)n * es(c), hipMemcpyDeviceToDevice, c->stream));
    return MMD_OK;
}

// Pillow tap tables (pixel_taps.h) + scratch for frames of resolution R (cached per context)
static int ensure_preprocess_tables(mmd_ctx* c, int T, int R) {
    const int size = c->cfg.vit_image;
    if (R != size && c->pp_R != R) {
        std::vector<int32_t> coef, bounds; int ks;
        pil_coeffs(R, size, coef, bounds, ks);
        if (c->pp_coef) { dev_free(c, c->pp_coef); dev_free(c, c->pp_bounds); }
        int rc = dev_alloc(c, (void**)&c->pp_coef, coef.size() * 4); if (rc) return rc;
        rc = dev_alloc(c, (void**)&c->pp_bounds, bounds.size() * 4); if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(c->pp_coef, coef.data(), coef.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->pp_bounds, bounds.data(), bounds.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->pp_R = R; c->pp_ksize = ks;
    }
    size_t need = (size_t)T * 3 * R * size;
    if (R != size && need > c->pp_tmp_bytes) {
        if (c->pp_tmp) { HIPCHK(c, hipStreamSynchronize(c->stream)); dev_free(c, c->pp_tmp); }
        int rc = dev_alloc(c, (void**)&c->pp_tmp, need, false); if (rc) return rc;
        c->pp_tmp_bytes = need;
    }
    return MMD_OK;
}

extern "C" int mmd_preprocess_frames(mmd_ctx* c, const uint8_t* frames, int T, int R, void* pixel_values) {
    if (!c || !frames || !pixel_values) return MMD_EINVAL;
    hipSetDevice(c->device);
    if (T <= 0) return MMD_OK;
    int rc = ensure_preprocess_tables(c, T, R); if (rc) return rc;
    ProfScope ps(c, MMD_K_OTHER, 0, 0);
    HIPCHK(c, launch_preprocess(c->cfg.dtype, frames, T, R, c->cfg.vit_image, c->pp_coef, c->pp_bounds, c->pp_ksize, c->pp_tmp, pixel_values, c->stream));
    return MMD_OK;
}

extern "C" int mmd_letterbox_geometry(int W, int H, int R, int* new_w, int* new_h, int* top, int* bottom, int* left, int* right) {
    if (W <= 0 || H <= 0 || R <= 0) return MMD_EINVAL;
    const LetterboxGeom g = letterbox_geom(W, H, R);       // test/datasets.py:53-60
    if (new_w) *new_w = g.new_w; if (new_h) *new_h = g.new_h;
    if (top) *top = g.top; if (bottom) *bottom = g.bottom;
    if (left) *left = g.left; if (right) *right = g.right;
    return MMD_OK;
}

extern "C" int mmd_letterbox_frames(mmd_ctx* c, const uint8_t* frames, int T, int H, int W, int R, const uint8_t* pad_color, int flip_channels,
                                    uint8_t* out) {
    if (!c || !frames || !out) return MMD_EINVAL;
    hipSetDevice(c->device);
    if (T <= 0) return MMD_OK;
    int nw, nh, top, left;
    int rc = mmd_letterbox_geometry(W, H, R, &nw, &nh, &top, nullptr, &left, nullptr); if (rc) return rc;
    if (nw <= 0 || nh <= 0) FAIL(c, MMD_EINVAL, "letterbox: %dx%d frame collapses at resolution %d", W, H, R);
    if (c->lb_W != W || c->lb_H != H || c->lb_R != R) {
        std::vector<int32_t> xt, yt;
        cv_linear_taps(W, nw, true, xt); cv_linear_taps(H, nh, false, yt);
        if (c->lb_xtab) { dev_free(c, c->lb_xtab); dev_free(c, c->lb_ytab); c->lb_xtab = c->lb_ytab = nullptr; }
        rc = dev_alloc(c, (void**)&c->lb_xtab, xt.size() * 4); if (rc) return rc;
        rc = dev_alloc(c, (void**)&c->lb_ytab, yt.size() * 4); if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(c->lb_xtab, xt.data(), xt.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->lb_ytab, yt.data(), yt.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->lb_W = W; c->lb_H = H; c->lb_R = R;
    }
    const int area2x = letterbox_area2x(W, H, nw, nh);
    uint32_t pad = 0;
    if (pad_color) pad = (uint32_t)pad_color[0] | ((uint32_t)pad_color[1] << 8) | ((uint32_t)pad_color[2] << 16);
    ProfScope ps(c, MMD_K_OTHER, 0, 0);
    HIPCHK(c, launch_letterbox(frames, T, H, W, nw, nh, R, top, left, c->lb_xtab, c->lb_ytab, area2x, flip_channels ? 1 : 0, pad, out, c->stream));
    return MMD_OK;
}

// ---- language ----------------------------------------------------------------------------------------------------------
extern "C" int mmd_embed_tokens(mmd_ctx* c, const int64_t* ids, int k, void* out) {
    NEED_FINAL(c);
    ProfScope ps(c, MMD_K_OTHER, 0, 0);
    HIPCHK(c, launch_embed(c->cfg.dtype, c->embed, ids, k, c->cfg.hidden_size, c->cfg.vocab_size, out, c->stream));
    return MMD_OK;
}

// ---- the stream KV arena: kv_plan.h states its geometry, what every operation on it checks, launches and leaves behind, and the capacities growth tries; the code here makes
// the runtime calls
static KvGeom kv_geom(const mmd_ctx* c) { KvGeom g; g.layers = c->cfg.num_layers; g.kv_heads = c->cfg.num_kv_heads; g.head_dim = c->cfg.head_dim; g.elem_bytes = (int)es(c); return g; }
static KvState kv_state(const mmd_stream* s) { KvState k; k.len = s->len; k.pos_off = s->pos_off; k.cap = s->cap; k.mapped = s->mapped; k.stash_from = s->stash_from; k.stash_to = s->stash_to; return k; }

// Map physical pages behind tokens [s->mapped, upto) of every (layer, kv head) row of K and V (whole chunks).
static int vmm_map_upto(mmd_ctx* c, mmd_stream* s, int64_t upto) {
    const KvGeom g = kv_geom(c);
    const size_t tok_bytes = g.tok_bytes(), rows = g.rows(), row_stride = g.pitch_bytes(s->cap);
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = c->device;
    hipMemAccessDesc acc = {};
    acc.location = prop.location; acc.flags = hipMemAccessFlagsProtReadWrite;
    while (s->mapped < upto) {
        if (s->mapped + s->chunk_tokens > s->cap) FAIL(c, MMD_ENOMEM, "KV arena: %lld tokens exceed the reserved virtual capacity %lld (MMDUET_KV_VIRTUAL_TOKENS)", (long long)upto, (long long)s->cap);
        const size_t cb = (size_t)s->chunk_tokens * tok_bytes, off = (size_t)s->mapped * tok_bytes;
        const size_t done0 = s->handles.size();
        // a chunk is all-or-nothing: `mapped` advances only when every row has its pages, so on a failure (out of HBM near the limit this arena is built
        // for) the rows already mapped for THIS chunk are unmapped again -- a later kv_reserve then retries on clean addresses instead of failing for good
        auto undo = [&]() {
            hipStreamSynchronize(c->stream);          // rows mapped earlier in this chunk have a zero-fill queued on the stream: let it finish before their pages go away
            while (s->handles.size() > done0) {
                hipMemUnmap(s->maps.back().first, s->maps.back().second); hipMemRelease(s->handles.back());
                s->maps.pop_back(); s->handles.pop_back();
            }
            (void)hipGetLastError();
        };
        for (int kv = 0; kv < 2; ++kv)
            for (size_t r = 0; r < rows; ++r) {
                char* at = (char*)(kv ? s->V : s->K) + r * row_stride + off;
                hipMemGenericAllocationHandle_t h;
                hipError_t er = hipMemCreate(&h, cb, &prop, 0);
                if (er != hipSuccess) { undo(); FAIL(c, MMD_ENOMEM, "KV arena: no physical memory for tokens %lld.. (%s)", (long long)s->mapped, hipGetErrorString(er)); }
                er = hipMemMap(at, cb, 0, h, 0);
                if (er != hipSuccess) { hipMemRelease(h); undo(); FAIL(c, MMD_EHIP, "KV arena: hipMemMap failed: %s", hipGetErrorString(er)); }
                s->handles.push_back(h); s->maps.push_back({at, cb});
                er = hipMemSetAccess(at, cb, &acc, 1);
                if (er != hipSuccess) { undo(); FAIL(c, MMD_EHIP, "KV arena: hipMemSetAccess failed: %s", hipGetErrorString(er)); }
                HIPCHK(c, hipMemsetAsync(at, 0, cb, c->stream));
            }
        s->mapped += s->chunk_tokens;
    }
    return MMD_OK;
}
static void vmm_release(mmd_stream* s) {
    for (auto& m : s->maps) hipMemUnmap(m.first, m.second);
    for (auto h : s->handles) hipMemRelease(h);
    s->maps.clear(); s->handles.clear();
    if (s->K) hipMemAddressFree(s->K, s->va_bytes);
    if (s->V) hipMemAddressFree(s->V, s->va_bytes);
    s->K = s->V = nullptr;
}

extern "C" int mmd_stream_create(mmd_ctx* c, int64_t initial_tokens, mmd_stream** out) {
    if (!c || !out) return MMD_EINVAL;
    hipSetDevice(c->device);
    initial_tokens = kv_initial_tokens(initial_tokens);
    mmd_stream* s = new mmd_stream();
    s->ctx = c; s->len = 0;
    const KvGeom g = kv_geom(c);
    // --- virtual-memory arena: reserve the row stride once, back it on demand
    const char* nv = getenv("MMDUET_KV_NO_VMM");
    if (!(nv && nv[0] == '1')) {
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = c->device;
        size_t gran = 0;
        if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) == hipSuccess && gran > 0) {
            const int64_t ct = kv_vmm_chunk_tokens(g.tok_bytes(), gran);
            const char* ev = getenv("MMDUET_KV_VIRTUAL_TOKENS");
            int64_t tries[KV_MAX_RESERVATIONS];
            const int n_tries = kv_vmm_reservations(initial_tokens, ev ? atoll(ev) : KV_VIRTUAL_TOKENS_DEFAULT, ct, tries);
            for (int t = 0; t < n_tries; ++t) {
                const int64_t vcap = tries[t];
                const size_t va = g.arena_bytes(vcap);
                void *K = nullptr, *V = nullptr;
                if (hipMemAddressReserve(&K, va, gran, nullptr, 0) == hipSuccess && hipMemAddressReserve(&V, va, gran, nullptr, 0) == hipSuccess) {
                    s->vmm = true; s->K = K; s->V = V; s->cap = vcap; s->chunk_tokens = ct; s->va_bytes = va; s->mapped = 0;
                    break;
                }
                if (K) hipMemAddressFree(K, va);
                (void)hipGetLastError();
            }
        }
        (void)hipGetLastError();
        if (s->vmm) {
            int rc = vmm_map_upto(c, s, initial_tokens);
            if (rc) { std::string keep = c->err; vmm_release(s); delete s; c->err = keep; return rc; }
            *out = s;
            return MMD_OK;
        }
    }
    // --- fallback: plain allocation, growth by reallocation + copy
    s->cap = initial_tokens; s->mapped = initial_tokens;
    size_t bytes = g.arena_bytes(s->cap);
    hipError_t e1 = hipMalloc(&s->K, bytes), e2 = hipMalloc(&s->V, bytes);
    if (e1 != hipSuccess || e2 != hipSuccess) { if (s->K) hipFree(s->K); if (s->V) hipFree(s->V); delete s; FAIL(c, MMD_ENOMEM, "KV arena of %lld tokens (%zu bytes x2) does not fit", (long long)initial_tokens, bytes); }
    hipMemsetAsync(s->K, 0, bytes, c->stream); hipMemsetAsync(s->V, 0, bytes, c->stream);
    *out = s;
    return MMD_OK;
}
extern "C" void mmd_stream_destroy(mmd_stream* s) {
    if (!s) return;
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    if (s->vmm) vmm_release(s); else { hipFree(s->K); hipFree(s->V); }
    if (s->stash_k) { hipFree(s->stash_k); hipFree(s->stash_v); }
    delete s;
}

static int kv_reserve(mmd_ctx* c, mmd_stream* s, int64_t need) {
    if (need <= s->mapped) return MMD_OK;
    if (s->vmm) return vmm_map_upto(c, s, need);            // growth = more pages behind the same addresses: no copy, no second arena
    const KvGeom g = kv_geom(c);
    int64_t ncap = kv_grow_doubled(s->cap, need);
    size_t bytes = g.arena_bytes(ncap);
    void *nK = nullptr, *nV = nullptr;
    if (hipMalloc(&nK, bytes) != hipSuccess || hipMalloc(&nV, bytes) != hipSuccess) {
        if (nK) { hipFree(nK); nK = nullptr; }
        (void)hipGetLastError();
        ncap = kv_grow_exact(need);
        bytes = g.arena_bytes(ncap);
        if (hipMalloc(&nK, bytes) != hipSuccess || hipMalloc(&nV, bytes) != hipSuccess) {
            if (nK) hipFree(nK);
            (void)hipGetLastError();
            FAIL(c, MMD_ENOMEM, "cannot grow KV arena to %lld tokens (%zu bytes x2 next to the live arena)", (long long)ncap, bytes);
        }
    }
    hipMemsetAsync(nK, 0, bytes, c->stream); hipMemsetAsync(nV, 0, bytes, c->stream);
    const size_t w = kv_grow_copy_bytes(g, s->len);
    if (w) {
        HIPCHK(c, hipMemcpy2DAsync(nK, g.pitch_bytes(ncap), s->K, g.pitch_bytes(s->cap), w, g.rows(), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(nV, g.pitch_bytes(ncap), s->V, g.pitch_bytes(s->cap), w, g.rows(), hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(s->K); hipFree(s->V);
    s->K = nK; s->V = nV; s->cap = ncap; s->mapped = ncap;
    return MMD_OK;
}

static int kv_bufs(const void* K, const void* V) { return !K || !V ? KV_BUF_MISSING : (((uintptr_t)K | (uintptr_t)V) & 15) != 0 ? KV_BUF_MISALIGNED : KV_BUF_OK; }
// the K and V launch_copy_rows pair of a plan's spans, between the arena (K, V) and the other side (Ko, Vo)
static int kv_copy_pair(mmd_ctx* c, const KvPlan& p, char* K, char* V, void* Ko, void* Vo) {
    if (p.launch == KV_ROWS_OUT) {
        HIPCHK(c, launch_copy_rows(MMD_F32, K + p.k_off, p.pitch4, Ko, p.k_other4, p.copy_rows, (int)p.k_cols, c->stream));
        HIPCHK(c, launch_copy_rows(MMD_F32, V + p.v_off, p.pitch4, Vo, p.v_other4, p.copy_rows, (int)p.v_cols, c->stream));
    } else {
        HIPCHK(c, launch_copy_rows(MMD_F32, Ko, p.k_other4, K + p.k_off, p.pitch4, p.copy_rows, (int)p.k_cols, c->stream));
        HIPCHK(c, launch_copy_rows(MMD_F32, Vo, p.v_other4, V + p.v_off, p.pitch4, p.copy_rows, (int)p.v_cols, c->stream));
    }
    return MMD_OK;
}
// KV_DROP_SPANS: kv_run's order of business for the one operation whose argument is a span LIST (kv_plan_spans): refused, nothing, or its launches in the planned order
// (highest group first).  The list is read here, on the host; nothing waits for the device.  The bookkeeping follows every launch (each is a complete compaction that ends
// at its own len_end), so a launch that fails behind an earlier one of a grouped plan leaves the stream's length and position those of the arena as it then stands.
static int kv_run_spans(mmd_stream* s, const int64_t* spans, int n, int flags) {
    mmd_ctx* c = s->ctx; const KvGeom g = kv_geom(c);
    const KvSpansPlan p = kv_plan_spans(g, kv_state(s), spans, n, flags);
    if (p.rc != MMD_OK) FAIL(c, p.rc, "%s", p.error);
    if (p.nothing) return MMD_OK;
    const bool shift = p.launch == KV_LAUNCH_COMPACT_SHIFT;
    if (shift && !c->inv_freq) FAIL(c, MMD_EINVAL, "kv_drop_shift: the context has no RoPE frequency table");
    if (p.launch != KV_LAUNCH_NONE) hipSetDevice(c->device);
    for (const KvCompact& l : p.launches) {
        HIPCHK(c, launch_kv_compact(c->cfg.dtype, s->K, s->V, (int)g.rows(), p.pitch_bytes, g.head_dim, reinterpret_cast<const int64_t*>(l.seg), l.nseg, l.dst0, l.len_end,
                                    shift ? c->inv_freq : nullptr, c->stream));
        if (!shift) s->pos_off += s->len - l.len_end;          // (what a dropped tail in front of this launch took is in the difference too)
        s->len = l.len_end;
    }
    s->len = p.after.len; s->pos_off = p.after.pos_off;
    return MMD_OK;
}
// One operation on s's arena as kv_plan states it: refused, or -- in this order -- memory behind the tokens it needs, the stash buffers, the launches, the bookkeeping.
// Ko / Vo: the side of the launches that is not s's arena -- the caller's buffers, a fork's source arena, nullptr for the stash buffers
static int kv_run(mmd_stream* s, int op, int64_t a = 0, int64_t b = 0, const mmd_stream* src = nullptr, const void* Ko = nullptr, const void* Vo = nullptr, int flags = 0) {
    if (op == KV_DROP_SPANS) return kv_run_spans(s, static_cast<const int64_t*>(Ko), (int)a, flags);          // a = n, Ko = the span list
    mmd_ctx* c = s->ctx; const KvGeom g = kv_geom(c);
    KvState from; if (src) from = kv_state(src);
    auto plan = [&]() { return kv_plan(op, g, kv_state(s), a, b, src ? &from : nullptr, kv_bufs(Ko, Vo), flags); };
    KvPlan p = plan();
    if (p.rc != MMD_OK) FAIL(c, p.rc, "%s", p.error);
    if (p.nothing) return MMD_OK;
    if (p.launch == KV_LAUNCH_DROP_SHIFT && !c->inv_freq) FAIL(c, MMD_EINVAL, "kv_drop_shift: the context has no RoPE frequency table");
    if (p.reserve || p.stash_bytes || p.launch != KV_LAUNCH_NONE) hipSetDevice(c->device);
    if (p.reserve) {
        int rc = kv_reserve(c, s, p.reserve); if (rc) return rc;
        p = plan();          // (the fallback arena grows into another row stride)
    }
    if (p.stash_bytes > s->stash_bytes) {
        if (s->stash_k) { HIPCHK(c, hipStreamSynchronize(c->stream)); hipFree(s->stash_k); hipFree(s->stash_v); s->stash_k = s->stash_v = nullptr; }
        s->stash_bytes = p.stash_bytes;
        if (hipMalloc(&s->stash_k, s->stash_bytes) != hipSuccess || hipMalloc(&s->stash_v, s->stash_bytes) != hipSuccess) { s->stash_bytes = 0; FAIL(c, MMD_ENOMEM, "kv_stash: no memory for %zu bytes x2", p.stash_bytes); }
    }
    if (!Ko) { Ko = s->stash_k; Vo = s->stash_v; }
    const int rows = (int)g.rows();
    switch (p.launch) {
    case KV_ROWS_OUT: case KV_ROWS_IN: { int rc = kv_copy_pair(c, p, (char*)s->K, (char*)s->V, (void*)Ko, (void*)Vo); if (rc) return rc; break; }
    case KV_LAUNCH_DROP: HIPCHK(c, launch_kv_drop(c->cfg.dtype, s->K, s->V, rows, p.pitch_bytes, g.head_dim, p.t0, p.t1, s->len, c->stream)); break;
    case KV_LAUNCH_DROP_SHIFT: HIPCHK(c, launch_kv_drop_shift(c->cfg.dtype, s->K, s->V, rows, p.pitch_bytes, g.head_dim, p.t0, p.t1, s->len, c->inv_freq, c->stream)); break;
    case KV_CANON_GATHER: case KV_CANON_SCATTER:
        HIPCHK(c, launch_kv_canon(c->cfg.dtype, p.launch == KV_CANON_SCATTER ? 1 : 0, s->K, s->V, rows, p.pitch_bytes, g.head_dim, p.t0, p.t1, (void*)Ko, (void*)Vo, c->stream)); break;
    default: break;
    }
    s->len = p.after.len; s->pos_off = p.after.pos_off; s->stash_from = p.after.stash_from; s->stash_to = p.after.stash_to;
    return MMD_OK;
}

extern "C" int64_t mmd_kv_len(const mmd_stream* s) { return s ? s->len : -1; }
extern "C" int64_t mmd_kv_capacity(const mmd_stream* s) { return s ? s->mapped : -1; }          // tokens with memory behind them
extern "C" int64_t mmd_kv_stride(const mmd_stream* s) { return s ? s->cap : -1; }                // row stride in tokens (= reserved virtual capacity)
extern "C" int64_t mmd_kv_position(const mmd_stream* s) { return s ? s->len + s->pos_off : -1; }          // the RoPE position the next token gets
extern "C" int mmd_kv_truncate(mmd_stream* s, int64_t n) { return s ? kv_run(s, KV_TRUNCATE, n) : MMD_EINVAL; }
extern "C" int mmd_stream_reset(mmd_stream* s) { return s ? kv_run(s, KV_RESET) : MMD_EINVAL; }
extern "C" int mmd_kv_stash(mmd_stream* s, int64_t from, int64_t to) { return s ? kv_run(s, KV_STASH, from, to) : MMD_EINVAL; }
extern "C" int mmd_kv_unstash(mmd_stream* s) { return s ? kv_run(s, KV_UNSTASH) : MMD_EINVAL; }
extern "C" int mmd_kv_drop(mmd_stream* s, int64_t from, int64_t to) { return s ? kv_run(s, KV_DROP, from, to) : MMD_EINVAL; }
extern "C" int mmd_kv_drop_shift(mmd_stream* s, int64_t from, int64_t to) { return s ? kv_run(s, KV_DROP, from, to, nullptr, nullptr, nullptr, KV_F_SHIFT) : MMD_EINVAL; }
extern "C" int mmd_kv_drop_spans(mmd_stream* s, const int64_t* spans_host, int n, int shift) {
    return s && n >= 0 && (spans_host || n == 0) ? kv_run(s, KV_DROP_SPANS, n, 0, nullptr, spans_host, nullptr, shift ? KV_F_SHIFT : 0) : MMD_EINVAL;
}
// snapshots (DESIGN.md section 5 "Snapshots")
extern "C" int mmd_kv_export(mmd_stream* s, int64_t from, int64_t to, void* K_out, void* V_out) { return s ? kv_run(s, KV_EXPORT, from, to, nullptr, K_out, V_out) : MMD_EINVAL; }
extern "C" int mmd_kv_import(mmd_stream* s, const void* K_in, const void* V_in, int64_t n) { return s ? kv_run(s, KV_IMPORT, n, 0, nullptr, K_in, V_in) : MMD_EINVAL; }
extern "C" int mmd_kv_set_position(mmd_stream* s, int64_t position) { return s ? kv_run(s, KV_SET_POSITION, position) : MMD_EINVAL; }
extern "C" int mmd_kv_fork(mmd_stream* dst, const mmd_stream* src, int64_t n) {
    if (!dst || !src) return MMD_EINVAL;
    mmd_ctx* c = dst->ctx;
    // (these two compare pointers, so they stand here, in front of kv_plan's checks as they always did)
    if (src->ctx != c) FAIL(c, MMD_EINVAL, "kv_fork: the two streams belong to different contexts");
    if (dst == src) FAIL(c, MMD_EINVAL, "kv_fork: a stream cannot be forked onto itself");
    return kv_run(dst, KV_FORK, n, 0, src, src->K, src->V);
}
extern "C" int mmd_kv_debug_set_len(mmd_stream* s, int64_t n) { return s && n >= 0 ? kv_run(s, KV_DEBUG_SET_LEN, n) : MMD_EINVAL; }
// (synchronises the stream)
extern "C" int mmd_kv_debug_read(mmd_stream* s, int layer, int64_t n, void* K_out, void* V_out) {
    if (!s) return MMD_EINVAL;
    int rc = kv_run(s, KV_DEBUG_READ, layer, n, nullptr, K_out, V_out); if (rc) return rc;
    HIPCHK(s->ctx, hipStreamSynchronize(s->ctx->stream));
    return MMD_OK;
}

// dyn != nullptr: the step is being captured into the decode graph -- position and arena come from device state, no
// host-side allocation / bookkeeping / event recording may happen here.
// One causal forward over `nseg` video streams: segment j is rows [row0, row0 + rows) of the step and extends stream j's
// arena; every GEMM / norm runs once over all S rows, RoPE + KV append + attention run per segment on that stream's arena.
// Which launches that takes is decided once per step by step_plan() (step_plan.h); the functions below read the plan and launch.
struct StepSeg { mmd_stream* s; int row0; int rows; };
// one step in flight: its arguments, its plan, and the little state the layers hand on
struct StepRun {
    mmd_ctx* c; const StepSeg* segs; int nseg; int S; const StepState* dyn; const int32_t* need_rows; int n_need;
    StepPlan p;
    const StepState* seg_states = nullptr;          // device copy of the batched attention run's per-stream states
    GemvChain ch_fin, ch_xn;                        // decode chain: producer / consumer side
    bool xn_ready = false;                          // tile schedule: the previous layer's fused slab consumer already left this layer's normalised input in l_xn
};
static StepModel step_model(const mmd_ctx* c) {
    const mmd_config& g = c->cfg; static const LlmLayer none; const LlmLayer& L = c->L.empty() ? none : c->L[0]; StepModel m;          // (no layers: nothing packed, the tile schedule)
    m.dtype = g.dtype; m.H = g.hidden_size; m.I = g.intermediate_size; m.nh = g.num_heads; m.nkv = g.num_kv_heads; m.d = g.head_dim; m.qkv_w = c->qkv_w; m.layers = g.num_layers;
    m.qkv_p = L.wqkv_p != nullptr; m.o_p = L.wo_p != nullptr; m.gu_p = L.wgu_p != nullptr; m.down_p = L.wdown_p != nullptr; m.fp8 = L.sgu != nullptr;
    m.attn_ws = c->attn_ws != nullptr; m.splitk_ws_bytes = c->splitk_ws ? c->splitk_bytes : 0; return m;
}
// the GemmArgs of a slab-mode GEMM of a step: the weight-streaming kernels leave fp32 K slabs in the split-K workspace and the NEXT operator consumes them
// (reduce + bias + RoPE + KV append; reduce + residual + RMSNorm) -- identical rounding points, fewer launches
static GemmArgs slab_args(mmd_ctx* c, const void* X, int64_t ldx, const void* Wp, int M, int N, int K) {
    GemmArgs a; memset(&a, 0, sizeof(a));
    a.X = X; a.ldx = ldx; a.Wp = Wp; a.M = M; a.N = N; a.K = K; a.epi = EPI_NONE; a.variant = GEMM_SKINNY;
    a.splitk_ws = c->splitk_ws; a.splitk_ws_bytes = c->splitk_bytes;
    return a;
}
// Mrows > 0: the GEMM runs on that many gathered rows (sparse last layer)
static int slab_gemm(const StepRun& r, const void* X, int64_t ldx, const void* Wp, int N, int K, int* splits, const void* Wp8, const float* wscale, const GemvChain* chn = nullptr, int Mrows = 0) {
    mmd_ctx* c = r.c; const int S = r.S; const double e = (double)es(c);
    GemmArgs a = slab_args(c, X, ldx, Wp, Mrows > 0 ? Mrows : S, N, K);
    a.chain = chn; a.Wp8 = Wp8; a.wscale = wscale; a.slabs_out = splits;
    ProfScope ps(c, MMD_K_GEMM_SKINNY, (double)S * K * e + (double)N * K * (Wp8 ? 1.0 : e) + (double)S * N * e, 2.0 * S * N * K);
    HIPCHK(c, launch_gemm(c->cfg.dtype, a, c->stream));
    return MMD_OK;
}
// the per-stream (context, capacity, arena) of the batched decode attention's run, uploaded through one of eight rotating pinned slots
static int upload_seg_states(StepRun& r) {
    mmd_ctx* c = r.c; hipStream_t st = c->stream;
    const int slot = c->seg_slot;
    StepState* hs = c->seg_host + (size_t)slot * STEP_MULTI_ATTN_MAX_RUN; StepState* ds = c->seg_dev + (size_t)slot * STEP_MULTI_ATTN_MAX_RUN;
    c->seg_slot = (slot + 1) & 7;
    if (!c->seg_event[slot]) HIPCHK(c, hipEventCreateWithFlags(&c->seg_event[slot], hipEventDisableTiming));
    else HIPCHK(c, hipEventSynchronize(c->seg_event[slot]));          // (eight steps old: long done unless the caller queues steps without ever synchronising)
    for (int j = 0; j < r.p.run_n; ++j) { mmd_stream* sj = r.segs[r.p.run0 + j].s; hs[j].n_ctx = sj->len; hs[j].cap = sj->cap; hs[j].K = sj->K; hs[j].V = sj->V; hs[j].n_prev = 0; hs[j].step = 0; hs[j].pos_off = sj->pos_off; }
    HIPCHK(c, hipMemcpyAsync(ds, hs, sizeof(StepState) * r.p.run_n, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(c->seg_event[slot], st));
    r.seg_states = ds;
    return MMD_OK;
}
// layer i: the qkv GEMM, then RoPE + KV append per segment (unless the attention kernel prepares q / k / v from the slabs itself); *splits = the qkv slabs left in the workspace
static int layer_qkv(StepRun& r, int i, int* splits) {
    mmd_ctx* c = r.c; const mmd_config& g = c->cfg; LlmLayer& L = c->L[i]; hipStream_t st = c->stream;
    const int dt = g.dtype, S = r.S, H = g.hidden_size, nh = g.num_heads, nkv = g.num_kv_heads, d = g.head_dim; const size_t e = es(c); int rc;
    if (r.p.schedule != STEP_TILE) {
        r.ch_xn.xn_gamma = L.ln1;
        rc = slab_gemm(r, c->l_xn, H, L.wqkv_p, c->qkv_w, H, splits, L.wqkv_8, L.sqkv, r.p.schedule == STEP_CHAIN && i > 0 ? &r.ch_xn : nullptr); if (rc) return rc;
        if (r.p.rope_fused) return MMD_OK;
    } else {
        if (!r.xn_ready) { ProfScope ps(c, MMD_K_NORM_ROPE, 2.0 * S * H * e, 0); HIPCHK(c, launch_rmsnorm(dt, c->l_h, L.ln1, c->l_xn, S, H, g.rms_norm_eps, st)); }
        r.xn_ready = false;
        rc = gemm(c, c->l_xn, H, L.wqkv, H, L.bqkv, nullptr, 0, c->l_qkv, c->qkv_w, S, c->qkv_w, H, EPI_NONE, 0, GEMM_AUTO, L.wqkv_p, false, L.wqkv_8, L.sqkv); if (rc) return rc;
    }
    ProfScope ps(c, MMD_K_NORM_ROPE, 2.0 * S * c->qkv_w * e, 0);
    for (int j = 0; j < r.nseg; ++j) {
        const StepSeg& sg = r.segs[j]; mmd_stream* sj = sg.s;
        const size_t lb = kv_geom(c).layer_bytes(sj->cap);
        void* q = (char*)c->l_q + (size_t)sg.row0 * nh * d * e; void* K = (char*)sj->K + (size_t)i * lb; void* V = (char*)sj->V + (size_t)i * lb;
        if (r.p.schedule != STEP_TILE)
            HIPCHK(c, launch_slab_rope_append(c->splitk_ws + (size_t)sg.row0 * c->qkv_w, *splits, L.bqkv, sg.rows, nh, nkv, d, c->inv_freq, sj->len, q, K, V, sj->cap, st, r.dyn, i, S, sj->pos_off));
        else if (r.p.chunk_rope)          // vectorised form over the step's (cos, sin) table (built once, before the layer loop)
            HIPCHK(c, launch_rope_append_chunk((char*)c->l_qkv + (size_t)sg.row0 * c->qkv_w * e, sg.rows, nh, nkv, (char*)c->rope_tab + (size_t)sg.row0 * 64 * 8, sj->len, q, K, V, sj->cap, st));
        else
            HIPCHK(c, launch_rope_append(dt, (char*)c->l_qkv + (size_t)sg.row0 * c->qkv_w * e, sg.rows, nh, nkv, d, c->inv_freq, sj->len, q, K, V, sj->cap, 1, st, sj->pos_off));
    }
    return MMD_OK;
}
// what the batched and the per-stream attention launch of layer i share: `rows` query rows from step row `row0` on
static AttnArgs attn_args(const StepRun& r, int i, int row0, int rows, int splits) {
    mmd_ctx* c = r.c; const mmd_config& g = c->cfg;
    const int nh = g.num_heads, d = g.head_dim; const size_t e = es(c);
    AttnArgs a; memset(&a, 0, sizeof(a));
    a.q = (char*)c->l_q + (size_t)row0 * nh * d * e; a.ldq = (int64_t)nh * d; a.out = (char*)c->l_attn + (size_t)row0 * nh * d * e; a.ldo = (int64_t)nh * d;
    a.k_ts = d; a.v_ts = d; a.v_transposed = 1;
    a.S = rows; a.nh = nh; a.nkv = g.num_kv_heads; a.d = d; a.causal = 1; a.batch = 1; a.ws = c->attn_ws; a.ws_bytes = c->attn_bytes; a.layer = i;
    // few rows, head_dim 128: the attention kernel prepares q / k / v from the qkv slabs itself (AttnArgs::qkv_slabs)
    if (r.p.rope_fused) { a.qkv_slabs = c->splitk_ws + (size_t)row0 * c->qkv_w; a.slab_rows = r.S; a.n_slabs = splits; a.qkv_bias = c->L[i].bqkv; a.rope_tab = (char*)c->rope_tab + (size_t)row0 * 64 * 8; }
    return a;
}
// layer i: ONE launch for the plan's run of talking streams (a quarter of the launches, partials and merge work of per-stream launches whose 64-way key splits each fill
// the chip alone), one launch per other segment on its stream's arena
static int layer_attention(const StepRun& r, int i, int splits) {
    mmd_ctx* c = r.c; const mmd_config& g = c->cfg; hipStream_t st = c->stream;
    const int nh = g.num_heads, nkv = g.num_kv_heads, d = g.head_dim, run0 = r.p.run0, run_n = r.p.run_n; const size_t e = es(c);
    if (run_n > 0) {
        const int rr = r.segs[run0].rows;
        AttnArgs a = attn_args(r, i, r.segs[run0].row0, rr, splits);
        a.segs = r.seg_states; a.nseg = run_n;
        double kvb = 0, fl = 0;
        for (int j = run0; j < run0 + run_n; ++j) { const double nk = (double)(r.segs[j].s->len + r.segs[j].rows); kvb += 2.0 * nk * nkv * d * e; fl += 4.0 * r.segs[j].rows * nk * nh * d; }
        ProfScope ps(c, MMD_K_ATTN_LLM, kvb + 2.0 * rr * run_n * nh * d * e, fl);
        a.plan_out = c->last_form;
        HIPCHK(c, launch_attention_decode_multi(a, st));
    }
    for (int j = 0; j < r.nseg; ++j) {
        if (j >= run0 && j < run0 + run_n) continue;
        mmd_stream* sj = r.segs[j].s;
        const size_t lb = kv_geom(c).layer_bytes(sj->cap);
        const int Sj = r.segs[j].rows; const int64_t nj = sj->len;
        AttnArgs a = attn_args(r, i, r.segs[j].row0, Sj, splits);
        a.K = (char*)sj->K + (size_t)i * lb; a.V = (char*)sj->V + (size_t)i * lb;
        a.k_hs = sj->cap * d; a.v_hs = sj->cap * d; a.n_ctx = nj;
        a.dyn = r.dyn; a.dyn_splits = 64;
        double kvb = 2.0 * (double)(nj + Sj) * nkv * d * e;
        ProfScope ps(c, MMD_K_ATTN_LLM, kvb + 2.0 * Sj * nh * d * e, 4.0 * Sj * (double)(nj + Sj) * nh * d);
        a.plan_out = c->last_form;
        HIPCHK(c, launch_attention(g.dtype, a, st));
    }
    return MMD_OK;
}
// the norm weight and the destination of the normalised rows behind layer i: the next layer's input, or the final norm into l_hid
static const void* next_norm(const mmd_ctx* c, int i) { return i + 1 < c->cfg.num_layers ? c->L[i + 1].ln1 : c->fnorm; }
static void* next_xn(const mmd_ctx* c, int i) { return i + 1 < c->cfg.num_layers ? c->l_xn : c->l_hid; }
// Decode chain (every GEMM is the weight-streaming GEMV): o_proj / down_proj fold their result into the residual stream themselves and leave the row sums of squares,
// qkv / gate_up build the normalised activation per lane (GemvChain, gemm_plan.h): 7 launches per layer
static int layer_tail_chain(StepRun& r, int i) {
    mmd_ctx* c = r.c; const mmd_config& g = c->cfg; LlmLayer& L = c->L[i];
    const int S = r.S, H = g.hidden_size, I = g.intermediate_size, nh = g.num_heads, d = g.head_dim; const size_t e = es(c); int splits = 1;
    int rc = slab_gemm(r, c->l_attn, (int64_t)nh * d, L.wo_p, H, nh * d, &splits, L.wo_8, L.so, &r.ch_fin); if (rc) return rc;
    r.ch_xn.xn_gamma = L.ln2;
    rc = gemm(c, c->l_xn, H, L.wgu, H, nullptr, nullptr, 0, c->l_act, I, S, 2 * I, H, EPI_SWIGLU, 0, GEMM_AUTO, L.wgu_p, false, L.wgu_8, L.sgu, &r.ch_xn); if (rc) return rc;
    const bool last = i + 1 == g.num_layers;              // the caller wants the final norm's output materialised
    rc = slab_gemm(r, c->l_act, I, L.wdown_p, H, I, &splits, L.wdown_8, L.sdown, last ? nullptr : &r.ch_fin); if (rc) return rc;
    if (last) {
        ProfScope ps(c, MMD_K_NORM_ROPE, 4.0 * S * H * e, 0);
        HIPCHK(c, launch_slab_resid_rmsnorm(c->splitk_ws, splits, S, H, c->l_h, c->l_h, next_norm(c, i), g.rms_norm_eps, next_xn(c, i), c->stream));
    }
    return MMD_OK;
}
// Fused slabs: o_proj and down_proj leave slabs, one reduce + residual + RMSNorm pass each consumes them: 9 launches per layer instead of 12
static int layer_tail_fused(StepRun& r, int i) {
    mmd_ctx* c = r.c; const mmd_config& g = c->cfg; LlmLayer& L = c->L[i]; hipStream_t st = c->stream;
    const int S = r.S, H = g.hidden_size, I = g.intermediate_size, nh = g.num_heads, d = g.head_dim; const size_t e = es(c); int splits = 1;
    int rc = slab_gemm(r, c->l_attn, (int64_t)nh * d, L.wo_p, H, nh * d, &splits, L.wo_8, L.so); if (rc) return rc;
    { ProfScope ps(c, MMD_K_NORM_ROPE, 4.0 * S * H * e, 0);
      HIPCHK(c, launch_slab_resid_rmsnorm(c->splitk_ws, splits, S, H, c->l_h, c->l_h, L.ln2, g.rms_norm_eps, c->l_xn, st)); }
    rc = gemm(c, c->l_xn, H, L.wgu, H, nullptr, nullptr, 0, c->l_act, I, S, 2 * I, H, EPI_SWIGLU, 0, GEMM_AUTO, L.wgu_p, false, L.wgu_8, L.sgu); if (rc) return rc;
    rc = slab_gemm(r, c->l_act, I, L.wdown_p, H, I, &splits, L.wdown_8, L.sdown); if (rc) return rc;
    ProfScope ps(c, MMD_K_NORM_ROPE, 4.0 * S * H * e, 0);
    HIPCHK(c, launch_slab_resid_rmsnorm(c->splitk_ws, splits, S, H, c->l_h, c->l_h, next_norm(c, i), g.rms_norm_eps, next_xn(c, i), st));
    return MMD_OK;
}
// Tile schedule: every GEMM applies its own epilogue; the plan says whether the SwiGLU product is piece-major and whether down_proj's split-K slabs go to ONE pass that
// sums them, adds the residual stream and normalises for the next layer (or the final norm) -- instead of splitk_reduce (+ residual) and a separate RMSNorm launch
static int layer_tail_tile(StepRun& r, int i) {
    mmd_ctx* c = r.c; const mmd_config& g = c->cfg; LlmLayer& L = c->L[i]; hipStream_t st = c->stream;
    const int dt = g.dtype, S = r.S, H = g.hidden_size, I = g.intermediate_size, nh = g.num_heads, d = g.head_dim; const size_t e = es(c); const bool pm = r.p.mlp_pm;
    int rc = gemm(c, c->l_attn, (int64_t)nh * d, L.wo, (int64_t)nh * d, nullptr, c->l_h, H, c->l_h, H, S, H, nh * d, EPI_RESID, 0, GEMM_AUTO, L.wo_p, false, L.wo_8, L.so); if (rc) return rc;
    { ProfScope ps(c, MMD_K_NORM_ROPE, 2.0 * S * H * e, 0); HIPCHK(c, launch_rmsnorm(dt, c->l_h, L.ln2, c->l_xn, S, H, g.rms_norm_eps, st)); }
    rc = gemm(c, c->l_xn, H, L.wgu, H, nullptr, nullptr, 0, c->l_act, I, S, 2 * I, H, EPI_SWIGLU, 0, GEMM_AUTO, L.wgu_p, false, L.wgu_8, L.sgu, nullptr, nullptr, pm ? 2 : 0); if (rc) return rc;
    int rs = 0;
    rc = gemm(c, c->l_act, I, L.wdown, I, nullptr, c->l_h, H, c->l_h, H, S, H, I, EPI_RESID, 0, GEMM_AUTO, L.wdown_p, false, L.wdown_8, L.sdown, nullptr,
              r.p.down_slab_norm ? &rs : nullptr, pm ? 1 : 0); if (rc) return rc;
    if (r.p.down_slab_norm) {
        ProfScope ps(c, MMD_K_NORM_ROPE, 4.0 * S * H * e + 4.0 * rs * S * H, 0);
        HIPCHK(c, launch_slab_resid_rmsnorm(c->splitk_ws, rs, S, H, c->l_h, c->l_h, next_norm(c, i), g.rms_norm_eps, next_xn(c, i), st, L.sdown));          // (fp8 matrices: the tile GEMM's slabs are unscaled)
        r.xn_ready = true;
    }
    return MMD_OK;
}
// The hidden states of a chunk's LAST layer are read at a few rows only (the frame-end rows of the two heads, the row whose logits are wanted); its K / V must exist
// for every token, but its o_proj and MLP are row-wise: they run on the rows somebody reads, through the weight-streaming kernels.  The reference computes all
// rows and drops them (the lm_head over all positions is "pure waste the build skips" -- the same holds one layer down).  l_hid is left compact.
static int layer_tail_sparse_last(StepRun& r, int i) {
    mmd_ctx* c = r.c; const mmd_config& g = c->cfg; LlmLayer& L = c->L[i]; hipStream_t st = c->stream;
    const int H = g.hidden_size, I = g.intermediate_size, nh = g.num_heads, d = g.head_dim, n_need = r.n_need; const size_t e = es(c);
    void* attn_c = c->l_q; void* h_c = c->l_qkv;          // (both dead here: the queries were consumed by the attention above, the fused qkv rows by RoPE + append)
    { ProfScope ps(c, MMD_K_OTHER, 0, 0);
      HIPCHK(c, launch_gather_rows2(c->l_attn, (int64_t)nh * d, attn_c, nh * d, c->l_h, H, h_c, H, r.need_rows, n_need, st)); }
    int sp = 1, rc = slab_gemm(r, attn_c, (int64_t)nh * d, L.wo_p, H, nh * d, &sp, L.wo_8, L.so, nullptr, n_need); if (rc) return rc;
    { ProfScope ps(c, MMD_K_NORM_ROPE, 4.0 * n_need * H * e, 0);
      HIPCHK(c, launch_slab_resid_rmsnorm(c->splitk_ws, sp, n_need, H, h_c, h_c, L.ln2, g.rms_norm_eps, c->l_xn, st)); }
    rc = gemm(c, c->l_xn, H, L.wgu, H, nullptr, nullptr, 0, c->l_act, I, n_need, 2 * I, H, EPI_SWIGLU, 0, GEMM_AUTO, L.wgu_p, false, L.wgu_8, L.sgu); if (rc) return rc;
    rc = slab_gemm(r, c->l_act, I, L.wdown_p, H, I, &sp, L.wdown_8, L.sdown, nullptr, n_need); if (rc) return rc;
    { ProfScope ps(c, MMD_K_NORM_ROPE, 4.0 * n_need * H * e, 0);
      HIPCHK(c, launch_slab_resid_rmsnorm(c->splitk_ws, sp, n_need, H, h_c, h_c, c->fnorm, g.rms_norm_eps, c->l_hid, st)); }
    c->hid_compact = n_need;
    r.xn_ready = true;          // (the final norm is done)
    return MMD_OK;
}
static int llm_step_segs(mmd_ctx* c, const StepSeg* segs, int nseg, const void* embeds, int S, void* hidden_out, const StepState* dyn, const int32_t* need_rows = nullptr, int n_need = 0) {
    NEED_FINAL(c);
    c->hid_compact = 0;
    if (S <= 0 || nseg <= 0) return MMD_OK;
    const mmd_config& g = c->cfg; const int dt = g.dtype, H = g.hidden_size; const size_t e = es(c); hipStream_t st = c->stream;
    if (S > g.max_step_tokens) FAIL(c, MMD_ERANGE, "step of %d tokens exceeds max_step_tokens %d", S, g.max_step_tokens);
    int rc = MMD_OK; int rows_few[16]; std::vector<int> rows_many(nseg > 16 ? nseg : 0); int* seg_rows = nseg > 16 ? rows_many.data() : rows_few;          // (no allocation for the usual few streams)
    {
        int at = 0;
        for (int j = 0; j < nseg; ++j) {
            if (!segs[j].s || segs[j].s->ctx != c) FAIL(c, MMD_EINVAL, "stream does not belong to this context");
            if (segs[j].rows <= 0 || segs[j].row0 != at) FAIL(c, MMD_EINVAL, "segments must be non-empty and consecutive");
            for (int k = 0; k < j; ++k) if (segs[k].s == segs[j].s) FAIL(c, MMD_EINVAL, "a stream may appear once per step");
            at += segs[j].rows; seg_rows[j] = segs[j].rows;
        }
        if (at != S) FAIL(c, MMD_EINVAL, "segments cover %d rows of a %d-row step", at, S);
    }
    if (!dyn) for (int j = 0; j < nseg; ++j) { rc = kv_reserve(c, segs[j].s, segs[j].s->len + segs[j].rows); if (rc) return rc; }
    StepShape shape;
    shape.S = S; shape.seg_rows = seg_rows; shape.nseg = nseg; shape.n_need = need_rows ? n_need : 0; shape.hidden_out = hidden_out != nullptr; shape.dyn = dyn != nullptr;
    StepRun r{c, segs, nseg, S, dyn, need_rows, n_need, step_plan(step_model(c), shape, c->sw, gemm_tuning())};
    const StepPlan& p = r.p;
    if (p.rc) FAIL(c, p.rc, "%s", p.error);
    if (p.sparse_last) for (int k = 0; k < n_need; ++k) if (need_rows[k] < 0 || need_rows[k] >= S) FAIL(c, MMD_ERANGE, "needed row %d outside the step", need_rows[k]);
    p.fields(c->step_last);
    if (embeds != c->l_h) HIPCHK(c, hipMemcpyAsync(c->l_h, embeds, (size_t)S * H * e, hipMemcpyDeviceToDevice, st));

    const bool tile = p.schedule == STEP_TILE;
    r.ch_fin.fin_h = c->l_h; r.ch_fin.fin_ssq = c->chain_ssq; r.ch_xn.xn_h = c->l_h; r.ch_xn.xn_ssq = c->chain_ssq; r.ch_xn.xn_eps = g.rms_norm_eps;
    if (!tile) { ProfScope ps(c, MMD_K_NORM_ROPE, 2.0 * S * H * e, 0); HIPCHK(c, launch_rmsnorm(dt, c->l_h, c->L[0].ln1, c->l_xn, S, H, g.rms_norm_eps, st)); }
    if (p.run_n > 0) { rc = upload_seg_states(r); if (rc) return rc; }
    // one (cos, sin) table per step and segment: read by the attention kernel's own q / k / v preparation, or by the vectorised RoPE + append kernel of every layer of a chunk
    if (p.rope_fused || p.chunk_rope) for (int j = 0; j < nseg; ++j) HIPCHK(c, launch_rope_table((char*)c->rope_tab + (size_t)segs[j].row0 * 64 * 8, segs[j].rows, 64, c->inv_freq, segs[j].s->len + segs[j].s->pos_off, st, dyn));
    for (int i = 0; i < g.num_layers; ++i) {
        int splits = 1;
        rc = layer_qkv(r, i, &splits); if (rc) return rc;
        rc = layer_attention(r, i, splits); if (rc) return rc;
        if (p.sparse_last && i + 1 == g.num_layers) rc = layer_tail_sparse_last(r, i);
        else rc = p.schedule == STEP_CHAIN ? layer_tail_chain(r, i) : p.schedule == STEP_FUSED ? layer_tail_fused(r, i) : layer_tail_tile(r, i);
        if (rc) return rc;
    }
    if (tile && !r.xn_ready) { ProfScope ps(c, MMD_K_NORM_ROPE, 2.0 * S * H * e, 0); HIPCHK(c, launch_rmsnorm(dt, c->l_h, c->fnorm, c->l_hid, S, H, g.rms_norm_eps, st)); }
    if (hidden_out) HIPCHK(c, hipMemcpyAsync(hidden_out, c->l_hid, (size_t)S * H * e, hipMemcpyDeviceToDevice, st));
    if (!dyn) for (int j = 0; j < nseg; ++j) segs[j].s->len += segs[j].rows;
    return MMD_OK;
}

static int llm_step_impl(mmd_ctx* c, mmd_stream* s, const void* embeds, int S, void* hidden_out, const StepState* dyn) {
    if (!c) return MMD_EINVAL;
    if (!s || s->ctx != c) FAIL(c, MMD_EINVAL, "stream does not belong to this context");
    if (S <= 0) return MMD_OK;
    StepSeg one{s, 0, S};
    return llm_step_segs(c, &one, 1, embeds, S, hidden_out, dyn);
}

extern "C" int mmd_llm_step(mmd_ctx* c, mmd_stream* s, const void* embeds, int S, void* hidden_out) {
    return llm_step_impl(c, s, embeds, S, hidden_out, nullptr);
}

static int build_segs(mmd_ctx* c, mmd_stream* const* streams, const int32_t* seg_rows, int n_segs, std::vector<StepSeg>& segs, int* S_out) {
    if (!streams || !seg_rows || n_segs <= 0) FAIL(c, MMD_EINVAL, "multi-stream step needs at least one segment");
    int at = 0;
    segs.resize(n_segs);
    for (int j = 0; j < n_segs; ++j) { segs[j] = StepSeg{streams[j], at, seg_rows[j]}; at += seg_rows[j]; }
    *S_out = at;
    return MMD_OK;
}

extern "C" int mmd_llm_step_multi(mmd_ctx* c, mmd_stream* const* streams, const int32_t* seg_rows, int n_segs, const void* embeds, void* hidden_out) {
    if (!c) return MMD_EINVAL;
    std::vector<StepSeg> segs; int S = 0;
    int rc = build_segs(c, streams, seg_rows, n_segs, segs, &S); if (rc) return rc;
    return llm_step_segs(c, segs.data(), n_segs, embeds, S, hidden_out, nullptr);
}

// the rows whose final hidden state a step's caller reads, `a` first and `b` behind it (llm_step_segs may then leave l_hid compact, in this order); more than STEP_NEED_MAX: no list
static int build_need_list(const int32_t* a, int na, const int32_t* b, int nb, int32_t need[STEP_NEED_MAX]) {
    int n = 0;
    if (na + nb <= STEP_NEED_MAX) { for (int i = 0; i < na; ++i) need[n++] = a[i]; for (int i = 0; i < nb; ++i) need[n++] = b[i]; }
    return n;
}
// enqueue the 4 head logits of n rows of l_hid (`compact`: its first n rows) and their copy into heads_host; the caller synchronises and reads heads_host
static int read_head_rows(mmd_ctx* c, const int32_t* rows, int n, bool compact) {
    hipStream_t st = c->stream; const int H = c->cfg.hidden_size;
    for (int i = 0; i < n; ++i) c->rows_host[i] = compact ? i : rows[i];
    HIPCHK(c, hipMemcpyAsync(c->rows_dev, c->rows_host, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    { ProfScope ps(c, MMD_K_OTHER, 0, 0);
      HIPCHK(c, launch_heads(c->cfg.dtype, c->l_hid, H, c->rows_dev, n, c->heads4, H, c->heads_dev, st)); }
    HIPCHK(c, hipMemcpyAsync(c->heads_host, c->heads_dev, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, st));
    return MMD_OK;
}

extern "C" int mmd_frame_step_multi(mmd_ctx* c, mmd_stream* const* streams, const int32_t* seg_rows, int n_segs, const void* embeds,
                                    const int32_t* head_rows, int n_head_rows, float* heads_out_host,
                                    const int32_t* hidden_rows, int n_hidden_rows, void* hidden_rows_out, float* logits_out) {
    if (!c) return MMD_EINVAL;
    NEED_FINAL(c);
    std::vector<StepSeg> segs; int S = 0;
    int rc = build_segs(c, streams, seg_rows, n_segs, segs, &S); if (rc) return rc;
    if (n_head_rows < 0 || n_head_rows > S || n_hidden_rows < 0 || n_hidden_rows > S) FAIL(c, MMD_EINVAL, "bad row count");
    if ((n_head_rows && (!head_rows || !heads_out_host)) || (n_hidden_rows && (!hidden_rows || !hidden_rows_out))) FAIL(c, MMD_EINVAL, "null row/result pointer");
    for (int i = 0; i < n_head_rows; ++i) if (head_rows[i] < 0 || head_rows[i] >= S) FAIL(c, MMD_ERANGE, "head row %d outside the step", head_rows[i]);
    for (int i = 0; i < n_hidden_rows; ++i) if (hidden_rows[i] < 0 || hidden_rows[i] >= S) FAIL(c, MMD_ERANGE, "hidden row %d outside the step", hidden_rows[i]);
    int32_t need[STEP_NEED_MAX]; const int n_need = build_need_list(head_rows, n_head_rows, hidden_rows, n_hidden_rows, need);          // heads first, then the hidden / logit rows
    rc = llm_step_segs(c, segs.data(), n_segs, embeds, S, nullptr, nullptr, n_need ? need : nullptr, n_need); if (rc) return rc;
    const bool compact = c->hid_compact > 0;
    hipStream_t st = c->stream; const int H = c->cfg.hidden_size; const size_t e = es(c);
    for (int i = 0; i < n_hidden_rows; ++i)
        HIPCHK(c, hipMemcpyAsync((char*)hidden_rows_out + (size_t)i * H * e, (char*)c->l_hid + (size_t)(compact ? n_head_rows + i : hidden_rows[i]) * H * e, (size_t)H * e, hipMemcpyDeviceToDevice, st));
    if (n_hidden_rows && logits_out) { rc = mmd_lm_head(c, hidden_rows_out, n_hidden_rows, logits_out); if (rc) return rc; }
    if (n_head_rows) {
        rc = read_head_rows(c, head_rows, n_head_rows, compact); if (rc) return rc;
        HIPCHK(c, hipStreamSynchronize(st));
        memcpy(heads_out_host, c->heads_host, sizeof(float) * 4 * n_head_rows);
    }
    return MMD_OK;
}

// ---- scheduler rounds of several streams with the greedy sampling on the device ---------------------------------------------------------------
// models/modeling_live.py:51-77 is a per-stream token loop; with several streams per GPU (mmduet_amd/multistream.py) the loops of all talking streams advance together,
// one token per round, inside the forwards that also carry the watching streams' frame chunks.
struct mmd_sampler {
    mmd_ctx* ctx;
    int64_t* tok_dev = nullptr;                  // the token drawn last (fed back by the next round's embedding gather)
    int64_t eos = -1;
    // sampling (mmd_sampler_set_sampling): off = arg-max.  `offset` counts the tokens drawn since the seed was set; `lane` is the sampler's id within its context
    bool sampling = false, seeded = false; float temperature = 1.f, top_p = 1.f; int top_k = 0; uint64_t seed = 0, offset = 0; uint32_t lane = 0;
    // the response of its rounds: the penalty list, the constraints (mmd_sampler_set_constraints), the records (mmd_sampler_set_logprobs; sized for the response's max_new)
    // and the counters -- tokens returned, records returned, whether the response is over
    Response resp;
};

// ---- constraints: the device descriptors -----------------------------------------------------------------------------------------------------------------------------------
// a set through constraint_set() (response_plan.h: the limits, the order of the checks and their messages); a refusal becomes the context's error
static int cons_checked(mmd_ctx* c, int V, const int64_t* eos_ids, int n_eos, int min_new, const int32_t* ids, const float* bias, int n, ConsSet& out) {
    const ConsSetResult r = constraint_set(V, eos_ids, n_eos, min_new, ids, bias, n);
    if (r.rc) FAIL(c, r.rc, "%s", r.error);
    out = r.set;
    return MMD_OK;
}
// the device descriptor of a set: the EOS ids are response_eos()'s answer, the same the host stops on
static void cons_fill_row(ConstraintRow& r, const ConsSet& s, const int32_t* ids_dev, const float* bias_dev, const ResponseEos& eos, int step, const int* step_ptr) {
    r.ids = ids_dev; r.bias = bias_dev; r.step_ptr = step_ptr; r.n = s.n; r.min_new = s.min_new; r.step = step;
    r.n_eos = eos.n;
    for (int k = 0; k < CONS_MAX_EOS; ++k) r.eos[k] = k < eos.n ? eos.ids[k] : -1;
}
static void cons_fill_row(ConstraintRow& r, const Response& rs, const ResponseEos& eos) { cons_fill_row(r, rs.cons, rs.cons_ids_dev, rs.cons_bias_dev, eos, rs.count.step, nullptr); }
// the row descriptors of constrained selections, on the device and pinned
static int cons_reserve(mmd_ctx* c) {
    if (c->cons_rows_host) return MMD_OK;
    int rc = dev_alloc(c, (void**)&c->cons_rows_dev, (size_t)(1 + MMD_ROUND_MAX_SAMPLERS) * sizeof(ConstraintRow)); if (rc) return rc;
    return host_alloc(c, (void**)&c->cons_rows_host, (size_t)(1 + MMD_ROUND_MAX_SAMPLERS) * sizeof(ConstraintRow));
}

// one draw's parameters
struct SampleArgs { float temperature; int top_k; float top_p; uint64_t seed; uint64_t* offset_inout; };
// every field of a row descriptor.  pen off: no list entry counts and the penalty is 1; n_prev_ptr (a decode step: &StepState::n_prev) overrides n_prev on the device
static void fill_sample_row(SampleRow& r, const SampleArgs& a, const int64_t* prev, bool pen, int n_prev, int prev_cap, float penalty, const int* n_prev_ptr, int64_t* tok,
                            int64_t* append, uint32_t lane, uint32_t advance) {
    r.prev = prev; r.n_prev_ptr = n_prev_ptr; r.tok = tok; r.append = append; r.offset = *a.offset_inout;
    r.n_prev = pen ? n_prev : 0; r.prev_cap = prev_cap; r.penalty = pen ? penalty : 1.f; r.temperature = a.temperature; r.top_k = a.top_k; r.top_p = a.top_p;
    r.seed_lo = (uint32_t)a.seed; r.seed_hi = (uint32_t)(a.seed >> 32); r.lane = lane; r.advance = advance;
}
// ... of a response's row: its list at the length that counts now
static void fill_sample_row(SampleRow& r, const SampleArgs& a, const Response& rs, const int* n_prev_ptr, int64_t* tok, int64_t* append, uint32_t lane, uint32_t advance) {
    fill_sample_row(r, a, rs.prev_dev, rs.penalty > 0.f, rs.count.n_prev, rs.prev_cap, rs.penalty, n_prev_ptr, tok, append, lane, advance);
}
static int sample_reserve(mmd_ctx* c) {
    if (c->samp_scratch) return MMD_OK;
    int rc = dev_alloc(c, (void**)&c->samp_rows_dev, (size_t)(1 + MMD_ROUND_MAX_SAMPLERS) * sizeof(SampleRow)); if (rc) return rc;
    rc = host_alloc(c, (void**)&c->samp_rows_host, (size_t)(1 + MMD_ROUND_MAX_SAMPLERS) * sizeof(SampleRow)); if (rc) return rc;
    return dev_alloc(c, &c->samp_scratch, sample_topkp_scratch_bytes(c->cfg.vocab_size, MMD_ROUND_MAX_SAMPLERS, true), false);
}
static int check_sampling(mmd_ctx* c, float temperature, int top_k, float top_p) {
    if (!(temperature > 0.f) || top_k < 0 || !(top_p > 0.f && top_p <= 1.f)) FAIL(c, MMD_EINVAL, "sampling needs temperature > 0, top_k >= 0, 0 < top_p <= 1 (got %g, %d, %g)", temperature, top_k, top_p);
    return MMD_OK;
}
// the rows of a selection as select_plan() takes them
static SelectRows select_rows(bool sampled, bool constrained, bool record, int n, bool single, bool dyn, int V, const SampleArgs* a) {
    SelectRows r;
    r.sampled = sampled; r.constrained = constrained; r.record = record; r.n = n; r.single = single; r.dyn = dyn; r.V = V;
    if (a) { r.top_k = a->top_k; r.top_p = a->top_p; }
    return r;
}
static int select_refused(mmd_ctx* c, const SelectPlan& p) { if (p.rc) FAIL(c, p.rc, "%s", p.error); return MMD_OK; }

// ---- the one place a token selection is launched from ---------------------------------------------------------------------------------------------------
// Everything a selection's launches are handed besides the plan; which of it a launch reads is the plan's business (select_plan.h), nothing is decided here.
struct SelectIO {
    const float* logits; int V, n;     // [n, V] fp32
    SampleRow* rows; const ConstraintRow* cons; const LogprobOut* lp;          // descriptors on the device, one per row; where the records go
    int64_t* toks;                     // tokens out (a draw may have none: its rows' descriptors name the slots)
    void* scratch; void* lp_scratch;   // the chain's and the records' scratch
    void* am_scratch = nullptr;        // the arg-max's candidates
    const SampleBatch* batch = nullptr;          // SEL_ARGMAX over a block: the rows' lists and slots
    const int64_t* prev = nullptr; int n_prev = 0; float penalty = 1.f; const StepState* dyn = nullptr;          // SEL_ARGMAX, single: the list rides in kernel arguments
    const unsigned long long* r_words = nullptr; float* info = nullptr; float* scores = nullptr;          // the raw operator's: explicit random words, the draw's info, the z rows
    // A round's block: only its tail [rec0, n) records.  The launches that exist for the record alone run over the tail; a draw writes sampling_logprob for every row whose
    // LogprobRow names a destination.  SEL_ARGMAX: `rows` describes the tail's rows alone (the arg-max reads `batch`).  0: every row records (the generate calls, the operators).
    int rec0 = 0;
};
static hipError_t select_enqueue(mmd_ctx* c, const SelectPlan& p, const SelectIO& io) {
    hipStream_t st = c->stream; hipError_t e = hipSuccess;
    const ConstraintRow* cons = p.needs_cons ? io.cons : nullptr;
    const LogprobOut* lp = p.record ? io.lp : nullptr;
    const int t0 = p.record ? io.rec0 : 0, tn = io.n - t0;          // the recording tail
    const float* tail_logits = io.logits + (size_t)t0 * io.V;
    p.fields(c->select_last);
    switch (p.kind) {
    case SEL_DRAW:          // (the draw records sampling_logprob itself)
        e = launch_sample_batch_topkp(io.logits, io.V, io.n, io.rows, p.any_k, p.any_p, io.r_words, io.toks, io.info, io.scores, io.scratch, st, lp, cons);
        break;
    case SEL_CONS_ARGMAX:          // the chain's scores with nothing filtered, then the first maximal index of z
        e = launch_sample_scores_unfiltered(io.logits, io.V, io.n, io.rows, io.scores, io.scratch, st, cons);
        if (e == hipSuccess) e = launch_argmax_scores(io.V, io.n, io.rows, io.scores, io.scratch, io.toks, st);
        break;
    default:
        e = p.single ? launch_argmax_penalty(io.logits, io.V, io.prev, io.n_prev, io.penalty, io.toks, st, io.dyn, io.am_scratch)
                     : launch_sample_batch(io.logits, io.V, *io.batch, io.n, io.toks, io.am_scratch, st);
        if (e == hipSuccess && p.scores_after_argmax) e = launch_sample_scores_unfiltered(tail_logits, io.V, tn, io.rows, io.scores ? io.scores + (size_t)t0 * io.V : nullptr, io.scratch, st);
    }
    if (e == hipSuccess && p.record) {
        LogprobOut tail = *lp;
        tail.toks += t0; tail.idx0 += t0; if (tail.rows) tail.rows += t0;
        const bool own_scores = p.kind == SEL_ARGMAX;          // the scores behind a plain arg-max ran over the tail alone; a constrained block's ran over all of its rows
        e = launch_logprob_rows(tail_logits, io.V, tn, tail, p.record_greedy, own_scores && io.scores ? io.scores + (size_t)t0 * io.V : io.scores, io.scratch, io.lp_scratch, st,
                                own_scores ? 0 : io.n, own_scores ? 0 : t0);
    }
    return e;
}

extern "C" int mmd_sampler_create(mmd_ctx* c, mmd_sampler** out) {
    NEED_FINAL(c);
    if (!out) FAIL(c, MMD_EINVAL, "null out pointer");
    mmd_sampler* sp = new (std::nothrow) mmd_sampler();
    if (!sp) FAIL(c, MMD_ENOMEM, "out of host memory");
    sp->ctx = c; sp->lane = c->n_samplers++;
    if (hipMalloc((void**)&sp->tok_dev, 64) != hipSuccess) { delete sp; FAIL(c, MMD_ENOMEM, "hipMalloc of a sampler failed"); }
    // the slot is zeroed before the call returns: c->stream is whatever stream the context was last bound to -- possibly the tower's side stream with batches queued on
    // it -- while the rounds that write and read the slot run on the caller's stream; a fill still pending there would wipe a drawn token before the next round feeds it
    hipError_t e = hipMemsetAsync(sp->tok_dev, 0, 64, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { hipFree(sp->tok_dev); delete sp; FAIL(c, MMD_EHIP, "zeroing a sampler failed: %s", hipGetErrorString(e)); }
    *out = sp;
    return MMD_OK;
}
extern "C" void mmd_sampler_destroy(mmd_sampler* sp) {
    if (!sp) return;
    hipSetDevice(sp->ctx->device);
    hipStreamSynchronize(sp->ctx->stream);
    if (sp->tok_dev) hipFree(sp->tok_dev);
    response_release(sp->ctx, sp->resp);
    delete sp;
}
// the records of a response: room for max_new of them once the sampler records
static int sampler_lp_reserve(mmd_sampler* sp) {
    if (sp->resp.lp_top < 0) return MMD_OK;
    return response_reserve_records(sp->ctx, sp->resp, sampler_records_need(sp->resp.count.max_new), RESPONSE_SAMPLER_RECORDS_FIRST);
}
extern "C" int mmd_sampler_begin(mmd_sampler* sp, int64_t eos_id, float rep_penalty, const int64_t* prev_ids_host, int n_prev, int max_new) {
    if (!sp) return MMD_EINVAL;
    mmd_ctx* c = sp->ctx; hipSetDevice(c->device);
    if (n_prev < 0 || max_new < 0 || (n_prev > 0 && !prev_ids_host)) FAIL(c, MMD_EINVAL, "bad sampler arguments");
    Response& r = sp->resp;
    sp->eos = eos_id; r.penalty = rep_penalty > 0.f ? rep_penalty : 0.f;
    r.count = ResponseCount{}; r.count.max_new = max_new;
    int rc = sampler_lp_reserve(sp); if (rc) return rc;
    if (r.penalty <= 0.f) return MMD_OK;
    rc = response_reserve_list(c, r, sampler_prev_need(n_prev, max_new), RESPONSE_SAMPLER_PREV_FIRST); if (rc) return rc;
    // (pageable host memory: the copy is staged before the call returns, the caller's list may change afterwards)
    if (n_prev > 0) HIPCHK(c, hipMemcpyAsync(r.prev_dev, prev_ids_host, sizeof(int64_t) * n_prev, hipMemcpyHostToDevice, c->stream));
    r.count.n_prev = n_prev;
    return MMD_OK;
}
extern "C" int mmd_sampler_prev_len(const mmd_sampler* sp) { return sp ? sp->resp.count.n_prev : MMD_EINVAL; }
extern "C" int mmd_sampler_set_sampling(mmd_sampler* sp, float temperature, int top_k, float top_p, uint64_t seed) {
    if (!sp) return MMD_EINVAL;
    mmd_ctx* c = sp->ctx;
    if (!(temperature > 0.f)) { sp->sampling = false; return MMD_OK; }
    int rc = check_sampling(c, temperature, top_k, top_p); if (rc) return rc;
    rc = select_refused(c, select_plan(select_rows(true, false, false, 1, false, false, c->cfg.vocab_size, nullptr))); if (rc) return rc;
    if (!sp->seeded || seed != sp->seed) { sp->seed = seed; sp->offset = 0; sp->seeded = true; }
    sp->sampling = true; sp->temperature = temperature; sp->top_k = top_k; sp->top_p = top_p;
    return MMD_OK;
}
extern "C" int mmd_sampler_set_constraints(mmd_sampler* sp, const int64_t* eos_ids_host, int n_eos, int min_new, const int32_t* ids_host, const float* bias_host, int n) {
    if (!sp) return MMD_EINVAL;
    mmd_ctx* c = sp->ctx; hipSetDevice(c->device);
    ConsSet s; int rc = cons_checked(c, c->cfg.vocab_size, eos_ids_host, n_eos, min_new, ids_host, bias_host, n, s); if (rc) return rc;
    if (s.on) {
        rc = select_refused(c, select_plan(select_rows(false, true, false, 1, false, false, c->cfg.vocab_size, nullptr))); if (rc) return rc;
        rc = cons_reserve(c); if (rc) return rc;
    }
    return response_set_constraints(c, sp->resp, s);
}
extern "C" int mmd_sampler_set_logprobs(mmd_sampler* sp, int top_n) {
    if (!sp) return MMD_EINVAL;
    mmd_ctx* c = sp->ctx; hipSetDevice(c->device);
    ResponseCount& n = sp->resp.count;
    int rc = response_lp_top_checked(c, top_n); if (rc) return rc;
    if (n.step > 0 && !n.ended) FAIL(c, MMD_EINVAL, "the response has returned %d token(s): log-probabilities are switched at a response boundary", n.step);
    if (top_n >= 0) { rc = select_refused(c, select_plan(select_rows(false, false, true, 1, false, false, c->cfg.vocab_size, nullptr))); if (rc) return rc; }
    sp->resp.lp_top = top_n; n.lp_n = 0;          // (behind a finished response: its records go with the setting they were written under)
    return sampler_lp_reserve(sp);
}
extern "C" int mmd_sampler_logprobs_read(mmd_sampler* sp, float* logprob_host, float* sampling_logprob_host, int64_t* top_ids_host, float* top_logprob_host, int cap_tokens, int* n_out) {
    if (!sp) return MMD_EINVAL;
    mmd_ctx* c = sp->ctx; hipSetDevice(c->device);
    if (!n_out || cap_tokens < 0) FAIL(c, MMD_EINVAL, "bad mmd_sampler_logprobs_read arguments");
    const int n = sp->resp.lp_top >= 0 ? sp->resp.count.lp_n : 0;
    *n_out = n;
    if (n == 0) return MMD_OK;
    return response_read_records(c, sp->resp, n, sp->resp.lp_top, logprob_host, sampling_logprob_host, top_ids_host, top_logprob_host, cap_tokens);
}
// the round's record descriptors and the record kernels' scratch for a round's rows
static int round_record_reserve(mmd_ctx* c) {
    if (c->round_lp_scratch) return MMD_OK;
    int rc = dev_alloc(c, (void**)&c->round_lp_rows_dev, MMD_ROUND_MAX_SAMPLERS * sizeof(LogprobRow)); if (rc) return rc;
    rc = host_alloc(c, (void**)&c->round_lp_rows_host, MMD_ROUND_MAX_SAMPLERS * sizeof(LogprobRow)); if (rc) return rc;
    return dev_alloc(c, &c->round_lp_scratch, logprob_scratch_bytes(MMD_ROUND_MAX_SAMPLERS), false);
}
extern "C" int mmd_sampler_lane(const mmd_sampler* sp) { return sp ? (int)sp->lane : MMD_EINVAL; }
extern "C" int64_t mmd_sampler_offset(const mmd_sampler* sp) { return sp ? (int64_t)sp->offset : MMD_EINVAL; }

extern "C" int mmd_round_multi(mmd_ctx* c, mmd_stream* const* streams, const int32_t* seg_rows, int n_segs, const void* const* seg_embeds, mmd_sampler* const* samplers,
                               const int32_t* seg_flags, const int32_t* head_rows, int n_head_rows, float* heads_out_host, int64_t* tokens_out_host) {
    if (!c) return MMD_EINVAL;
    NEED_FINAL(c);
    std::vector<StepSeg> segs; int S = 0;
    int rc = build_segs(c, streams, seg_rows, n_segs, segs, &S); if (rc) return rc;
    if (S > c->cfg.max_step_tokens) FAIL(c, MMD_ERANGE, "round of %d tokens exceeds max_step_tokens %d", S, c->cfg.max_step_tokens);
    if (n_head_rows < 0 || n_head_rows > S || (n_head_rows && (!head_rows || !heads_out_host))) FAIL(c, MMD_EINVAL, "bad head rows");
    for (int i = 0; i < n_head_rows; ++i) if (head_rows[i] < 0 || head_rows[i] >= S) FAIL(c, MMD_ERANGE, "head row %d outside the round", head_rows[i]);
    hipStream_t st = c->stream; const int H = c->cfg.hidden_size, V = c->cfg.vocab_size; const size_t e = es(c);
    // the round's input rows: embeddings handed in per segment, or -- FEED -- the embedding of the token the segment's sampler drew in the round before
    FeedBatch feed; int n_feed = 0;
    std::vector<RoundSeg> rsegs((size_t)n_segs);
    for (int j = 0; j < n_segs; ++j) {
        const int fl = seg_flags ? seg_flags[j] : 0;
        mmd_sampler* sp = samplers ? samplers[j] : nullptr;
        if ((fl & (MMD_SEG_FEED | MMD_SEG_SAMPLE)) && (!sp || sp->ctx != c)) FAIL(c, MMD_EINVAL, "segment %d feeds / samples without a sampler of this context", j);
        RoundSeg& r = rsegs[j];
        r.feed = (fl & MMD_SEG_FEED) != 0; r.sample = (fl & MMD_SEG_SAMPLE) != 0; r.rows = segs[j].rows;
        if (sp) { r.sampling = sp->sampling; r.constrained = sp->resp.cons.on; r.sampler = (int)sp->lane; r.top_k = sp->top_k; r.top_p = sp->top_p; }          // (lane: the sampler's index within its context)
        if (sp && sp->resp.lp_top >= 0) { r.record = true; r.lp_top = sp->resp.lp_top; }
        if (r.feed) {
            if (n_feed >= MMD_ROUND_MAX_SAMPLERS) FAIL(c, MMD_ERANGE, "more than %d feed segments", MMD_ROUND_MAX_SAMPLERS);
            feed.tok[n_feed] = sp->tok_dev; feed.row[n_feed] = segs[j].row0; ++n_feed;
        } else {
            if (!seg_embeds || !seg_embeds[j]) FAIL(c, MMD_EINVAL, "segment %d has no input rows", j);
            void* dst = (char*)c->l_h + (size_t)segs[j].row0 * H * e;
            if (seg_embeds[j] != dst) HIPCHK(c, hipMemcpyAsync(dst, seg_embeds[j], (size_t)segs[j].rows * H * e, hipMemcpyDeviceToDevice, st));
        }
    }
    // sampling rows: three blocks of logits rows, plain arg-max | constrained arg-max | sampled (round_blocks).  The last two have row descriptors (and constraint descriptors,
    // empty for an unconstrained sampled row) in slots 1.. of the context's arrays, in the order of their logits rows.  A block's recording rows are its tail: a recording row
    // has a LogprobRow (slot sp->step of the sampler's own records), and the plain block's tail gets row descriptors of its own behind the others -- T = 1, the penalty list at
    // its length before this token, no token or append slot: the arg-max has written both.  (plain tail + the other two blocks <= 32 rows: the arrays' 1 + 32 slots hold them.)
    const RoundBlocks rb = round_blocks(rsegs.data(), n_segs, V);
    if (rb.rc) FAIL(c, rb.rc, "%s", rb.error);
    const int n_plain = rb.n_plain, n_greedy = rb.n_greedy, n_sample = rb.n_sample; const int* sample_seg = rb.order;
    SampleBatch sb; int32_t sample_row[MMD_ROUND_MAX_SAMPLERS]; uint64_t no_offset = 0;
    const int nd = n_sample - n_plain, plain_tail = rb.rec_rows(SEL_ARGMAX), n_rec = plain_tail + rb.rec_rows(SEL_CONS_ARGMAX) + rb.rec_rows(SEL_DRAW);
    static_assert(SELECT_ROUND_MAX_ROWS == MMD_ROUND_MAX_SAMPLERS, "the descriptor arrays hold 1 + MMD_ROUND_MAX_SAMPLERS rows");
    if (nd > 0 || plain_tail > 0) { rc = sample_reserve(c); if (rc) return rc; }
    if (n_rec > 0) { rc = round_record_reserve(c); if (rc) return rc; }
    for (int i = 0; i < n_sample; ++i) {
        const int j = sample_seg[i]; mmd_sampler* sp = samplers[j]; const Response& r = sp->resp;
        const bool pen = r.penalty > 0.f;
        int64_t* append = (pen && r.count.n_prev < r.prev_cap) ? r.prev_dev + r.count.n_prev : nullptr;
        sample_row[i] = segs[j].row0 + segs[j].rows - 1;
        if (n_rec > 0) c->round_lp_rows_host[i] = r.lp_top >= 0 ? LogprobRow{r.lp_rec, r.count.step, r.lp_cap, r.lp_top} : LogprobRow{nullptr, 0, 0, 0};
        if (i < n_plain) {
            sb.prev[i] = r.prev_dev; sb.n_prev[i] = pen ? r.count.n_prev : 0; sb.penalty[i] = pen ? r.penalty : 1.f; sb.tok[i] = sp->tok_dev; sb.append[i] = append;
            if (i >= rb.rec0[SEL_ARGMAX]) fill_sample_row(c->samp_rows_host[1 + nd + (i - rb.rec0[SEL_ARGMAX])], SampleArgs{1.f, 0, 1.f, 0, &no_offset}, r, nullptr, nullptr, nullptr, 0, 0);
            continue;
        }
        if (r.cons.on) { rc = cons_reserve(c); if (rc) return rc; }
        const bool draw = i >= n_greedy;
        const SampleArgs a = draw ? SampleArgs{sp->temperature, sp->top_k, sp->top_p, sp->seed, &sp->offset} : SampleArgs{1.f, 0, 1.f, 0, &no_offset};
        const int slot = 1 + i - n_plain;
        fill_sample_row(c->samp_rows_host[slot], a, r, nullptr, sp->tok_dev, append, draw ? sp->lane : 0, 0);
        if (c->cons_rows_host) {
            if (r.cons.on) cons_fill_row(c->cons_rows_host[slot], r, response_eos(r.cons, sp->eos, V));
            else c->cons_rows_host[slot] = ConstraintRow{};
        }
    }
    c->select_last[SELECT_PLAN_FIELDS] = SELECT_OF_ROUND; rb.fields(c->select_last + SELECT_PLAN_FIELDS + 1);
    rb.record_fields(c->round_record_last);
    if (n_sample && !tokens_out_host) FAIL(c, MMD_EINVAL, "sampling segments need tokens_out_host");
    if (n_feed) { ProfScope ps(c, MMD_K_OTHER, 0, 0); HIPCHK(c, launch_embed_feed(c->cfg.dtype, c->embed, feed, n_feed, H, V, c->l_h, st)); }
    if (n_sample && !c->round_logits) {
        rc = dev_alloc(c, (void**)&c->round_logits, (size_t)MMD_ROUND_MAX_SAMPLERS * V * sizeof(float), false); if (rc) return rc;
        rc = dev_alloc(c, &c->round_hidden, (size_t)MMD_ROUND_MAX_SAMPLERS * H * e); if (rc) return rc;
        if (!c->round_scratch) { rc = dev_alloc(c, &c->round_scratch, sample_batch_scratch_bytes()); if (rc) return rc; }          // (mmd_op_argmax may have brought it)
        rc = dev_alloc(c, (void**)&c->round_toks_dev, MMD_ROUND_MAX_SAMPLERS * sizeof(int64_t)); if (rc) return rc;
        rc = host_alloc(c, (void**)&c->round_toks_host, MMD_ROUND_MAX_SAMPLERS * sizeof(int64_t)); if (rc) return rc;
    }
    int32_t need[STEP_NEED_MAX]; const int n_need = build_need_list(head_rows, n_head_rows, sample_row, n_sample, need);          // the heads' rows first, then the sampling rows
    rc = llm_step_segs(c, segs.data(), n_segs, c->l_h, S, nullptr, nullptr, n_need ? need : nullptr, n_need); if (rc) return rc;
    const bool compact = c->hid_compact > 0;
    if (n_sample) {
        const void* rows = nullptr;
        if (compact) rows = (const char*)c->l_hid + (size_t)n_head_rows * H * e;          // already gathered, in the order of the need list
        else if (n_sample == 1) rows = (const char*)c->l_hid + (size_t)sample_row[0] * H * e;
        else {
            ProfScope ps(c, MMD_K_OTHER, 0, 0);
            HIPCHK(c, launch_gather_rows2(c->l_hid, (int64_t)H * (int64_t)(e / 2), c->round_hidden, H * (int)(e / 2), c->l_hid, (int64_t)H * (int64_t)(e / 2), c->l_xn, H * (int)(e / 2), sample_row, n_sample, st));
            rows = c->round_hidden;
        }
        rc = gemm(c, rows, H, c->lm_head, H, nullptr, nullptr, 0, c->round_logits, V, n_sample, V, H, EPI_NONE, 1, GEMM_AUTO, c->lm_head_p); if (rc) return rc;
        // one block of the round's logits rows; the descriptors of a row behind the plain ones sit in slot 1 + (row - n_plain).  (The sampled rows reuse the constrained arg-max's scratch: same stream.)
        auto block = [&](int kind) -> hipError_t {
            const SelectPlan p = rb.plan(kind);
            const int r0 = rb.row0(kind);
            SelectIO io{};
            io.logits = c->round_logits + (size_t)r0 * V; io.V = V; io.n = rb.rows(kind); io.toks = c->round_toks_dev + r0;
            if (kind == SEL_ARGMAX) io.rows = p.needs_row ? c->samp_rows_dev + 1 + nd : nullptr;          // (the tail's alone)
            else io.rows = p.needs_row ? c->samp_rows_dev + 1 + (r0 - n_plain) : nullptr;
            io.cons = p.needs_cons ? c->cons_rows_dev + 1 + (r0 - n_plain) : nullptr;
            io.scratch = c->samp_scratch; io.am_scratch = c->round_scratch; io.batch = &sb;
            const LogprobOut lpo{nullptr, 0, nullptr, 0, c->round_toks_dev + r0, 0, c->round_lp_rows_dev + r0};
            if (p.record) { io.lp = &lpo; io.lp_scratch = c->round_lp_scratch; io.rec0 = rb.rec0[kind] - r0; }
            return select_enqueue(c, p, io);
        };
        // the descriptors go to the device once, in front of the first block that reads any: the plain block only when it has a recording tail
        bool posted = false;
        auto post = [&]() -> int {
            if (posted) return MMD_OK;
            posted = true;
            if (nd + plain_tail > 0) HIPCHK(c, hipMemcpyAsync(c->samp_rows_dev + 1, c->samp_rows_host + 1, sizeof(SampleRow) * (nd + plain_tail), hipMemcpyHostToDevice, st));          // (the round's synchronisation frees the staging)
            if (n_greedy > n_plain || rb.any_cons_sampled) HIPCHK(c, hipMemcpyAsync(c->cons_rows_dev + 1, c->cons_rows_host + 1, sizeof(ConstraintRow) * nd, hipMemcpyHostToDevice, st));
            if (n_rec > 0) HIPCHK(c, hipMemcpyAsync(c->round_lp_rows_dev, c->round_lp_rows_host, sizeof(LogprobRow) * n_sample, hipMemcpyHostToDevice, st));
            return MMD_OK;
        };
        if (n_plain) {
            if (plain_tail > 0) { rc = post(); if (rc) return rc; }
            ProfScope ps(c, MMD_K_OTHER, 0, 0); HIPCHK(c, block(SEL_ARGMAX));
        }
        if (n_sample > n_plain) {
            rc = post(); if (rc) return rc;
            ProfScope ps(c, MMD_K_OTHER, 0, 0);
            if (n_greedy > n_plain) HIPCHK(c, block(SEL_CONS_ARGMAX));
            if (n_sample > n_greedy) HIPCHK(c, block(SEL_DRAW));
        }
        HIPCHK(c, hipMemcpyAsync(c->round_toks_host, c->round_toks_dev, sizeof(int64_t) * n_sample, hipMemcpyDeviceToHost, st));
    }
    if (n_head_rows) { rc = read_head_rows(c, head_rows, n_head_rows, compact); if (rc) return rc; }
    if (n_head_rows || n_sample) HIPCHK(c, hipStreamSynchronize(st));          // the round's ONE synchronisation: head logits and drawn tokens cross together
    if (n_head_rows) memcpy(heads_out_host, c->heads_host, sizeof(float) * 4 * n_head_rows);
    if (tokens_out_host) for (int j = 0; j < n_segs; ++j) tokens_out_host[j] = -1;
    for (int i = 0; i < n_sample; ++i) {
        const int64_t tok = c->round_toks_host[i];
        mmd_sampler* sp = samplers[sample_seg[i]];
        tokens_out_host[sample_seg[i]] = tok;
        if (i >= n_greedy) sp->offset += 1;
        if (tok < 0) FAIL(c, MMD_EDOM, "segment %d: a NaN among the logits, or every score is -inf: no token drawn", sample_seg[i]);
        Response& r = sp->resp;          // (the kernels have appended the token where the list had room: the count follows)
        response_note_token(r.count, response_is_eos(response_eos(r.cons, sp->eos, V), tok), r.penalty > 0.f, r.lp_top >= 0, r.prev_cap);
    }
    return MMD_OK;
}

extern "C" int mmd_video_heads(mmd_ctx* c, const void* hidden, int M, float* out) {
    NEED_FINAL(c);
    ProfScope ps(c, MMD_K_OTHER, 0, 0);
    HIPCHK(c, launch_heads(c->cfg.dtype, hidden, c->cfg.hidden_size, nullptr, M, c->heads4, c->cfg.hidden_size, out, c->stream));
    return MMD_OK;
}

extern "C" int mmd_lm_head(mmd_ctx* c, const void* hidden, int M, float* logits) {
    NEED_FINAL(c);
    const int H = c->cfg.hidden_size, V = c->cfg.vocab_size;
    return gemm(c, hidden, H, c->lm_head, H, nullptr, nullptr, 0, logits, V, M, V, H, EPI_NONE, 1, GEMM_AUTO, c->lm_head_p);
}

// ---- teacher-forced scoring: CrossEntropyLoss(reduction='none') of labels under lm_head(hidden), the [M, V] logits never held --------------------------------
// (models/live_llava/video_head_live_llava_qwen.py:155,164-170).  Row blocks of at most max_step_tokens rows; inside a row block the vocabulary goes through the
// fp32 workspace one chunk at a time: the unchanged GEMM writes logits [m, nc], the reduce folds them into the rows' (max, sum exp, label logit), and after the
// last chunk the finalize kernel writes nll (and lse).  A chunk of W is a row range of the row-major matrix, so `ldw` stays K and the planner sees an ordinary GEMM.
// The packed copy is fragment-major over the WHOLE matrix: it is handed to the planner only for a chunk that is the whole vocabulary (every M <= 64 call at auto width).
constexpr size_t LM_NLL_WS_MAX = (size_t)64 << 20;
static void lm_nll_release(mmd_ctx* c) {
    dev_free(c, c->nll_ws); dev_free(c, c->nll_state); dev_free(c, c->nll_part);
    c->nll_ws = c->nll_state = c->nll_part = nullptr; c->nll_ws_bytes = 0; c->nll_rows = 0;
}
// the three buffers exist together or not at all: nll_part is allocated last and is what the guard looks at; a failure half way frees and resets all of them
static int lm_nll_reserve(mmd_ctx* c, size_t ws_bytes, int rows) {
    if (c->nll_part && c->nll_ws_bytes >= ws_bytes && c->nll_rows >= rows) return MMD_OK;
    if (c->nll_part) { hipStreamSynchronize(c->stream); ws_bytes = ws_bytes > c->nll_ws_bytes ? ws_bytes : c->nll_ws_bytes; rows = rows > c->nll_rows ? rows : c->nll_rows; }
    lm_nll_release(c);
    int rc = dev_alloc(c, (void**)&c->nll_ws, ws_bytes, false);
    if (!rc) rc = dev_alloc(c, (void**)&c->nll_state, (size_t)rows * 3 * sizeof(float), false);
    if (!rc) rc = dev_alloc(c, (void**)&c->nll_part, (size_t)(rows > LM_NLL_BLOCKS ? rows : LM_NLL_BLOCKS) * 3 * sizeof(float), false);
    if (rc) { lm_nll_release(c); return rc; }
    c->nll_ws_bytes = ws_bytes; c->nll_rows = rows;
    return MMD_OK;
}
static int lm_nll_run(mmd_ctx* c, const void* X, const void* W, const void* Wp, int M, int V, int K, const int64_t* labels, int64_t ignore_index, int chunk_cols,
                      float* nll_out, float* lse_out) {
    if (V <= 0 || K <= 0 || chunk_cols < 0) FAIL(c, MMD_EINVAL, "lm_nll: V = %d, K = %d, chunk_cols = %d", V, K, chunk_cols);
    hipStream_t st = c->stream; const size_t e = es(c);
    int rows = c->cfg.max_step_tokens < 1 ? 1 : c->cfg.max_step_tokens;
    if (rows > 32768) rows = 32768;          // (a row is a grid row of the reduce; 256 columns of 32768 rows still fit the workspace)
    if (rows > M) rows = M;
    const int64_t vpad = round_up(V, 256);
    size_t ws_bytes = (size_t)rows * vpad * sizeof(float); if (ws_bytes > LM_NLL_WS_MAX) ws_bytes = LM_NLL_WS_MAX;
    int64_t forced = 0;
    if (chunk_cols > 0) {
        forced = round_up(chunk_cols, 8); if (forced > round_up(V, 8)) forced = round_up(V, 8);
        const int64_t fit = (int64_t)(ws_bytes / (forced * sizeof(float)));
        if (fit < 1) FAIL(c, MMD_EINVAL, "lm_nll: a chunk of %lld columns does not fit the %zu-byte workspace", (long long)forced, ws_bytes);
        if (rows > fit) rows = (int)fit;
    }
    int rc = lm_nll_reserve(c, ws_bytes, rows); if (rc) return rc;
    for (int r0 = 0; r0 < M; r0 += rows) {
        const int m = M - r0 < rows ? M - r0 : rows;
        // auto width: the largest multiple of 256 columns this row block's logits fit the workspace with, at most the vocabulary
        int64_t cw = forced ? forced : (int64_t)(ws_bytes / ((size_t)m * sizeof(float))) / 256 * 256;
        if (cw > V) cw = V;
        const int64_t ld = round_up(cw, 8);
        const void* x = (const char*)X + (size_t)r0 * K * e;
        for (int64_t n0 = 0; n0 < V; n0 += cw) {
            const int nc = (int)(V - n0 < cw ? V - n0 : cw);
            rc = gemm(c, x, K, (const char*)W + (size_t)n0 * K * e, K, nullptr, nullptr, 0, c->nll_ws, ld, m, nc, K, EPI_NONE, /*out_f32*/1, GEMM_AUTO, nc == V ? Wp : nullptr);
            if (rc) return rc;
            ProfScope ps(c, MMD_K_OTHER, (double)m * nc * sizeof(float), 0);
            HIPCHK(c, launch_lm_nll_chunk(c->nll_ws, ld, m, nc, n0, labels + r0, n0 == 0, c->nll_state, c->nll_part, st));
        }
        ProfScope ps(c, MMD_K_OTHER, (double)m * 5 * sizeof(float), 0);
        HIPCHK(c, launch_lm_nll_finalize(c->nll_state, labels + r0, ignore_index, m, nll_out + r0, lse_out ? lse_out + r0 : nullptr, st));
    }
    return MMD_OK;
}
extern "C" int mmd_lm_nll(mmd_ctx* c, const void* hidden, int M, const int64_t* labels, int64_t ignore_index, int chunk_cols, float* nll_out, float* lse_out) {
    if (!c || M < 0) return MMD_EINVAL;
    if (M == 0) return MMD_OK;
    if (!hidden || !labels || !nll_out) return MMD_EINVAL;
    NEED_FINAL(c);
    return lm_nll_run(c, hidden, c->lm_head, c->lm_head_p, M, c->cfg.vocab_size, c->cfg.hidden_size, labels, ignore_index, chunk_cols, nll_out, lse_out);
}

extern "C" int mmd_frame_step(mmd_ctx* c, mmd_stream* s, const void* embeds, int S, const int32_t* rows_host, int n_rows, float* out_host) {
    NEED_FINAL(c);
    if (n_rows < 0 || n_rows > S) FAIL(c, MMD_EINVAL, "bad head row count");
    for (int i = 0; i < n_rows; ++i) if (rows_host[i] < 0 || rows_host[i] >= S) FAIL(c, MMD_ERANGE, "head row %d outside the step", rows_host[i]);
    if (!s || s->ctx != c) FAIL(c, MMD_EINVAL, "stream does not belong to this context");
    StepSeg one{s, 0, S};
    int32_t need[STEP_NEED_MAX]; const int n_need = build_need_list(rows_host, n_rows, nullptr, 0, need);
    int rc = S > 0 ? llm_step_segs(c, &one, 1, embeds, S, nullptr, nullptr, n_need ? need : nullptr, n_need) : MMD_OK; if (rc) return rc;
    if (n_rows == 0) return MMD_OK;
    rc = read_head_rows(c, rows_host, n_rows, c->hid_compact > 0); if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out_host, c->heads_host, sizeof(float) * 4 * n_rows);
    return MMD_OK;
}

// what a generate call's selection launches over: the context's one-row buffers -- logits_ws, row / constraint descriptor 0, tok_dev; the plain arg-max takes the penalty list
// in kernel arguments (dyn: its length from *dyn)
static SelectIO generate_select_io(mmd_ctx* c, const SelectPlan& p, const StepState* dyn, const LogprobOut* lp) {
    const Response& r = c->resp; const bool pen = r.penalty > 0.f;
    SelectIO io{};
    io.logits = c->logits_ws; io.V = c->cfg.vocab_size; io.n = 1; io.rows = c->samp_rows_dev; io.cons = c->cons_rows_dev; io.lp = lp;
    io.toks = p.kind == SEL_DRAW ? nullptr : c->tok_dev;          // (the draw's row descriptor names tok_dev itself)
    io.scratch = c->samp_scratch; io.lp_scratch = c->lp_scratch; io.am_scratch = c->argmax_scratch;
    io.prev = r.prev_dev; io.n_prev = pen ? r.count.n_prev : 0; io.penalty = pen ? r.penalty : 1.f; io.dyn = dyn;
    return io;
}

// one decode step (feed the previously drawn token, choose the next as `sel` says) enqueued on the stream; `dyn` selects the graph-capturable form that reads position / arena /
// penalty-list length from device state.  `lp`: where the step records (the kernels stand between the choice of the token and the state's advance)
static int decode_step_enqueue(mmd_ctx* c, mmd_stream* s, const SelectPlan& sel, int64_t eos_id, const StepState* dyn, const LogprobOut* lp) {
    const mmd_config& g = c->cfg; hipStream_t st = c->stream; const int H = g.hidden_size;
    // the next token's embedding is gathered straight into the residual-stream buffer (llm_step_segs skips its copy when embeds == l_h)
    HIPCHK(c, launch_embed(g.dtype, c->embed, c->tok_dev, 1, H, g.vocab_size, c->l_h, st));
    int rc = llm_step_impl(c, s, c->l_h, 1, nullptr, dyn); if (rc) return rc;
    rc = gemm(c, c->l_hid, H, c->lm_head, H, nullptr, nullptr, 0, c->logits_ws, g.vocab_size, 1, g.vocab_size, H, EPI_NONE, 1, GEMM_AUTO, c->lm_head_p); if (rc) return rc;
    HIPCHK(c, select_enqueue(c, sel, generate_select_io(c, sel, dyn, lp)));
    if (sel.advance) HIPCHK(c, launch_advance_state(c->step_dev, c->tok_dev, c->resp.prev_dev, c->resp.prev_cap, eos_id, c->resp.penalty > 0.f ? 1 : 0, st, sel.needs_cons ? c->cons_rows_dev : nullptr));
    return MMD_OK;
}

// captures one dynamic decode step into dg for the key (key_pen, eos_id, the plan's key).  Capture runs on the context's own stream (the legacy null stream -- torch's default --
// cannot be captured); the instantiated graph is then launched on whatever stream the caller bound
static int capture_decode_step(mmd_ctx* c, mmd_stream* s, DecodeGraph& dg, const SelectPlan& sel, const GeneratePlan& gp, int64_t eos_id, float key_pen, const LogprobOut* lp) {
    hipStream_t st = c->stream;
    dg.drop();
    HIPCHK(c, hipStreamSynchronize(st));
    c->stream = c->own_stream;
    hipError_t be = hipStreamBeginCapture(c->own_stream, hipStreamCaptureModeThreadLocal);
    if (be != hipSuccess) { c->stream = st; HIPCHK(c, be); }
    int rc = decode_step_enqueue(c, s, sel, eos_id, c->step_dev, lp);
    hipError_t ce = hipStreamEndCapture(c->own_stream, &dg.src);
    c->stream = st;
    if (rc) { dg.drop(); return rc; }
    HIPCHK(c, ce);
    HIPCHK(c, hipGraphInstantiate(&dg.exec, dg.src, nullptr, nullptr, 0));
    dg.pen = key_pen; dg.eos = eos_id; dg.sel = gp.key_sel; dg.lp = gp.key_lp; dg.cons = gp.key_cons_gen;
    return MMD_OK;
}

// The reference penalises EVERY id generated so far in the video (models/modeling_live.py:60-66; the list persists across turns): the device copy grows with it.  No cap.
// Both captured decode steps hold the list's and the records' pointers: when either buffer moves they are dropped.
static void generate_buffer_moved(mmd_ctx* c, bool moved) { if (moved) { c->dec_greedy.drop(); c->dec_sampled.drop(); } }

// ---- the token loop of a response: prompt step, then one token in, one token out --------------------------------------------------------------------------
// samp == nullptr: arg-max (+ repetition penalty).  Otherwise the sampling chain of sample.hip stands where the arg-max stood.  Which launches choose a token is
// select_plan()'s answer, what surrounds them -- captured or eager steps, which descriptor is posted when, who grows the penalty list -- generate_plan()'s (select_plan.h);
// this function follows the two.  Everything the chain needs per step is in row descriptor 0 on the device: the penalty-list length is read through &step_dev->n_prev and
// grown by advance_state_kernel, the Philox offset is advanced by the draw kernel, so the captured step is replayed as it is for any temperature / top_k / top_p / seed.
// Draw i of the call uses offset *offset_inout + i; *offset_inout advances with every token read (EOS included).  *n_out is up to date whenever the call returns.
// Log-probabilities (mmd_set_generate_logprobs): every step, the prompt's included, records behind its choice into lp_rec[step]; the captured step reads its index from
// step_dev->step.  Nothing is read back here: mmd_generate_logprobs_read copies the records once.
static int generate_impl(mmd_ctx* c, mmd_stream* s, const void* prompt_embeds, int S, int64_t eos_id, float rep_penalty, int64_t* prev_ids_host, int* n_prev, int prev_cap,
                         int64_t* out_ids_host, int max_new, int* n_out, const SampleArgs* samp) {
    c->dec_route = 0; *n_out = 0;
    Response& rs = c->resp; ResponseCount& cnt = rs.count;
    const int lp_top = rs.lp_top; const bool lp_on = lp_top >= 0;
    cnt = ResponseCount{}; cnt.max_new = max_new; c->lp_call_top = lp_top;
    if (max_new == 0) return MMD_OK;          // nothing asked for: nothing is enqueued, the stream is not extended
    if (!s || s->ctx != c) FAIL(c, MMD_EINVAL, "stream does not belong to this context");
    if (S < 1) FAIL(c, MMD_EINVAL, "empty prompt");
    int rc;
    if (samp) { rc = check_sampling(c, samp->temperature, samp->top_k, samp->top_p); if (rc) return rc; }
    const mmd_config& g = c->cfg; hipStream_t st = c->stream; const int H = g.hidden_size, V = g.vocab_size; const size_t e = es(c);
    const bool cons_on = rs.cons.on;
    const SelectPlan sel0 = select_plan(select_rows(samp != nullptr, cons_on, lp_on, 1, true, false, V, samp));          // the prompt step's choice
    rc = select_refused(c, sel0); if (rc) return rc;
    const bool pen = rep_penalty > 0.f;
    rs.penalty = pen ? rep_penalty : 0.f;
    const int np0 = (pen && n_prev) ? *n_prev : 0;          // cnt.n_prev from here on: the list's length, grown by response_note_token
    bool moved = false;
    if (pen) { rc = response_reserve_list(c, rs, generate_prev_need(np0, max_new), MODEL_PREV_CAP, &moved); generate_buffer_moved(c, moved); if (rc) return rc; }
    if (sel0.needs_row) { rc = sample_reserve(c); if (rc) return rc; }
    // constraints on: descriptor 0 on the device carries the response's EOS ids (response_eos: the call's own eos_id when the set has none), min_new and the table; the captured
    // step reads the response step through &step_dev->step, an eager arg-max step gets it posted.  The host stops on the same ids.
    const ResponseEos eos = response_eos(rs.cons, eos_id, V);
    ConstraintRow crow{};
    if (cons_on) cons_fill_row(crow, rs, eos);
    auto post_cons = [&](bool dynamic, int step) -> int {
        crow.step = step; crow.step_ptr = dynamic ? &c->step_dev->step : nullptr;
        c->cons_rows_host[0] = crow;
        HIPCHK(c, hipMemcpyAsync(c->cons_rows_dev, c->cons_rows_host, sizeof(ConstraintRow), hipMemcpyHostToDevice, st));
        return MMD_OK;
    };
    if (lp_on && !c->lp_scratch) { rc = dev_alloc(c, &c->lp_scratch, logprob_scratch_bytes(1), false); if (rc) return rc; }
    if (lp_on) { rc = response_reserve_records(c, rs, max_new, RESPONSE_CTX_RECORDS_FIRST, &moved); generate_buffer_moved(c, moved); if (rc) return rc; }
    if (np0 > 0) HIPCHK(c, hipMemcpyAsync(rs.prev_dev, prev_ids_host, sizeof(int64_t) * np0, hipMemcpyHostToDevice, st));
    cnt.n_prev = np0;
    uint64_t no_offset = 0;
    // row descriptor 0: the draw's row, or -- behind an arg-max -- the row of the scores that the constraints and the records read: the penalty at T = 1, no filter, no draw.
    // (Every earlier upload from this staging slot has been waited for: a token read lies in between.)
    auto post_row = [&](bool dynamic) -> int {
        const SampleArgs plain{1.f, 0, 1.f, 0, &no_offset};
        fill_sample_row(c->samp_rows_host[0], samp ? *samp : plain, rs, dynamic ? &c->step_dev->n_prev : nullptr, samp ? c->tok_dev : nullptr, nullptr, samp ? c->sample_lane : 0, samp ? 1 : 0);
        HIPCHK(c, hipMemcpyAsync(c->samp_rows_dev, c->samp_rows_host, sizeof(SampleRow), hipMemcpyHostToDevice, st));
        return MMD_OK;
    };
    LogprobOut lpo{rs.lp_rec, rs.lp_cap, nullptr, 0, c->tok_dev, lp_top};
    // a token read: returned and counted; unless it is EOS it joins the penalty list -- on the device by a copy here (`copy`) or by advance_state_kernel, in the caller's list here
    auto take_token = [&](int64_t tok, bool copy) -> int {
        out_ids_host[cnt.step] = tok; *n_out = cnt.step + 1;
        if (!response_note_token(cnt, response_is_eos(eos, tok), pen, lp_on, rs.prev_cap)) return MMD_OK;
        const int at = cnt.n_prev - 1;
        if (copy) HIPCHK(c, hipMemcpyAsync(rs.prev_dev + at, c->tok_dev, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        if (prev_ids_host && at < prev_cap) prev_ids_host[at] = tok;
        return MMD_OK;
    };
    auto read_token = [&](int64_t* tok) -> int {
        HIPCHK(c, hipMemcpyAsync(c->tok_host, c->tok_dev, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        *tok = c->tok_host[0];
        if (samp) ++*samp->offset_inout;
        // every route: the plain arg-max answers -1 for a row with a NaN too (argmax_final_kernel)
        if (*tok < 0) FAIL(c, MMD_EDOM, cons_on ? "NaN in the logits, or every score is -inf under the constraints: no token drawn" : "NaN in the logits: no token drawn");
        return MMD_OK;
    };
    // step 0: the prompt (eager)
    rc = llm_step_impl(c, s, prompt_embeds, S, nullptr, nullptr); if (rc) return rc;
    {
        const void* last = (const char*)c->l_hid + (size_t)(S - 1) * H * e;
        rc = gemm(c, last, H, c->lm_head, H, nullptr, nullptr, 0, c->logits_ws, V, 1, V, H, EPI_NONE, 1, GEMM_AUTO, c->lm_head_p); if (rc) return rc;
        if (sel0.needs_row) { rc = post_row(false); if (rc) return rc; }
        if (sel0.needs_cons) { rc = post_cons(false, 0); if (rc) return rc; }
        ProfScope ps(c, MMD_K_OTHER, 0, 0);
        HIPCHK(c, select_enqueue(c, sel0, generate_select_io(c, sel0, nullptr, &lpo)));
    }
    int64_t tok = 0;
    rc = read_token(&tok); if (rc) return rc;
    rc = take_token(tok, true); if (rc) return rc;
    const bool stop = response_is_eos(eos, tok);
    // steps 1..: one token in, one token out
    GenerateShape shape;
    shape.sampled = samp != nullptr; shape.constrained = cons_on; shape.record = lp_on; shape.pen = pen; shape.max_new = max_new; shape.first_is_eos = stop;
    shape.V = V; if (samp) { shape.top_k = samp->top_k; shape.top_p = samp->top_p; }
    shape.lp_top = lp_top; shape.cons_gen = c->cons_gen;
    shape.gate.no_graph = c->no_graph; shape.gate.no_fuse = c->sw.no_fuse; shape.gate.prof_on = c->prof.on != 0; shape.gate.dtype = g.dtype; shape.gate.qkv_p = c->L[0].wqkv_p != nullptr;
    shape.gate.H = g.hidden_size; shape.gate.d = g.head_dim;
    const GeneratePlan gp = generate_plan(shape);
    const SelectPlan sel = select_plan(select_rows(samp != nullptr, cons_on, lp_on, 1, true, gp.can_graph, V, samp));          // the steps' choice
    c->select_last[SELECT_PLAN_FIELDS] = SELECT_OF_GENERATE; gp.fields(c->select_last + SELECT_PLAN_FIELDS + 1);
    if (gp.can_graph) { rc = kv_reserve(c, s, s->len + max_new + 1); if (rc) return rc; }
    if (gp.upload_state) {
        StepState* hs = c->step_host;
        hs->n_ctx = s->len; hs->cap = s->cap; hs->K = s->K; hs->V = s->V; hs->n_prev = cnt.n_prev; hs->step = 1; hs->pos_off = s->pos_off;
        HIPCHK(c, hipMemcpyAsync(c->step_dev, hs, sizeof(StepState), hipMemcpyHostToDevice, st));
    }
    if (gp.post_row_dynamic) { rc = post_row(true); if (rc) return rc; }
    if (gp.post_cons_dynamic) { rc = post_cons(true, 1); if (rc) return rc; }
    if (gp.can_graph) lpo.dyn = c->step_dev;
    DecodeGraph& dg = samp ? c->dec_sampled : c->dec_greedy;
    if (gp.can_graph) {
        const float key_pen = pen ? (gp.pen_key_is_value ? rep_penalty : 1.f) : 0.f;
        c->dec_route = 1;
        if (!dg.exec || dg.pen != key_pen || dg.eos != eos_id || dg.sel != gp.key_sel || dg.lp != gp.key_lp || dg.cons != gp.key_cons_gen) {
            rc = capture_decode_step(c, s, dg, sel, gp, eos_id, key_pen, &lpo); if (rc) { c->dec_route = 0; return rc; }
            c->dec_route = 2;
        }
        sel.fields(c->select_last);          // the plan the replayed step was captured from
    }
    for (int i = 1; i < max_new && !stop; ++i) {
        if (gp.can_graph) { HIPCHK(c, hipGraphLaunch(dg.exec, st)); s->len += 1; }
        else {
            if (gp.post_row_each_eager_step) { rc = post_row(false); if (rc) return rc; }
            if (gp.post_cons_each_eager_step) { rc = post_cons(false, i); if (rc) return rc; }
            lpo.idx0 = i;
            rc = decode_step_enqueue(c, s, sel, eos_id, nullptr, &lpo); if (rc) return rc;
        }
        rc = read_token(&tok); if (rc) return rc;
        rc = take_token(tok, gp.host_appends_penalty); if (rc) return rc;
        if (response_is_eos(eos, tok)) break;
    }
    if (pen && n_prev) *n_prev = cnt.n_prev;
    return MMD_OK;
}

extern "C" int mmd_greedy_generate(mmd_ctx* c, mmd_stream* s, const void* prompt_embeds, int S, int64_t eos_id, float rep_penalty,
                                   int64_t* prev_ids_host, int* n_prev, int prev_cap, int64_t* out_ids_host, int max_new, int* n_out) {
    NEED_FINAL(c);
    if (!n_out || !out_ids_host || max_new <= 0) FAIL(c, MMD_EINVAL, "bad generate arguments");
    return generate_impl(c, s, prompt_embeds, S, eos_id, rep_penalty, prev_ids_host, n_prev, prev_cap, out_ids_host, max_new, n_out, nullptr);
}

extern "C" int mmd_set_sample_lane(mmd_ctx* c, int lane) { if (!c || lane < 0) return MMD_EINVAL; c->sample_lane = (uint32_t)lane; return MMD_OK; }

extern "C" int mmd_sample_generate(mmd_ctx* c, mmd_stream* s, const void* prompt_embeds, int S, int64_t eos_id, float rep_penalty, int64_t* prev_ids_host, int* n_prev, int prev_cap,
                                   float temperature, int top_k, float top_p, uint64_t seed, uint64_t* offset_inout, int64_t* out_ids_host, int max_new, int* n_out) {
    NEED_FINAL(c);
    if (!n_out || max_new < 0 || (max_new > 0 && !out_ids_host) || !offset_inout) FAIL(c, MMD_EINVAL, "bad generate arguments");
    const SampleArgs samp{temperature, top_k, top_p, seed, offset_inout};
    return generate_impl(c, s, prompt_embeds, S, eos_id, rep_penalty, prev_ids_host, n_prev, prev_cap, out_ids_host, max_new, n_out, &samp);
}

extern "C" int mmd_set_generate_constraints(mmd_ctx* c, const int64_t* eos_ids_host, int n_eos, int min_new, const int32_t* ids_host, const float* bias_host, int n) {
    NEED_FINAL(c);
    ConsSet s; int rc = cons_checked(c, c->cfg.vocab_size, eos_ids_host, n_eos, min_new, ids_host, bias_host, n, s); if (rc) return rc;
    if (s.on) { rc = cons_reserve(c); if (rc) return rc; }
    rc = response_set_constraints(c, c->resp, s); if (rc) return rc;
    c->cons_gen = s.on ? 1 : 0;          // on <-> off: another captured step.  Everything else about a set -- EOS ids, min_new, the table -- is read from descriptor 0 on the device
    return MMD_OK;
}

extern "C" int mmd_set_generate_logprobs(mmd_ctx* c, int top_n) {
    if (!c) return MMD_EINVAL;
    const int rc = response_lp_top_checked(c, top_n); if (rc) return rc;
    c->resp.lp_top = top_n;          // (the next call's; the last call's records stay readable under lp_call_top)
    return MMD_OK;
}

extern "C" int mmd_generate_logprobs_read(mmd_ctx* c, float* logprob_host, float* sampling_logprob_host, int64_t* top_ids_host, float* top_logprob_host, int cap_tokens, int* n_out) {
    if (!c) return MMD_EINVAL;
    hipSetDevice(c->device);
    if (!n_out || cap_tokens < 0) FAIL(c, MMD_EINVAL, "bad mmd_generate_logprobs_read arguments");
    *n_out = 0;
    const int n = c->resp.count.lp_n;
    if (n == 0) return MMD_OK;
    const int rc = response_read_records(c, c->resp, n, c->lp_call_top, logprob_host, sampling_logprob_host, top_ids_host, top_logprob_host, cap_tokens); if (rc) return rc;
    *n_out = n;
    return MMD_OK;
}

// raw operator: n rows of logits through the selection, one set of parameters, row i on lane i (MMD_ROUND_MAX_SAMPLERS rows per launch).  lp_host != null: the rows'
// log-probability records too.  oc != null: one constraint set per row.  greedy: the arg-max stands in the draw's place -- the multi-row arg-max with penalty, under
// constraints the first maximal index of the unfiltered scores (select_plan decides).  fail_no_token: a row without a token (-1) fails the call with MMD_EDOM.
struct OpConstraints { const ConsSet* sets; const int32_t* tab_off; const int32_t* step; };          // row i's table: entries [tab_off[i], tab_off[i + 1]) of the tables back to back
// the argument checks the three entries share (`who` names the entry in the message); greedy: the chain's parameters are those of the unfiltered scores
static int op_select_check(mmd_ctx* c, const char* who, const float* logits, const int64_t* tokens_out, const float* info_out, bool greedy, int n, int V, int n_prev,
                           const int64_t* prev_ids_dev, float& temperature, int& top_k, float& top_p) {
    if (greedy) { temperature = 1.f; top_k = 0; top_p = 1.f; }
    if (!logits || !tokens_out || (!info_out && !greedy) || n < 1 || n > 4096 || V < 1 || V > SELECT_MAX_V || n_prev < 0 || (n_prev > 0 && !prev_ids_dev)) FAIL(c, MMD_EINVAL, "bad %s arguments", who);
    if (!(temperature > 0.f) || top_k < 0 || !(top_p > 0.f && top_p <= 1.f)) FAIL(c, MMD_EINVAL, "sampling needs temperature > 0, top_k >= 0, 0 < top_p <= 1");
    return MMD_OK;
}
static int op_select_impl(mmd_ctx* c, const float* logits, int n, int V, const int64_t* prev_ids_dev, int n_prev, float rep_penalty, float temperature, int top_k, float top_p,
                          uint64_t seed, uint64_t offset, const uint64_t* r_host, int64_t* tokens_out, float* info_out, float* scores_out,
                          bool greedy, int top_n, float* lp_host, int64_t* top_ids_host, float* top_lp_host, const OpConstraints* oc, bool fail_no_token) {
    hipStream_t st = c->stream;
    const int chunk = n < MMD_ROUND_MAX_SAMPLERS ? n : MMD_ROUND_MAX_SAMPLERS, total = oc ? oc->tab_off[n] : 0;
    const SampleArgs a{temperature, top_k, top_p, seed, &offset};
    const bool pen_on = rep_penalty > 0.f && n_prev > 0;
    const SelectPlan plan = select_plan(select_rows(!greedy, oc != nullptr, lp_host != nullptr, chunk, false, false, V, &a));          // of every chunk
    SampleRow* rows_dev = nullptr; ConstraintRow* cons_dev = nullptr; int32_t* ids_dev = nullptr; float* bias_dev = nullptr; unsigned long long* r_dev = nullptr; void* scratch = nullptr;
    LogprobRec* rec_dev = nullptr; void* lp_scratch = nullptr; void* am_scratch = nullptr;
    auto release = [&]() {
        hipStreamSynchronize(st);
        if (rows_dev) hipFree(rows_dev); if (cons_dev) hipFree(cons_dev); if (ids_dev) hipFree(ids_dev); if (bias_dev) hipFree(bias_dev); if (r_dev) hipFree(r_dev);
        if (scratch) hipFree(scratch); if (rec_dev) hipFree(rec_dev); if (lp_scratch) hipFree(lp_scratch); if (am_scratch) hipFree(am_scratch);
    };
#define OPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { release(); FAIL(c, MMD_EHIP, "%s failed: %s", #expr, hipGetErrorString(_e)); } } while (0)
    std::vector<SampleRow> rows((size_t)n); std::vector<ConstraintRow> crows(oc ? (size_t)n : 0); std::vector<int32_t> ids((size_t)(total > 0 ? total : 1)); std::vector<float> bias(ids.size());
    OPCHK(hipMalloc((void**)&rows_dev, sizeof(SampleRow) * n));
    OPCHK(hipMalloc(&scratch, sample_topkp_scratch_bytes(V, chunk, scores_out == nullptr)));
    if (oc) {
        OPCHK(hipMalloc((void**)&cons_dev, sizeof(ConstraintRow) * n));
        OPCHK(hipMalloc((void**)&ids_dev, sizeof(int32_t) * ids.size()));
        OPCHK(hipMalloc((void**)&bias_dev, sizeof(float) * bias.size()));
    }
    for (int i = 0; i < n; ++i) {
        fill_sample_row(rows[i], a, prev_ids_dev, pen_on, n_prev, n_prev, rep_penalty, nullptr, nullptr, nullptr, (uint32_t)i, 0);
        if (!oc) continue;
        const int o = oc->tab_off[i];
        for (int k = 0; k < oc->sets[i].n; ++k) { ids[o + k] = oc->sets[i].ids[k]; bias[o + k] = oc->sets[i].bias[k]; }          // (sorted by constraint_set)
        cons_fill_row(crows[i], oc->sets[i], ids_dev + o, bias_dev + o, response_eos(oc->sets[i], -1, V), oc->step[i], nullptr);
    }
    // (synchronous copies: the vectors above are pageable)
    OPCHK(hipMemcpy(rows_dev, rows.data(), sizeof(SampleRow) * n, hipMemcpyHostToDevice));
    if (oc) {
        OPCHK(hipMemcpy(cons_dev, crows.data(), sizeof(ConstraintRow) * n, hipMemcpyHostToDevice));
        OPCHK(hipMemcpy(ids_dev, ids.data(), sizeof(int32_t) * ids.size(), hipMemcpyHostToDevice));
        OPCHK(hipMemcpy(bias_dev, bias.data(), sizeof(float) * bias.size(), hipMemcpyHostToDevice));
    }
    if (r_host) { OPCHK(hipMalloc((void**)&r_dev, sizeof(uint64_t) * n)); OPCHK(hipMemcpy(r_dev, r_host, sizeof(uint64_t) * n, hipMemcpyHostToDevice)); }
    if (plan.record) { OPCHK(hipMalloc((void**)&rec_dev, sizeof(LogprobRec) * n)); OPCHK(hipMalloc(&lp_scratch, logprob_scratch_bytes(chunk))); }
    if (plan.kind == SEL_ARGMAX) OPCHK(hipMalloc(&am_scratch, sample_batch_scratch_bytes()));
    c->select_last[SELECT_PLAN_FIELDS] = SELECT_OF_OP;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = n - i0 < chunk ? n - i0 : chunk;
        ProfScope ps(c, MMD_K_OTHER, 0, 0);
        const LogprobOut lpo{rec_dev, n, nullptr, i0, tokens_out + i0, top_n};
        SampleBatch b{};
        for (int r = 0; r < m; ++r) { b.prev[r] = prev_ids_dev; b.tok[r] = tokens_out + i0 + r; b.append[r] = nullptr; b.n_prev[r] = pen_on ? n_prev : 0; b.penalty[r] = pen_on ? rep_penalty : 1.f; }
        SelectIO io{};
        io.logits = logits + (size_t)i0 * V; io.V = V; io.n = m; io.rows = rows_dev + i0; io.cons = oc ? cons_dev + i0 : nullptr; io.lp = &lpo; io.toks = tokens_out + i0;
        io.scratch = scratch; io.lp_scratch = lp_scratch; io.am_scratch = am_scratch; io.batch = &b;
        io.r_words = r_dev ? r_dev + i0 : nullptr; io.info = info_out ? info_out + (size_t)i0 * 4 : nullptr; io.scores = scores_out ? scores_out + (size_t)i0 * V : nullptr;
        OPCHK(select_enqueue(c, plan, io));
    }
    OPCHK(hipStreamSynchronize(st));
    std::vector<int64_t> toks(fail_no_token ? (size_t)n : 0);
    if (fail_no_token) OPCHK(hipMemcpy(toks.data(), tokens_out, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    if (plan.record) {
        std::vector<LogprobRec> h((size_t)n);
        OPCHK(hipMemcpy(h.data(), rec_dev, sizeof(LogprobRec) * n, hipMemcpyDeviceToHost));
        std::vector<float> l1((size_t)n), l2((size_t)n);
        unpack_logprobs(h.data(), n, top_n, l1.data(), l2.data(), top_ids_host, top_lp_host);
        for (int i = 0; i < n; ++i) { lp_host[2 * i] = l1[i]; lp_host[2 * i + 1] = l2[i]; }
    }
#undef OPCHK
    release();
    for (size_t i = 0; i < toks.size(); ++i) if (toks[i] < 0) FAIL(c, MMD_EDOM, "row %d: a NaN among the logits, or every score is -inf under the constraints: no token drawn", (int)i);
    return MMD_OK;
}

extern "C" int mmd_op_sample(mmd_ctx* c, const float* logits, int n, int V, const int64_t* prev_ids_dev, int n_prev, float rep_penalty, float temperature, int top_k, float top_p,
                             uint64_t seed, uint64_t offset, const uint64_t* r_host, int64_t* tokens_out, float* info_out, float* scores_out) {
    if (!c) return MMD_EINVAL;
    hipSetDevice(c->device);
    int rc = op_select_check(c, "mmd_op_sample", logits, tokens_out, info_out, false, n, V, n_prev, prev_ids_dev, temperature, top_k, top_p); if (rc) return rc;
    return op_select_impl(c, logits, n, V, prev_ids_dev, n_prev, rep_penalty, temperature, top_k, top_p, seed, offset, r_host, tokens_out, info_out, scores_out, false, 0, nullptr, nullptr, nullptr,
                          nullptr, false);
}

extern "C" int mmd_op_sample_logprobs(mmd_ctx* c, const float* logits, int n, int V, const int64_t* prev_ids_dev, int n_prev, float rep_penalty, float temperature, int top_k, float top_p,
                                      uint64_t seed, uint64_t offset, const uint64_t* r_host, int greedy, int top_n, int64_t* tokens_out, float* info_out, float* scores_out,
                                      float* lp_out_host, int64_t* top_ids_out_host, float* top_lp_out_host) {
    if (!c) return MMD_EINVAL;
    if (top_n < 0 || top_n > LP_MAX_TOP) FAIL(c, MMD_ERANGE, "top_n 0..%d, got %d", LP_MAX_TOP, top_n);
    if (!lp_out_host || (top_n > 0 && (!top_ids_out_host || !top_lp_out_host))) FAIL(c, MMD_EINVAL, "bad mmd_op_sample_logprobs arguments");
    hipSetDevice(c->device);
    int rc = op_select_check(c, "mmd_op_sample", logits, tokens_out, info_out, greedy != 0, n, V, n_prev, prev_ids_dev, temperature, top_k, top_p); if (rc) return rc;
    // (greedy without constraints: the multi-row arg-max with penalty, then the unfiltered scores for the record -- SEL_ARGMAX over a block, not the constrained route)
    return op_select_impl(c, logits, n, V, prev_ids_dev, n_prev, rep_penalty, temperature, top_k, top_p, seed, offset, r_host, tokens_out, info_out, scores_out, greedy != 0, top_n,
                          lp_out_host, top_ids_out_host, top_lp_out_host, nullptr, false);
}

// raw operator of the constrained chain: mmd_op_sample_logprobs with one constraint set per row.  Row i's table is entries [tab_off[i], tab_off[i + 1]) of tab_ids / tab_bias;
// every set goes through constraint_set (the limits of mmd_set_generate_constraints).  Unlike the two entries above, a row without a token fails the call.
extern "C" int mmd_op_sample_constrained(mmd_ctx* c, const float* logits, int n, int V, const int64_t* prev_ids_dev, int n_prev, float rep_penalty, float temperature, int top_k, float top_p,
                                         uint64_t seed, uint64_t offset, const uint64_t* r_host, int greedy, int top_n,
                                         const int32_t* tab_off_host, const int32_t* tab_ids_host, const float* tab_bias_host, const int64_t* eos_host, const int32_t* n_eos_host,
                                         const int32_t* min_new_host, const int32_t* step_host,
                                         int64_t* tokens_out, float* info_out, float* scores_out, float* lp_out_host, int64_t* top_ids_out_host, float* top_lp_out_host) {
    if (!c) return MMD_EINVAL;
    hipSetDevice(c->device);
    if (!tab_off_host || !n_eos_host || !min_new_host || !step_host) FAIL(c, MMD_EINVAL, "bad mmd_op_sample_constrained arguments");
    int rc = op_select_check(c, "mmd_op_sample_constrained", logits, tokens_out, info_out, greedy != 0, n, V, n_prev, prev_ids_dev, temperature, top_k, top_p); if (rc) return rc;
    if (lp_out_host && (top_n < 0 || top_n > LP_MAX_TOP)) FAIL(c, MMD_ERANGE, "top_n 0..%d, got %d", LP_MAX_TOP, top_n);
    if (lp_out_host && top_n > 0 && (!top_ids_out_host || !top_lp_out_host)) FAIL(c, MMD_EINVAL, "bad mmd_op_sample_constrained arguments");
    if (tab_off_host[0] != 0) FAIL(c, MMD_EINVAL, "table offsets start at 0");
    std::vector<ConsSet> sets((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int o = tab_off_host[i], m = tab_off_host[i + 1] - o;
        if (m < 0 || step_host[i] < 0) FAIL(c, MMD_EINVAL, "row %d: bad table offsets or step", i);
        rc = cons_checked(c, V, eos_host ? eos_host + (size_t)i * CONS_MAX_EOS : nullptr, n_eos_host[i], min_new_host[i], tab_ids_host ? tab_ids_host + o : nullptr,
                          tab_bias_host ? tab_bias_host + o : nullptr, m, sets[i]);
        if (rc) return rc;
    }
    const OpConstraints oc{sets.data(), tab_off_host, step_host};
    return op_select_impl(c, logits, n, V, prev_ids_dev, n_prev, rep_penalty, temperature, top_k, top_p, seed, offset, r_host, tokens_out, info_out, scores_out, greedy != 0, top_n,
                          lp_out_host, top_ids_out_host, top_lp_out_host, &oc, true);
}

// ---- measurement -------------------------------------------------------------------------------------------------------
extern "C" int mmd_prof_enable(mmd_ctx* c, int mask) { if (!c) return MMD_EINVAL; if (!mask) prof_drain(c); c->prof.on = (unsigned)mask; return MMD_OK; }
extern "C" int mmd_prof_set_stride(mmd_ctx* c, int stride) { if (!c || stride < 1) return MMD_EINVAL; c->prof.stride = stride; return MMD_OK; }
extern "C" int mmd_prof_reset(mmd_ctx* c) {
    if (!c) return MMD_EINVAL;
    prof_drain(c);
    for (int i = 0; i < MMD_K_COUNT; ++i) { c->prof.ms[i] = 0; c->prof.n[i] = 0; c->prof.bytes[i] = 0; c->prof.flops[i] = 0; c->prof.seen[i] = 0; }
    return MMD_OK;
}
extern "C" int mmd_prof_read(mmd_ctx* c, double* ms, int64_t* n, double* bytes, double* flops) {
    if (!c) return MMD_EINVAL;
    prof_drain(c);
    for (int i = 0; i < MMD_K_COUNT; ++i) { if (ms) ms[i] = c->prof.ms[i]; if (n) n[i] = c->prof.n[i]; if (bytes) bytes[i] = c->prof.bytes[i]; if (flops) flops[i] = c->prof.flops[i]; }
    return MMD_OK;
}

// ---- raw operator entry points (parity tests) ---------------------------------------------------------------------------
extern "C" int mmd_op_gemm(mmd_ctx* c, const void* X, const void* W, const void* bias, const void* R, void* Y, int M, int N, int K, int epi,
                           int out_f32, int variant) {
    if (!c) return MMD_EINVAL;
    hipSetDevice(c->device);
    if (!c->splitk_ws) { c->splitk_bytes = model_splitk_bytes(c->cfg); int rc = dev_alloc(c, (void**)&c->splitk_ws, c->splitk_bytes); if (rc) return rc; }
    int NO = epi == EPI_SWIGLU ? N / 2 : N;
    void* Wp = nullptr;
    // the model holds every matrix in both layouts (or packed only): give the dispatcher the same choice, variant 0 included
    if (variant == GEMM_AUTO || variant == GEMM_SKINNY || variant == GEMM_BIG || variant == GEMM_RING256 || variant == GEMM_RING256_SPLIT || variant == GEMM_STREAM || variant >= GEMM_RINGX) { int rc = make_packed(c, W, N, K, &Wp); if (rc) return rc; }
    int rc = gemm(c, X, K, W, K, bias, R, NO, Y, NO, M, N, K, epi, out_f32, variant, Wp);
    if (Wp) { hipStreamSynchronize(c->stream); dev_free(c, Wp); }
    return rc;
}
// mmd_lm_nll's path over an explicit W [V,K] / X [M,K] (the packed copy is made only where the path uses it: bf16, the whole vocabulary in one chunk)
extern "C" int mmd_op_lm_nll(mmd_ctx* c, const void* X, const void* W, int M, int V, int K, const int64_t* labels, int64_t ignore_index, int chunk_cols,
                             float* nll_out, float* lse_out) {
    if (!c || M < 0) return MMD_EINVAL;
    if (M == 0) return MMD_OK;
    if (!X || !W || !labels || !nll_out) return MMD_EINVAL;
    hipSetDevice(c->device);
    if (!c->splitk_ws) { c->splitk_bytes = model_splitk_bytes(c->cfg); int rc = dev_alloc(c, (void**)&c->splitk_ws, c->splitk_bytes); if (rc) return rc; }
    void* Wp = nullptr;
    if (M <= 64 && (chunk_cols == 0 || chunk_cols >= V)) { int rc = make_packed(c, W, V, K, &Wp); if (rc) return rc; }
    int rc = lm_nll_run(c, X, W, Wp, M, V, K, labels, ignore_index, chunk_cols, nll_out, lse_out);
    if (Wp) { hipStreamSynchronize(c->stream); dev_free(c, Wp); }
    return rc;
}
// the weight-streaming kernels in slab mode (what the fused LLM schedule launches): X [M,K] . W [N,K]^T as `*splits_out` fp32 partial slabs [splits][M][N] in
// slabs_out (device, room for max_splits); variant GEMM_SKINNY (auto by M: gemv16 / skinny / stream) or GEMM_STREAM
extern "C" int mmd_op_gemm_slabs(mmd_ctx* c, const void* X, const void* W, int M, int N, int K, int variant, float* slabs_out, int max_splits, int* splits_out) {
    if (!c || !X || !W || !slabs_out || !splits_out || max_splits < 1) return MMD_EINVAL;
    if (M <= 0 || N <= 0 || K <= 0 || M > 256 || (N % 16) != 0 || (K % 32) != 0 || (variant != GEMM_SKINNY && variant != GEMM_STREAM)) FAIL(c, MMD_EINVAL, "gemm_slabs: 1 <= M <= 256, N %% 16 == 0, K %% 32 == 0, variant 2 or 8");
    hipSetDevice(c->device);
    void* Wp = nullptr;
    int rc = make_packed(c, W, N, K, &Wp); if (rc) return rc;
    GemmArgs g; memset(&g, 0, sizeof(g));
    int splits = 0;
    g.X = X; g.ldx = K; g.Wp = Wp; g.M = M; g.N = N; g.K = K; g.epi = EPI_NONE; g.variant = variant;
    g.splitk_ws = slabs_out; g.splitk_ws_bytes = (size_t)max_splits * M * N * sizeof(float); g.slabs_out = &splits; g.plan_out = c->last_plan;
    if (!Wp || !gemm_can_slab(c->cfg.dtype, g)) { if (Wp) dev_free(c, Wp); FAIL(c, MMD_EINVAL, "gemm_slabs: no slab kernel takes M = %d, N = %d, K = %d in this context's dtype", M, N, K); }          // (a shape no slab kernel accepts would fall through to a tile kernel with Y == nullptr)
    hipError_t e = launch_gemm(c->cfg.dtype, g, c->stream);
    hipStreamSynchronize(c->stream);
    dev_free(c, Wp);
    if (e != hipSuccess) FAIL(c, MMD_EHIP, "slab GEMM launch failed: %s", hipGetErrorString(e));
    *splits_out = splits;
    return MMD_OK;
}
extern "C" int mmd_op_quantize_fp8(mmd_ctx* c, void* W, int N, int K, uint8_t* q8_out, float* scale_out) {
    if (!c || !W || !q8_out || !scale_out) return MMD_EINVAL;
    if (c->cfg.dtype != MMD_BF16) FAIL(c, MMD_EINVAL, "fp8 weights need a bf16 context");
    hipSetDevice(c->device);
    HIPCHK(c, launch_quantize_fp8_rows(W, N, K, q8_out, scale_out, c->stream));
    return MMD_OK;
}
extern "C" int mmd_op_gemm_w8(mmd_ctx* c, const void* X, const void* Wq, const uint8_t* q8, const float* scale, const void* bias, const void* R, void* Y,
                              int M, int N, int K, int epi, int out_f32, int variant) {
    if (!c || !X || !Wq || !q8 || !scale || !Y) return MMD_EINVAL;
    if (c->cfg.dtype != MMD_BF16 || (N % 16) != 0 || (K % 64) != 0) FAIL(c, MMD_EINVAL, "mmd_op_gemm_w8: bf16 context, N %% 16 == 0, K %% 64 == 0");
    hipSetDevice(c->device);
    if (!c->splitk_ws) { c->splitk_bytes = model_splitk_bytes(c->cfg); int rc = dev_alloc(c, (void**)&c->splitk_ws, c->splitk_bytes); if (rc) return rc; }
    void *Wp = nullptr, *Wp8 = nullptr;
    int rc = make_packed(c, Wq, N, K, &Wp); if (rc) return rc;
    rc = dev_alloc(c, &Wp8, (size_t)N * K, false); if (rc) return rc;
    HIPCHK(c, launch_pack_w8(q8, N, K, Wp8, c->stream));
    const int NO = epi == EPI_SWIGLU ? N / 2 : N;
    rc = gemm(c, X, K, Wq, K, bias, R, NO, Y, NO, M, N, K, epi, out_f32, variant, Wp, false, Wp8, scale);
    hipStreamSynchronize(c->stream);
    dev_free(c, Wp); dev_free(c, Wp8);
    return rc;
}
// producer GEMM (epilogue epi1) -> its only consumer (residual R or none), the intermediate piece-major when `piece_major` and both take the ring kernel (parity tests:
// the same pair with piece_major = 0 must give the same bits).  *used_pm_out reports whether the piece-major layout really was used.
extern "C" int mmd_op_gemm_pair(mmd_ctx* c, const void* X, const void* W1, const void* b1, int epi1, const void* W2, const void* R, void* Y, int M, int N1, int K1, int N2,
                                int piece_major, int* used_pm_out) {
    if (!c || !X || !W1 || !W2 || !Y) return MMD_EINVAL;
    hipSetDevice(c->device);
    if (!c->splitk_ws) { c->splitk_bytes = model_splitk_bytes(c->cfg); int rc = dev_alloc(c, (void**)&c->splitk_ws, c->splitk_bytes); if (rc) return rc; }
    const int T = epi1 == EPI_SWIGLU ? N1 / 2 : N1;
    void *W1p = nullptr, *W2p = nullptr, *mid = nullptr; int rc;
    if ((rc = make_packed(c, W1, N1, K1, &W1p)) || (rc = make_packed(c, W2, N2, T, &W2p)) || (rc = dev_alloc(c, &mid, (size_t)round_up(M, 16) * T * es(c)))) return rc;
    const int epi2 = R ? EPI_RESID : EPI_NONE;
    const bool pm = piece_major && gemm_pair_pm(c, X, K1, W1p, b1, N1, K1, epi1, mid, T, W2p, N2, R, N2, Y, N2, epi2, M);
    if (used_pm_out) *used_pm_out = pm ? 1 : 0;
    rc = gemm(c, X, K1, W1, K1, b1, nullptr, 0, mid, T, M, N1, K1, epi1, 0, GEMM_AUTO, W1p, false, nullptr, nullptr, nullptr, nullptr, pm ? 2 : 0);
    if (!rc) rc = gemm(c, mid, T, W2, T, nullptr, R, N2, Y, N2, M, N2, T, epi2, 0, GEMM_AUTO, W2p, false, nullptr, nullptr, nullptr, nullptr, pm ? 1 : 0);
    hipStreamSynchronize(c->stream);
    dev_free(c, W1p); dev_free(c, W2p); dev_free(c, mid);
    return rc;
}
extern "C" int mmd_op_attention_last_form(mmd_ctx* c, int* out2) { if (!c || !out2) return MMD_EINVAL; out2[0] = c->last_form[0]; out2[1] = c->last_form[1]; return MMD_OK; }
extern "C" int mmd_op_gemm_last_plan(mmd_ctx* c, int* out4) {
    if (!c || !out4) return MMD_EINVAL;
    for (int i = 0; i < 4; ++i) out4[i] = c->last_plan[i];
    return MMD_OK;
}
// the decode steps of the most recent generate call: 0 none or eager, 1 replayed an existing captured step, 2 captured in that call, then replayed
extern "C" int mmd_op_decode_last_route(mmd_ctx* c) { return c ? c->dec_route : MMD_EINVAL; }
extern "C" int mmd_op_step_last_plan(mmd_ctx* c, int* out) { if (!c || !out) return MMD_EINVAL; for (int i = 0; i < STEP_PLAN_FIELDS; ++i) out[i] = c->step_last[i]; return MMD_OK; }
extern "C" int mmd_op_tower_last_plan(mmd_ctx* c, int* out) { if (!c || !out) return MMD_EINVAL; c->tower_last.fields(out); return MMD_OK; }
extern "C" int mmd_op_round_last_record(mmd_ctx* c, int* out4) { if (!c || !out4) return MMD_EINVAL; for (int i = 0; i < ROUND_RECORD_FIELDS; ++i) out4[i] = c->round_record_last[i]; return MMD_OK; }
extern "C" int mmd_op_select_last_plan(mmd_ctx* c, int* out) { if (!c || !out) return MMD_EINVAL; for (int i = 0; i < SELECT_LAST_FIELDS; ++i) out[i] = c->select_last[i]; return MMD_OK; }
// times one GEMM shape on the context's stream with HIP events (weights packed once, outside the timed region)
extern "C" int mmd_op_gemm_bench(mmd_ctx* c, int M, int N, int K, int epi, int variant, int iters, float* avg_ms_out, const void* Xin, const void* Win) {
    if (!c || !avg_ms_out || iters <= 0) return MMD_EINVAL;
    hipSetDevice(c->device);
    if (!c->splitk_ws) { c->splitk_bytes = model_splitk_bytes(c->cfg); int rc = dev_alloc(c, (void**)&c->splitk_ws, c->splitk_bytes); if (rc) return rc; }
    const size_t e = es(c);
    int NO = epi == EPI_SWIGLU ? N / 2 : N;
    void *X = nullptr, *W = nullptr, *Y = nullptr, *R = nullptr, *Wp = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &X, (size_t)M * K * e)) || (rc = dev_alloc(c, &W, (size_t)N * K * e)) || (rc = dev_alloc(c, &Y, (size_t)M * NO * e)) ||
        (rc = dev_alloc(c, &R, (size_t)M * NO * e))) return rc;
    // operand values set the clock (zero / constant operands run 15-20 % faster than random ones, MI355X guide rule 25): the caller
    // passes random X [M,K] / W [N,K]; the byte-pattern fill is only the fallback
    if (Xin) HIPCHK(c, hipMemcpyAsync(X, Xin, (size_t)M * K * e, hipMemcpyDeviceToDevice, c->stream)); else HIPCHK(c, hipMemsetAsync(X, 0x3c, (size_t)M * K * e, c->stream));
    if (Win) HIPCHK(c, hipMemcpyAsync(W, Win, (size_t)N * K * e, hipMemcpyDeviceToDevice, c->stream)); else HIPCHK(c, hipMemsetAsync(W, 0x3b, (size_t)N * K * e, c->stream));
    if (Xin) HIPCHK(c, hipMemcpyAsync(R, Xin, std::min((size_t)M * K, (size_t)M * NO) * e, hipMemcpyDeviceToDevice, c->stream));
    // variant + 1000: the matrix is quantised to fp8 e4m3 first (per-channel scales); the streaming kernels then read the 1-byte copy
    void* Wp8 = nullptr; float* wsc = nullptr;
    if (variant >= 1000) { variant -= 1000; rc = quantize_fp8(c, W, N, K, &Wp8, &wsc); if (rc) return rc; }
    if (variant != GEMM_GENERIC && variant != GEMM_LARGE) { rc = make_packed(c, W, N, K, &Wp); if (rc) return rc; }
    if (variant == 5 && !Wp) FAIL(c, MMD_EINVAL, "slab mode needs a packable shape");
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    unsigned was = c->prof.on; c->prof.on = 0;
    int slabs = 0;
    auto run = [&]() -> int {
        if (variant == 5) {        // skinny path in slab mode (what the fused LLM schedule launches); the consumer kernel is not part of this timing
            GemmArgs g; memset(&g, 0, sizeof(g));
            g.X = X; g.ldx = K; g.Wp = Wp; g.Wp8 = Wp8; g.wscale = wsc; g.M = M; g.N = N; g.K = K; g.epi = EPI_NONE; g.variant = GEMM_SKINNY;
            g.splitk_ws = c->splitk_ws; g.splitk_ws_bytes = c->splitk_bytes; g.slabs_out = &slabs;
            return launch_gemm(c->cfg.dtype, g, c->stream) == hipSuccess ? MMD_OK : MMD_EHIP;
        }
        return gemm(c, X, K, W, K, nullptr, epi == EPI_RESID ? R : nullptr, NO, Y, NO, M, N, K, epi, 0, variant, Wp, false, Wp8, wsc);
    };
    for (int i = 0; i < 3; ++i) { rc = run(); if (rc) return rc; }
    hipEventRecord(a, c->stream);
    for (int i = 0; i < iters; ++i) run();
    hipEventRecord(b, c->stream);
    hipEventSynchronize(b);
    float ms = 0; hipEventElapsedTime(&ms, a, b);
    *avg_ms_out = ms / iters;
    c->prof.on = was;
    hipEventDestroy(a); hipEventDestroy(b);
    dev_free(c, X); dev_free(c, W); dev_free(c, Y); dev_free(c, R); if (Wp) dev_free(c, Wp); if (Wp8) dev_free(c, Wp8); if (wsc) dev_free(c, wsc);
    return MMD_OK;
}
extern "C" int mmd_op_rmsnorm(mmd_ctx* c, const void* x, const void* w, void* y, int M, int H, float eps) {
    if (!c) return MMD_EINVAL; hipSetDevice(c->device);
    HIPCHK(c, launch_rmsnorm(c->cfg.dtype, x, w, y, M, H, eps, c->stream)); return MMD_OK;
}
extern "C" int mmd_op_layernorm(mmd_ctx* c, const void* x, const void* w, const void* b, void* y, int M, int H, float eps) {
    if (!c) return MMD_EINVAL; hipSetDevice(c->device);
    HIPCHK(c, launch_layernorm(c->cfg.dtype, x, w, b, y, M, H, eps, c->stream)); return MMD_OK;
}
extern "C" int mmd_op_resid32_layernorm(mmd_ctx* c, const void* y16, float* h32, const void* pos16, int period, const void* w16, const void* b16, void* out16, void* outbf,
                                        int M, int H, float eps) {
    if (!c) return MMD_EINVAL; hipSetDevice(c->device);
    if (!y16 || !h32 || (w16 && (!b16 || !out16)) || (pos16 && period <= 0)) FAIL(c, MMD_EINVAL, "resid32_layernorm: missing operand");
    if (outbf && w16) FAIL(c, MMD_EINVAL, "resid32_layernorm: outbf (the tower's final bf16 result: h32 is not rewritten) and a LayerNorm output are exclusive");
    HIPCHK(c, launch_resid32_layernorm(y16, h32, pos16, period, w16, b16, out16, outbf, M, H, eps, c->stream)); return MMD_OK;
}
// every piece of code that writes the KV arena, on caller-owned buffers (tests/test_gpu_kv_write.py): what is refused here is refused before any launch
extern "C" int mmd_op_kv_write(mmd_ctx* c, int writer, const void* src, int n_slabs, int slab_rows, const void* bias, const float* inv_freq_host, int S, int nh, int nkv, int d,
                               int64_t pos0, void* q_out, void* Kc, void* Vc, int64_t cap, void* attn_out) {
    if (!c) return MMD_EINVAL;
    if (!src || !inv_freq_host || !Kc || !Vc) FAIL(c, MMD_EINVAL, "kv_write: missing operand");
    if (writer < 0 || writer > 4) FAIL(c, MMD_EINVAL, "kv_write: writer %d (0 .. 4)", writer);
    if (S < 1 || nh < 1 || nkv < 1 || (nh % nkv) != 0 || d < 2 || (d & 1) || pos0 < 0 || cap < 1 || pos0 + S > cap) FAIL(c, MMD_EINVAL, "kv_write: shape (S %d, heads %d / %d, d %d, tokens [%lld, %lld) of %lld)", S, nh, nkv, d, (long long)pos0, (long long)pos0 + S, (long long)cap);
    if (writer >= 1 && (cap % 64) != 0) FAIL(c, MMD_EINVAL, "kv_write: the transposed V layout needs cap %% 64 == 0");
    if (writer >= 2 && c->cfg.dtype != MMD_BF16) FAIL(c, MMD_EINVAL, "kv_write: writer %d is a bf16 kernel", writer);
    if ((writer == 2 || writer == 4) && d != 128) FAIL(c, MMD_EINVAL, "kv_write: writer %d needs head_dim 128", writer);
    if (writer <= 3 && !q_out) FAIL(c, MMD_EINVAL, "kv_write: q_out missing");
    if (writer >= 3 && (!bias || slab_rows < S)) FAIL(c, MMD_EINVAL, "kv_write: the slab writers need a bias and slab_rows >= S");
    if (writer == 3 && (n_slabs < 1 || n_slabs > 16)) FAIL(c, MMD_EINVAL, "kv_write: 1 .. 16 slabs");
    if (writer == 4 && (n_slabs < 1 || n_slabs > 4 || S * (nh / nkv) > 16 || !attn_out)) FAIL(c, MMD_EINVAL, "kv_write: the decode attention takes 1 .. 4 slabs, S x G <= 16 and an output buffer");
    hipSetDevice(c->device);
    const int half = d / 2;
    float* freq = nullptr; void* tab = nullptr;
    HIPCHK(c, hipMalloc((void**)&freq, sizeof(float) * half));
    auto done = [&](int rc) { hipStreamSynchronize(c->stream); hipFree(freq); if (tab) hipFree(tab); return rc; };
    hipError_t e = hipMemcpyAsync(freq, inv_freq_host, sizeof(float) * half, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && (writer == 2 || writer == 4)) {
        e = hipMalloc(&tab, (size_t)S * half * sizeof(float) * 2);
        if (e == hipSuccess) e = launch_rope_table(tab, S, half, freq, pos0, c->stream);
    }
    // (the split-KV workspace of a context that never ran a step: 128 MiB as in mmd_op_attention, an arbitrary test size that stays with the context -- not the model's own sizing)
    if (e == hipSuccess && writer == 4 && !c->attn_ws) { c->attn_bytes = MODEL_ATTN_WS_BYTES; int rc = dev_alloc(c, (void**)&c->attn_ws, c->attn_bytes); if (rc) return done(rc); }
    if (e == hipSuccess) {
        if (writer <= 1) e = launch_rope_append(c->cfg.dtype, src, S, nh, nkv, d, freq, pos0, q_out, Kc, Vc, cap, writer, c->stream);
        else if (writer == 2) e = launch_rope_append_chunk(src, S, nh, nkv, tab, pos0, q_out, Kc, Vc, cap, c->stream);
        else if (writer == 3) e = launch_slab_rope_append((const float*)src, n_slabs, bias, S, nh, nkv, d, freq, pos0, q_out, Kc, Vc, cap, c->stream, nullptr, 0, slab_rows);
        else {
            AttnArgs a; memset(&a, 0, sizeof(a));
            a.q = nullptr; a.ldq = (int64_t)nh * d; a.K = Kc; a.V = Vc; a.k_hs = cap * d; a.k_ts = d; a.v_hs = cap * d; a.v_ts = d; a.v_transposed = 1; a.out = attn_out; a.ldo = (int64_t)nh * d;
            a.S = S; a.nh = nh; a.nkv = nkv; a.d = d; a.n_ctx = pos0; a.causal = 1; a.batch = 1; a.ws = c->attn_ws; a.ws_bytes = c->attn_bytes; a.variant = 3;
            a.qkv_slabs = (const float*)src; a.slab_rows = slab_rows; a.n_slabs = n_slabs; a.qkv_bias = bias; a.rope_tab = tab;
            a.plan_out = c->last_form;
            e = launch_attention(c->cfg.dtype, a, c->stream);
        }
    }
    const int rc = done(MMD_OK);
    if (e != hipSuccess) FAIL(c, MMD_EHIP, "kv_write: writer %d failed: %s", writer, hipGetErrorString(e));
    return rc;
}
// the fused slab consumer (reduce + residual + RMSNorm) on caller-owned buffers (tests/test_gpu_residual_stream.py): launch_slab_resid_rmsnorm and nothing else
extern "C" int mmd_op_slab_resid_rmsnorm(mmd_ctx* c, const float* slabs, int splits, int M, int H, const void* resid, void* h_out, const void* norm_w, float eps, void* xn_out,
                                         const float* wscale) {
    if (!c) return MMD_EINVAL;
    if (!slabs || !resid || !h_out || !norm_w || !xn_out) FAIL(c, MMD_EINVAL, "slab_resid_rmsnorm: missing operand");
    if (c->cfg.dtype != MMD_BF16) FAIL(c, MMD_EINVAL, "slab_resid_rmsnorm: a bf16 kernel");
    if (M < 1 || H < 4 || H > 4096 || (H % 4) != 0 || splits < 1 || splits > 16) FAIL(c, MMD_EINVAL, "slab_resid_rmsnorm: M %d >= 1, H %d <= 4096 and %% 4 == 0, splits %d in 1 .. 16", M, H, splits);
    hipSetDevice(c->device);
    c->last_plan[0] = OP_PLAN_SLAB_RESID; c->last_plan[1] = slab_resid_maxs(splits); c->last_plan[2] = splits; c->last_plan[3] = M;
    const hipError_t e = launch_slab_resid_rmsnorm(slabs, splits, M, H, resid, h_out, norm_w, eps, xn_out, c->stream, wscale);
    hipStreamSynchronize(c->stream);
    if (e != hipSuccess) FAIL(c, MMD_EHIP, "slab_resid_rmsnorm failed: %s", hipGetErrorString(e));
    return MMD_OK;
}
// one GEMV of the decode chain on explicit operands, with the GemmArgs the step builds for it: role GEMV_PRODUCER as layer_tail_chain's o_proj / down_proj (slab_gemm with
// ch_fin), role GEMV_CONSUMER with epi EPI_NONE as layer_qkv (slab_gemm with ch_xn) and with EPI_SWIGLU as layer_tail_chain's gate_up (gemm with ch_xn).  The planner is asked
// first: what it refuses, and a plan of another chain form than `role`, is MMD_EINVAL before anything is packed or launched.
extern "C" int mmd_op_gemv_chain(mmd_ctx* c, int role, const void* X, const void* W, const uint8_t* q8, const float* scale, void* h, const void* gamma, float* ssq, float eps,
                                 void* Y, int M, int N, int K, int epi, int max_splits, int* splits_out) {
    if (!c) return MMD_EINVAL;
    if (role != GEMV_CONSUMER && role != GEMV_PRODUCER) FAIL(c, MMD_EINVAL, "gemv_chain: role %d (1 consumer, 2 producer)", role);
    if (!X || !W || !h || !ssq || (q8 != nullptr) != (scale != nullptr)) FAIL(c, MMD_EINVAL, "gemv_chain: missing operand");
    if (role == GEMV_PRODUCER && (gamma || Y || epi != EPI_NONE)) FAIL(c, MMD_EINVAL, "gemv_chain: the producer takes no gamma, no output and no epilogue (h is updated in place)");
    if (role == GEMV_CONSUMER && (!gamma || !Y || (epi != EPI_NONE && epi != EPI_SWIGLU) || (epi == EPI_NONE && (max_splits < 1 || !splits_out))))
        FAIL(c, MMD_EINVAL, "gemv_chain: the consumer takes gamma and an output; epi 0 (fp32 slabs: max_splits >= 1, splits_out) or 4 (SwiGLU)");
    if (c->cfg.dtype != MMD_BF16) FAIL(c, MMD_EINVAL, "gemv_chain: a bf16 kernel");
    if (M < 1 || M > 16 || N < 16 || (N % 16) != 0 || K < 32 || (K % (q8 ? 64 : 32)) != 0 || (epi == EPI_SWIGLU && (N % 32) != 0))
        FAIL(c, MMD_EINVAL, "gemv_chain: 1 <= M <= 16, N %% 16 == 0 (SwiGLU: %% 32), K %% 32 == 0 (fp8: %% 64); got %d x %d x %d", M, N, K);
    hipSetDevice(c->device);
    if (!c->splitk_ws) { c->splitk_bytes = model_splitk_bytes(c->cfg); int rc = dev_alloc(c, (void**)&c->splitk_ws, c->splitk_bytes); if (rc) return rc; }
    GemvChain ch;
    if (role == GEMV_PRODUCER) { ch.fin_h = h; ch.fin_ssq = ssq; }
    else { ch.xn_h = h; ch.xn_gamma = gamma; ch.xn_ssq = ssq; ch.xn_eps = eps; }
    int splits = 0;
    // the planner looks at null / non-null / alignment of the weight pointers only: W stands in for its packed copies until the plan is known
    GemmArgs a;
    if (role == GEMV_CONSUMER && epi == EPI_SWIGLU) a = gemm_args(c, X, K, W, K, nullptr, nullptr, 0, Y, N / 2, M, N, K, EPI_SWIGLU, 0, GEMM_AUTO, W, false, q8, scale);
    else {
        a = slab_args(c, X, K, W, M, N, K);
        a.Wp8 = q8; a.wscale = scale; a.slabs_out = &splits;
        if (role == GEMV_CONSUMER) { a.splitk_ws = (float*)Y; a.splitk_ws_bytes = (size_t)max_splits * M * N * sizeof(float); }
    }
    a.chain = &ch; a.plan_out = c->last_plan;
    const GemmPlan pl = gemm_plan_for(c->cfg.dtype, a);
    if (!pl.valid() || pl.kernel != GEMM_K_GEMV16 || pl.chain != role) FAIL(c, MMD_EINVAL, "gemv_chain: the planner gives role %d no chain GEMV at %d x %d x %d", role, M, N, K);
    void *Wp = nullptr, *Wp8 = nullptr;
    int rc = make_packed(c, W, N, K, &Wp); if (rc) return rc;
    if (q8) { rc = dev_alloc(c, &Wp8, (size_t)N * K, false); if (rc) { dev_free(c, Wp); return rc; } }
    hipError_t e = q8 ? launch_pack_w8(q8, N, K, Wp8, c->stream) : hipSuccess;
    a.Wp = Wp; a.Wp8 = Wp8;
    if (role == GEMV_PRODUCER || epi == EPI_NONE) a.W = nullptr;          // (slab_gemm knows the packed copies only)
    if (e == hipSuccess) e = launch_gemm(c->cfg.dtype, a, c->stream, &pl);
    hipStreamSynchronize(c->stream);
    dev_free(c, Wp); if (Wp8) dev_free(c, Wp8);
    if (e != hipSuccess) FAIL(c, MMD_EHIP, "gemv_chain: launch failed: %s", hipGetErrorString(e));
    if (splits_out) *splits_out = role == GEMV_CONSUMER && epi == EPI_NONE ? splits : 0;
    return MMD_OK;
}
// the kernels of the plain greedy token loop on caller-owned buffers (tests/test_gpu_greedy.py): the production launchers over the context's own scratch, nothing else.
// What is refused is refused before any launch.
extern "C" int mmd_op_argmax(mmd_ctx* c, int form, const float* logits, int n, int V, const int64_t* prev_ids_dev, const int32_t* prev_off_host, const float* penalty_host,
                             int64_t* tokens_out, int64_t* tok_slots_out, int64_t* append_out) {
    if (!c) return MMD_EINVAL;
    if (form < 0 || form > 2) FAIL(c, MMD_EINVAL, "argmax: form %d (0 list length in the argument, 1 in a StepState, 2 the multi-row launch)", form);
    if (!logits || !tokens_out || !prev_off_host || !penalty_host || n < 1 || n > 4096 || V < 1) FAIL(c, MMD_EINVAL, "argmax: missing operand, or n %d outside 1 .. 4096, or V %d < 1", n, V);
    if (form == 2 && (n > MMD_ROUND_MAX_SAMPLERS || !tok_slots_out || !append_out)) FAIL(c, MMD_EINVAL, "argmax: form 2 takes at most %d rows, token slots and append slots", MMD_ROUND_MAX_SAMPLERS);
    if (prev_off_host[0] != 0) FAIL(c, MMD_EINVAL, "argmax: the list offsets start at 0");
    for (int r = 0; r < n; ++r) if (prev_off_host[r + 1] < prev_off_host[r]) FAIL(c, MMD_EINVAL, "argmax: the list offsets decrease at row %d", r);
    if (prev_off_host[n] > 0 && !prev_ids_dev) FAIL(c, MMD_EINVAL, "argmax: lists without ids");
    hipSetDevice(c->device);
    hipStream_t st = c->stream;
    // per row what generate_impl / mmd_round_multi hand on: penalty off -> no list and the factor 1
    auto len_of = [&](int r) { return penalty_host[r] > 0.f ? prev_off_host[r + 1] - prev_off_host[r] : 0; };
    auto pen_of = [&](int r) { return penalty_host[r] > 0.f ? penalty_host[r] : 1.f; };
    StepState* dyn = nullptr;
    hipError_t e = hipSuccess;
    if (form == 1) {
        std::vector<StepState> hs((size_t)n);
        for (int r = 0; r < n; ++r) { memset(&hs[r], 0, sizeof(StepState)); hs[r].n_prev = len_of(r); }
        HIPCHK(c, hipMalloc((void**)&dyn, sizeof(StepState) * n));
        e = hipMemcpy(dyn, hs.data(), sizeof(StepState) * n, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && form == 2) {
        if (!c->round_scratch) { int rc = dev_alloc(c, &c->round_scratch, sample_batch_scratch_bytes()); if (rc) return rc; }
        SampleBatch b{};
        for (int r = 0; r < n; ++r) {
            b.prev[r] = prev_ids_dev + prev_off_host[r]; b.n_prev[r] = len_of(r); b.penalty[r] = pen_of(r);
            b.tok[r] = tok_slots_out + r; b.append[r] = penalty_host[r] > 0.f ? append_out + r : nullptr;
        }
        e = launch_sample_batch(logits, V, b, n, tokens_out, c->round_scratch, st);
    } else if (e == hipSuccess) {
        for (int r = 0; r < n && e == hipSuccess; ++r)          // (one row after the other through the one scratch: same stream)
            e = launch_argmax_penalty(logits + (size_t)r * V, V, prev_ids_dev + prev_off_host[r], form == 1 ? 0 : len_of(r), pen_of(r), tokens_out + r, st, dyn ? dyn + r : nullptr, c->argmax_scratch);
    }
    hipStreamSynchronize(st);
    if (dyn) hipFree(dyn);
    if (e != hipSuccess) FAIL(c, MMD_EHIP, "argmax: form %d failed: %s", form, hipGetErrorString(e));
    return MMD_OK;
}
// one launch of advance_state_kernel without constraints on a StepState of its own: the token and the state go in and come out on the host, the list is the caller's
extern "C" int mmd_op_advance_state(mmd_ctx* c, int64_t token, int64_t eos_id, int use_penalty, int64_t* prev_dev, int prev_cap, int* n_prev_inout_host, int64_t* n_ctx_inout_host,
                                    int* step_inout_host) {
    if (!c) return MMD_EINVAL;
    if (!prev_dev || !n_prev_inout_host || !n_ctx_inout_host || !step_inout_host) FAIL(c, MMD_EINVAL, "advance_state: missing operand");
    if (prev_cap < 0 || *n_prev_inout_host < 0 || *n_prev_inout_host > prev_cap) FAIL(c, MMD_EINVAL, "advance_state: list length %d outside 0 .. prev_cap %d", *n_prev_inout_host, prev_cap);
    hipSetDevice(c->device);
    struct { StepState s; int64_t tok; } h;
    memset(&h, 0, sizeof(h));
    h.s.n_prev = *n_prev_inout_host; h.s.n_ctx = *n_ctx_inout_host; h.s.step = *step_inout_host; h.tok = token;
    char* dev = nullptr;
    HIPCHK(c, hipMalloc((void**)&dev, sizeof(h)));
    hipError_t e = hipMemcpy(dev, &h, sizeof(h), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_advance_state((StepState*)dev, (const int64_t*)(dev + offsetof(decltype(h), tok)), prev_dev, prev_cap, eos_id, use_penalty ? 1 : 0, c->stream, nullptr);
    hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(&h, dev, sizeof(h), hipMemcpyDeviceToHost);
    hipFree(dev);
    if (e != hipSuccess) FAIL(c, MMD_EHIP, "advance_state failed: %s", hipGetErrorString(e));
    *n_prev_inout_host = h.s.n_prev; *n_ctx_inout_host = h.s.n_ctx; *step_inout_host = h.s.step;
    return MMD_OK;
}
// launch_embed_feed over the context's embedding table: out[rows_host[i], :] = embed[clamp(tok_slots_dev[i]), :], out [out_rows, hidden] in the context dtype
extern "C" int mmd_op_embed_feed(mmd_ctx* c, const int64_t* tok_slots_dev, const int32_t* rows_host, int n, int out_rows, void* out) {
    NEED_FINAL(c);
    if (!tok_slots_dev || !rows_host || !out || n < 1 || n > MMD_ROUND_MAX_SAMPLERS) FAIL(c, MMD_EINVAL, "embed_feed: missing operand, or n %d outside 1 .. %d", n, MMD_ROUND_MAX_SAMPLERS);
    for (int i = 0; i < n; ++i) if (rows_host[i] < 0 || rows_host[i] >= out_rows) FAIL(c, MMD_EINVAL, "embed_feed: row %d outside the %d rows of the output", rows_host[i], out_rows);
    FeedBatch f{};
    for (int i = 0; i < n; ++i) { f.tok[i] = tok_slots_dev + i; f.row[i] = rows_host[i]; }
    const hipError_t e = launch_embed_feed(c->cfg.dtype, c->embed, f, n, c->cfg.hidden_size, c->cfg.vocab_size, out, c->stream);
    hipStreamSynchronize(c->stream);
    if (e != hipSuccess) FAIL(c, MMD_EHIP, "embed_feed failed: %s", hipGetErrorString(e));
    return MMD_OK;
}
extern "C" int mmd_op_rope_append(mmd_ctx* c, void* qkv, int S, int nh, int nkv, int d, float theta, int64_t pos0, void* q_out, void* Kc, void* Vc, int64_t cap) {
    if (!c) return MMD_EINVAL; hipSetDevice(c->device);
    std::vector<float> t(d / 2);
    for (int i = 0; i < d / 2; ++i) t[i] = (float)(1.0 / std::pow((double)theta, (double)(2 * i) / (double)d));
    float* dev = nullptr;
    HIPCHK(c, hipMalloc((void**)&dev, sizeof(float) * (d / 2)));
    HIPCHK(c, hipMemcpyAsync(dev, t.data(), sizeof(float) * (d / 2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_rope_append(c->cfg.dtype, qkv, S, nh, nkv, d, dev, pos0, q_out, Kc, Vc, cap, 0, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(dev);
    return MMD_OK;
}
extern "C" int mmd_op_attention(mmd_ctx* c, const void* q, const void* Kc, const void* Vc, void* out, int S, int nh, int nkv, int d, int64_t n_ctx,
                                int64_t cap, int causal, int variant) {
    if (!c) return MMD_EINVAL; hipSetDevice(c->device);
    if (!c->attn_ws) { c->attn_bytes = MODEL_ATTN_WS_BYTES; int rc = dev_alloc(c, (void**)&c->attn_ws, c->attn_bytes); if (rc) return rc; }
    AttnArgs a; memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = (int64_t)nh * d; a.K = Kc; a.V = Vc; a.k_hs = cap * d; a.k_ts = d; a.v_hs = cap * d; a.v_ts = d; a.out = out; a.ldo = (int64_t)nh * d;
    a.S = S; a.nh = nh; a.nkv = nkv; a.d = d; a.n_ctx = n_ctx; a.causal = causal; a.batch = 1; a.ws = c->attn_ws; a.ws_bytes = c->attn_bytes; a.variant = variant;
    void* vt = nullptr;
    if (variant == 3 || variant == 5 || variant == 6) {        // the GQA-128 kernels read the transposed V arena layout: convert the row-major test input
        if (cap % 64 != 0) FAIL(c, MMD_EINVAL, "variant 3 needs cap %% 64 == 0");
        int rc = dev_alloc(c, &vt, (size_t)nkv * cap * d * es(c)); if (rc) return rc;
        HIPCHK(c, launch_transpose_v(c->cfg.dtype, Vc, vt, nkv, cap, d, c->stream));
        a.V = vt; a.v_transposed = 1;
    }
    a.plan_out = c->last_form;
    hipError_t le = launch_attention(c->cfg.dtype, a, c->stream);
    if (vt) { hipStreamSynchronize(c->stream); dev_free(c, vt); }
    HIPCHK(c, le);
    return MMD_OK;
}
// times the LLM attention (incl. the split-KV combine) at a given step size / context length with HIP events
extern "C" int mmd_op_attention_bench(mmd_ctx* c, int S, int nh, int nkv, int d, int64_t n_ctx, int variant, int iters, float* avg_ms_out) {
    if (!c || !avg_ms_out || iters <= 0) return MMD_EINVAL;
    hipSetDevice(c->device);
    if (!c->attn_ws) { c->attn_bytes = MODEL_ATTN_WS_BYTES; int rc = dev_alloc(c, (void**)&c->attn_ws, c->attn_bytes); if (rc) return rc; }
    const size_t e = es(c);
    int64_t cap = round_up(n_ctx + S, 64);
    void *q = nullptr, *K = nullptr, *V = nullptr, *o = nullptr; int rc;
    if ((rc = dev_alloc(c, &q, (size_t)S * nh * d * e)) || (rc = dev_alloc(c, &K, (size_t)nkv * cap * d * e)) || (rc = dev_alloc(c, &V, (size_t)nkv * cap * d * e)) ||
        (rc = dev_alloc(c, &o, (size_t)S * nh * d * e))) return rc;
    HIPCHK(c, hipMemsetAsync(q, 0x3c, (size_t)S * nh * d * e, c->stream));
    HIPCHK(c, hipMemsetAsync(K, 0x3b, (size_t)nkv * cap * d * e, c->stream));
    HIPCHK(c, hipMemsetAsync(V, 0x3c, (size_t)nkv * cap * d * e, c->stream));
    AttnArgs a; memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = (int64_t)nh * d; a.K = K; a.V = V; a.k_hs = cap * d; a.k_ts = d; a.v_hs = cap * d; a.v_ts = d; a.out = o; a.ldo = (int64_t)nh * d;
    a.S = S; a.nh = nh; a.nkv = nkv; a.d = d; a.n_ctx = n_ctx; a.causal = 1; a.batch = 1; a.ws = c->attn_ws; a.ws_bytes = c->attn_bytes; a.variant = variant;
    a.v_transposed = 1; a.plan_out = c->last_form;
    hipEvent_t ea, eb; hipEventCreate(&ea); hipEventCreate(&eb);
    for (int i = 0; i < 3; ++i) HIPCHK(c, launch_attention(c->cfg.dtype, a, c->stream));
    hipEventRecord(ea, c->stream);
    for (int i = 0; i < iters; ++i) launch_attention(c->cfg.dtype, a, c->stream);
    hipEventRecord(eb, c->stream);
    hipEventSynchronize(eb);
    float ms = 0; hipEventElapsedTime(&ms, ea, eb);
    *avg_ms_out = ms / iters;
    hipEventDestroy(ea); hipEventDestroy(eb);
    dev_free(c, q); dev_free(c, K); dev_free(c, V); dev_free(c, o);
    return MMD_OK;
}
extern "C" int mmd_op_pool(mmd_ctx* c, const void* x, void* y, int B, int grid, int H, int mode, int stride) {
    if (!c) return MMD_EINVAL; hipSetDevice(c->device);
    HIPCHK(c, launch_pool(c->cfg.dtype, x, y, B, grid, H, mode, stride, c->stream)); return MMD_OK;
}
