// tower_plan.h -- which schedule one vision-tower run takes, and nothing else.  One pure host function, tower_plan(): no GPU header, no runtime call, no environment; it
// compiles with the host C++17 compiler alone (tests/test_tower_plan_host.py runs the table of tests/tower_regimes.py through it without a GPU).  tower_begin (model.hip)
// evaluates it once per run and stores it in the context, tower_run launches what it says; the projector behind the tower takes its row set from the same plan, and
// mmd_op_tower_last_plan reads the answer back.  Every threshold of the schedule lives here; whether fc1's output may be piece-major is asked of gemm_plan() about the
// arguments the tail will launch with, never restated.
#pragma once
#include <stdio.h>
#include "gemm_plan.h"

// ---- the thresholds ------------------------------------------------------------------------------------------------
constexpr int TOWER_POOL_TAPS = 4;                // the bilinear pool behind the projector reads 2 x 2 taps per output: (2 out)^2 = 4 out^2 tokens of a frame (196 of 729 at the shipped sizes)
// the half forms of the kernels exist for M > 64 GEMMs and S >= 64 attention only: a compact block below either keeps the full last layer
constexpr int TOWER_HALF_MIN_QUERIES = 64;        //   attention: the compact block's query rows per frame, U >= 64
constexpr int TOWER_HALF_GEMM_ABOVE = 64;         //   GEMMs: the compact block's rows in all, B * U > 64

// what the decision depends on besides the run itself: what mmd_create / mmd_finalize_weights know
struct TowerModel {
    int dtype = MMD_BF16;              // the model dtype
    int tower_f16 = 0;                 // 0: the tower computes in the model dtype | 1: IEEE half with the fp32 residual stream (autocast) | 2: IEEE half, fp16 residual stream
    int C = 0, heads = 0, ipad = 0;    // width, heads, fc1 rows / fc2 columns (padded to 64)
    int grid = 0, tokens = 0, seq = 0, layers = 0;          // tokens = grid^2; seq = tokens (+ 1 with a class token)
    int pool_mode = MMD_POOL_BILINEAR, pool_stride = 1;
    bool class_token = false, pre_ln = false, post_ln = false;          // (pre_ln governs no field: pre_layrnorm runs in place on the stream's start in every form)
    int act = 0;                       // 1: quick-GELU (CLIP) -- plain fc1, then the activation in a pass of its own
    bool vision_only = false;
    int max_batch = 0;
    bool fc1_p = false, fc2_p = false;          // the MFMA-fragment-major copies of fc1 / fc2 exist (bf16 context, N % 16 == 0, K % 32 == 0)
    size_t splitk_ws_bytes = 0;        // the tower's own split-K workspace
};
struct TowerShape {
    int B = 0;
    bool for_pool = false;             // the encode entry points (projector + pool follow); false: mmd_vision_tower, which returns every token
    bool full_tower = false;           // mmd_vit_set_full_tower(1): the last layer runs on ALL tokens (feature extraction, debug taps)
    int ring_flags = -1, ring_max_blocks = 0;          // mmd_set_tower_share (ring_flags < 0: never called): the cap reaches gemm_plan()
};

enum { TOWER_RESID_EPI = 0,            // model-dtype residual stream: o_proj / fc2 add it in their epilogue (EPI_RESID), LayerNorm is a launch of its own
       TOWER_RESID_F32 = 1,            // fp32 residual stream, as under autocast (`fp16 + model-dtype` and `fp32 + fp16` promote; LayerNorm returns fp32): the linears write their
                                       //   fp16 result (bias inside, one rounding) and resid32_layernorm folds it into the stream and emits the next linear's input
       TOWER_RESID_F16 = 2 };          // the EPI schedule in IEEE half (the sum is rounded to fp16 after every sublayer), ONE convert to the model dtype at the end
enum { TOWER_EMBED_ADD_ROWS = 0,       // position table added to the patch rows in place
       TOWER_EMBED_CLS = 1,            // class token spliced in front of the patch rows, position table added (CLIP)
       TOWER_EMBED_F32 = 2 };          // stream = float(patch fp16) + float(position table), layer 0's LayerNorm 1 in the same pass
constexpr int TOWER_PLAN_FIELDS = 12;
struct TowerPlan {
    int rc = MMD_OK; char error[96] = "";          // rc != MMD_OK: the run is refused with this message
    int dt = MMD_BF16;                 // the element type the tower computes in (MMD_F16 under tower_f16; pixel_values arrive in the model dtype and become half in the im2col pass)
    int resid = TOWER_RESID_EPI, embed = TOWER_EMBED_ADD_ROWS;
    // everything after the LAST layer's K / V is row-wise: that layer's queries, o_proj, LayerNorm, MLP run on the rows the pool reads alone (K and V still come from all tokens)
    bool sparse_last = false;
    int pout = 0, U = 0;               // pool outputs per grid side; rows of a frame the pool reads, TOWER_POOL_TAPS * pout^2
    int compact_rows = 0;              // B * U when sparse_last, else 0
    bool proj_compact = false;         // the projector behind the tower runs on the rows the pool reads ...
    bool proj_gather = false;          // ... and gathers them itself (false: the sparse last layer already left exactly these rows)
    bool mlp_pm = false, mlp_pm_last = false;          // fc1's output (its only reader is fc2) is piece-major: in the full-row layers / in the compact last layer
    bool final_convert = false;        // the output is converted from half to the model dtype in a pass of its own (TOWER_RESID_F32 casts in its last residual pass)
    void fields(int* out) const {      // what mmd_op_tower_last_plan reports
        const int v[TOWER_PLAN_FIELDS] = {dt, resid, embed, sparse_last, pout, U, compact_rows, proj_compact, proj_gather, mlp_pm, mlp_pm_last, final_convert};
        for (int i = 0; i < TOWER_PLAN_FIELDS; ++i) out[i] = v[i];
    }
};

static inline int tower_pool_out(const TowerModel& m) { return (m.grid + m.pool_stride - 1) / m.pool_stride; }

// The row set of the projector (row-wise: Linear, GELU, Linear) in front of the pool.  Bilinear pooling reads TOWER_POOL_TAPS * pout^2 tokens of each frame: the projector runs on
// those alone.  A class token is not among the grid tokens the pool reads (seq > tokens): such towers keep every row, indexed per frame by `tokens`.  all_tokens: the stage-1
// debug tap wants connector() of every token.  tower_left_compact: the tower's sparse last layer already left exactly these rows.
struct TowerProjectorPlan { bool compact = false, gather = false; int pout = 0; };
static inline TowerProjectorPlan tower_projector_plan(const TowerModel& m, bool all_tokens, bool tower_left_compact = false) {
    TowerProjectorPlan p;
    p.pout = tower_pool_out(m);
    p.compact = m.pool_mode == MMD_POOL_BILINEAR && !all_tokens && TOWER_POOL_TAPS * p.pout * p.pout < m.tokens && m.seq == m.tokens;
    p.gather = p.compact && !tower_left_compact;
    return p;
}

// ---- the GEMM pair the plan asks gemm_plan() about --------------------------------------------------------------------
// Buffers and weights count as present / absent only (gemm_plan reads a pointer as null / non-null / aligned): every tower buffer, bias and the compact blocks inside v_col /
// v_mlp start an allocation of their own (256-byte aligned), so one aligned stand-in serves.
static inline void* tower_stub() { alignas(256) static char b[256]; return b; }
// fc1 (+ GELU) -> fc2 over M rows as the tail launches them: may fc1's output live in the ring kernel's piece-major layout?  Yes when the automatic dispatch runs BOTH on
// gemm_ringx_kernel, fc1 on the PLAIN ring (its split-K form writes row-major through splitk_reduce -- ADVICE r05)
static inline bool tower_mlp_pm(const TowerModel& m, const TowerShape& s, int dt, bool resid_epi, int M, const GemmTuning& tune) {
    GemmArgs a{}, b{};
    a.X = tower_stub(); a.ldx = m.C; a.Wp = m.fc1_p ? tower_stub() : nullptr; a.bias = tower_stub(); a.Y = tower_stub(); a.ldy = m.ipad;
    a.M = M; a.N = m.ipad; a.K = m.C; a.epi = EPI_GELU_TANH;
    b.X = tower_stub(); b.ldx = m.ipad; b.Wp = m.fc2_p ? tower_stub() : nullptr; b.Y = tower_stub(); b.ldy = m.C; if (resid_epi) { b.R = tower_stub(); b.ldr = m.C; }
    b.M = M; b.N = m.C; b.K = m.ipad; b.epi = resid_epi ? EPI_RESID : EPI_NONE;
    GemmArgs* const both[2] = {&a, &b};
    for (GemmArgs* g : both) {
        g->variant = GEMM_AUTO; g->splitk_ws = m.splitk_ws_bytes ? (float*)tower_stub() : nullptr; g->splitk_ws_bytes = m.splitk_ws_bytes;
        if (s.ring_flags >= 0) { g->ring_flags = s.ring_flags; g->ring_max_blocks = s.ring_max_blocks; }
    }
    return gemm_plan(dt, a, tune).ring_auto == RING_AUTO_PLAIN && gemm_plan(dt, b, tune).ring_auto != RING_AUTO_NONE;
}

// The schedule of one tower run over B frames.  no_pm: MMDUET_NO_FUSE=1 | 2 (StepSwitches::no_pm): MLP intermediates stay row-major.
static inline TowerPlan tower_plan(const TowerModel& m, const TowerShape& s, bool no_pm, const GemmTuning& tune) {
    TowerPlan p;
    if (s.B > m.max_batch) { p.rc = MMD_ERANGE; snprintf(p.error, sizeof(p.error), "vit batch %d exceeds max_vit_batch %d", s.B, m.max_batch); return p; }
    p.dt = m.tower_f16 ? MMD_F16 : m.dtype;
    p.resid = m.tower_f16 == 1 ? TOWER_RESID_F32 : m.tower_f16 == 2 ? TOWER_RESID_F16 : TOWER_RESID_EPI;
    p.embed = p.resid == TOWER_RESID_F32 ? TOWER_EMBED_F32 : m.class_token ? TOWER_EMBED_CLS : TOWER_EMBED_ADD_ROWS;
    p.final_convert = p.resid == TOWER_RESID_F16;
    p.pout = tower_pool_out(m); p.U = TOWER_POOL_TAPS * p.pout * p.pout;
    // Same values into the same arithmetic as the full last layer; callers that want the tower's full output switch it off with mmd_vit_set_full_tower.  Not with a
    // post_layernorm or a class token (the projector then keeps every row), nor for the quick-GELU MLP (secondary towers)
    p.sparse_last = s.for_pool && !s.full_tower && m.pool_mode == MMD_POOL_BILINEAR && p.U < m.tokens && m.seq == m.tokens && !m.post_ln && m.act != 1 && m.layers > 0 &&
                    !m.vision_only && (!m.tower_f16 || (p.U >= TOWER_HALF_MIN_QUERIES && s.B * p.U > TOWER_HALF_GEMM_ABOVE));
    p.compact_rows = p.sparse_last ? s.B * p.U : 0;
    if (s.for_pool && !m.vision_only) {
        const TowerProjectorPlan pp = tower_projector_plan(m, false, p.sparse_last);
        p.proj_compact = pp.compact; p.proj_gather = pp.gather;
    }
    if (!no_pm && m.act != 1) {
        const bool epi = p.resid != TOWER_RESID_F32;
        p.mlp_pm = m.layers > 0 && tower_mlp_pm(m, s, p.dt, epi, s.B * m.seq, tune);
        p.mlp_pm_last = p.sparse_last && tower_mlp_pm(m, s, p.dt, epi, p.compact_rows, tune);
    }
    return p;
}
