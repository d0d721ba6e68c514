// step_plan.h -- which launch schedule one LLM step takes, and nothing else.  One pure host function, step_plan(): no GPU header, no runtime call, no environment; it
// compiles with the host C++17 compiler alone (tests/test_step_plan_host.py runs the table of tests/step_regimes.py through it without a GPU).  llm_step_segs (model.hip)
// evaluates it once per step, after validating its arguments, and launches what it says; mmd_op_step_last_plan reads the answer back.  Every threshold of the schedule
// lives here; what a GEMM kernel can take is asked of gemm_plan() about the arguments the step will launch with, never restated.
#pragma once
#include "gemm_plan.h"

// ---- the thresholds ------------------------------------------------------------------------------------------------
constexpr int STEP_FUSED_MAX_ROWS = 256;          // fused slabs: the weight-streaming regime (gemv16 / skinny up to 64 rows, gemm_stream_kernel up to 256) -- above it the tile GEMMs
//                GEMV_CHAIN_ROWS (gemm_plan.h)   // decode chain: rows the chain's consumer GEMV keeps in LDS
constexpr int STEP_ROW_MAX_H = 4096;              // the slab consumers (reduce + residual + RMSNorm) and the chain's sums of squares hold one row of H: H <= 4096,
constexpr int STEP_ROW_H_VEC = 4;                 //   H a whole number of 4-element vectors (slab consumers) ...
constexpr int STEP_CHAIN_H_TILE = 64;             //   ... and of 64-column producer tiles (chain)
constexpr int STEP_TABLE_HEAD_DIM = 128;          // the (cos, sin) table kernels, the attention kernel's own q / k / v preparation and the batched decode attention exist at head_dim 128
constexpr int STEP_ROPE_FUSED_MULTI_ROWS = 16;    // a round of talking streams only prepares q / k / v inside the batched attention up to this many rows in all
constexpr int STEP_ROPE_FUSED_MAX_SLABS = 4;      // the attention kernel's own q / k / v preparation sums at most four qkv slabs
constexpr int STEP_CHUNK_ROPE_MIN_ROWS = 64;      // the vectorised RoPE + append over a per-step table pays from this many rows
constexpr int STEP_SPARSE_LAST_ABOVE = 64;        // the last layer runs on the read rows only in steps LONGER than this ...
constexpr int STEP_NEED_MAX = 64;                 // ... that read at most this many rows (the weight-streaming kernels' M <= 64); also the capacity of a step's need list
constexpr int STEP_MULTI_ATTN_Q_ROWS = 16;        // batched decode attention: rows per stream x query heads per kv head fill at most one 16-row MFMA tile
constexpr int STEP_MULTI_ATTN_MIN_RUN = 2;        //   from two streams
constexpr int STEP_MULTI_ATTN_MAX_RUN = 64;       //   up to 64 (a slot of per-stream states holds 64)
constexpr int STEP_MULTI_ATTN_MAX_KV = 256;       //   and run x kv heads <= 256

// the A/B switches of the schedule: read from the environment when a context is created (mmd_create)
struct StepSwitches {
    bool no_fuse = false;              // MMDUET_NO_FUSE=1: keep the unfused launch schedule (A/B and parity cross-check)
    bool no_pm = false;                // MMDUET_NO_FUSE=1 | 2: MLP intermediates stay row-major (gemm_pair_pm)
    bool no_chain = false;             // MMDUET_NO_CHAIN=1: decode steps keep the separate reduce+residual+RMSNorm launches
    bool no_slab_norm = false;         // MMDUET_NO_SLAB_NORM=1: a chunk's split-K down_proj keeps splitk_reduce + a separate RMSNorm launch
    bool full_last_layer = false;      // MMDUET_FULL_LAST_LAYER=1: a chunk's last decoder layer keeps o_proj / MLP / final norm on all rows
    bool no_rope_fuse = false;         // MMDUET_NO_ROPE_FUSE=1: decode steps keep the slab_rope_append launch
    bool no_multi_fuse = false;        // MMDUET_NO_MULTI_FUSE set: steps of several streams keep the unfused form
    bool no_multi_attn = false;        // MMDUET_NO_MULTI_ATTN set: the talking streams' attention runs per stream
    bool no_chunk_rope = false;        // MMDUET_NO_CHUNK_ROPE set: chunks keep the scalar RoPE + append kernel
};

// what the decision depends on besides the step itself: the context's model and buffers
struct StepModel {
    int dtype = MMD_BF16;
    int H = 0, I = 0, nh = 0, nkv = 0, d = 0, qkv_w = 0, layers = 0;
    bool qkv_p = false, o_p = false, gu_p = false, down_p = false;          // the MFMA-fragment-major copy of each layer matrix exists (bf16, N % 16 == 0, K % 32 == 0)
    bool fp8 = false;                  // fp8 copies + per-channel scales exist (weight_dtype fp8)
    bool attn_ws = false;              // the attention workspace exists
    size_t splitk_ws_bytes = 0;        // the split-K workspace (0: none)
};
struct StepShape {
    int S = 0;                         // rows of the step
    const int* seg_rows = nullptr; int nseg = 0;          // rows of each stream's segment, in order
    int n_need = 0;                    // rows of the caller's need list (0: none)
    bool hidden_out = false;           // the caller wants every row's final hidden state
    bool dyn = false;                  // the step is being captured into the decode graph
};

enum { STEP_TILE = 0,                  // the tile schedule: every GEMM applies its own epilogue (chunks, fp32 contexts)
       STEP_FUSED = 1,                 // fused slabs: the streaming GEMMs leave fp32 K slabs, the next operator consumes them
       STEP_CHAIN = 2 };               // decode chain: o_proj / down_proj fold into the residual stream, qkv / gate_up normalise per lane (GemvChain)
constexpr int STEP_PLAN_FIELDS = 9;
struct StepPlan {
    int rc = MMD_OK; const char* error = nullptr;          // rc != MMD_OK: the arguments are refused with this message
    int schedule = STEP_TILE;
    bool rope_fused = false;           // the attention kernel prepares q / k / v from the qkv slabs itself (fused and chain schedules)
    bool chunk_rope = false;           // tile schedule: one (cos, sin) table per step, the vectorised RoPE + append kernel
    bool sparse_last = false;          // tile schedule: the last layer's o_proj / MLP / final norm run on the need list's rows
    int run0 = 0, run_n = 0;           // segments [run0, run0 + run_n) share ONE batched decode attention launch (run_n == 0: none)
    bool run_all = false;              // ... and they are all the segments of the step (a round of talking streams only)
    bool down_slab_norm = false;       // tile schedule: down_proj leaves its split-K slabs to the fused residual + RMSNorm pass
    bool mlp_pm = false;               // tile schedule: the SwiGLU product between gate_up and down_proj is piece-major
    void fields(int* out) const {      // what mmd_op_step_last_plan reports
        const int v[STEP_PLAN_FIELDS] = {schedule, rope_fused, chunk_rope, sparse_last, run0, run_n, run_all, down_slab_norm, mlp_pm};
        for (int i = 0; i < STEP_PLAN_FIELDS; ++i) out[i] = v[i];
    }
};

// ---- the GEMMs the plan asks gemm_plan() about ------------------------------------------------------------------------
// Buffers and weights count as present / absent only: every activation buffer of a context is an allocation of its own (256-byte aligned), so one aligned stand-in serves.
static inline void* step_stub() { alignas(256) static char b[256]; return b; }
// a slab-mode GEMM of the step (slab_args of model.hip): X [M,K] at row stride ldx, packed weights, fp32 K slabs into the split-K workspace
static inline GemmArgs step_slab_args(const StepModel& m, bool packed, int64_t ldx, int M, int N, int K) {
    GemmArgs a{};
    a.X = step_stub(); a.ldx = ldx; a.Wp = packed ? step_stub() : nullptr; a.M = M; a.N = N; a.K = K; a.epi = EPI_NONE; a.variant = GEMM_SKINNY;
    a.splitk_ws = m.splitk_ws_bytes ? (float*)step_stub() : nullptr; a.splitk_ws_bytes = m.splitk_ws_bytes;
    return a;
}
static inline bool step_can_slab(const StepModel& m, const GemmArgs& a, const GemmTuning& tune) {          // (gemm_can_slab)
    int sink = 0; GemmArgs b = a; b.slabs_out = &sink; b.epi = EPI_NONE;
    const int k = gemm_plan(m.dtype, b, tune).kernel;
    return k == GEMM_K_GEMV16 || k == GEMM_K_SKINNY || k == GEMM_K_STREAM;
}
// a tile-schedule GEMM as gemm() of model.hip launches it (GEMM_AUTO, packed weights where they exist; the row-major copy does not change which packed kernel runs)
static inline GemmArgs step_tile_args(const StepModel& m, bool packed, int64_t ldx, bool resid, int64_t ldy, int M, int N, int K, int epi) {
    GemmArgs a{};
    a.X = step_stub(); a.ldx = ldx; a.Wp = packed ? step_stub() : nullptr; a.Y = step_stub(); a.ldy = ldy; if (resid) { a.R = step_stub(); a.ldr = ldy; }
    a.M = M; a.N = N; a.K = K; a.epi = epi; a.variant = GEMM_AUTO;
    a.splitk_ws = m.splitk_ws_bytes ? (float*)step_stub() : nullptr; a.splitk_ws_bytes = m.splitk_ws_bytes;
    return a;
}

// The schedule of one causal forward over `nseg` streams' segments.  The caller has checked that the segments are non-empty and cover the S rows.
static inline StepPlan step_plan(const StepModel& m, const StepShape& s, const StepSwitches& sw, const GemmTuning& tune) {
    StepPlan p;
    const int S = s.S, H = m.H, I = m.I, q_w = m.nh * m.d;
    const bool bf16 = m.dtype == MMD_BF16;
    if (s.dyn && s.nseg != 1) { p.rc = MMD_EINVAL; p.error = "graph decode is single-stream"; return p; }
    const bool row_ok = bf16 && H <= STEP_ROW_MAX_H && (H % STEP_ROW_H_VEC) == 0 && !sw.no_fuse;          // the fused slab consumers take this context's rows
    const bool table_ok = bf16 && m.d == STEP_TABLE_HEAD_DIM && !sw.no_fuse;

    // Fused slabs: qkv, o_proj and down_proj all leave slabs at S rows.  (Several streams in one step -- a scheduler round's talking streams -- take the same schedule: the
    // GEMVs and the slab consumers are row-wise, RoPE + KV append + attention read each stream's rows of the slabs at its row offset.)
    const bool fused = (s.nseg == 1 || !sw.no_multi_fuse) && row_ok && S <= STEP_FUSED_MAX_ROWS &&
                       step_can_slab(m, step_slab_args(m, m.qkv_p, H, S, m.qkv_w, H), tune) && step_can_slab(m, step_slab_args(m, m.down_p, I, S, H, I), tune) &&
                       step_can_slab(m, step_slab_args(m, m.o_p, q_w, S, H, q_w), tune);
    // Decode chain: every GEMM of the step is the weight-streaming GEMV
    const bool chain = fused && S <= GEMV_CHAIN_ROWS && !sw.no_chain && (H % STEP_CHAIN_H_TILE) == 0 && H <= STEP_ROW_MAX_H;
    p.schedule = chain ? STEP_CHAIN : fused ? STEP_FUSED : STEP_TILE;
    if (s.dyn && !fused) { p.rc = MMD_EINVAL; p.error = "graph decode needs the fused bf16 schedule"; return p; }

    // Batched decode attention: the longest run of consecutive segments with the same few rows (the scheduler puts the talking streams' rows behind the watching streams' chunks)
    if (s.nseg > 1 && table_ok && !sw.no_multi_attn && !s.dyn && m.attn_ws) {
        for (int j = 0; j < s.nseg;) {
            int k = j + 1;
            while (k < s.nseg && s.seg_rows[k] == s.seg_rows[j]) ++k;
            if (s.seg_rows[j] * (m.nh / m.nkv) <= STEP_MULTI_ATTN_Q_ROWS && k - j > p.run_n) { p.run0 = j; p.run_n = k - j; }
            j = k;
        }
        if (p.run_n < STEP_MULTI_ATTN_MIN_RUN || p.run_n > STEP_MULTI_ATTN_MAX_RUN || p.run_n * m.nkv > STEP_MULTI_ATTN_MAX_KV) p.run0 = p.run_n = 0;
    }
    p.run_all = p.run_n > 0 && p.run_n == s.nseg;

    // q / k / v prepared inside the attention kernel: the chain's steps and small rounds of talking streams only, while the qkv GEMM (as the step launches it; the chain's
    // consumer form does not change its split count) leaves no more slabs than the kernel sums
    if ((chain || (fused && p.run_all && S <= STEP_ROPE_FUSED_MULTI_ROWS)) && m.d == STEP_TABLE_HEAD_DIM && !sw.no_rope_fuse) {
        int sink = 0;
        GemmArgs a = step_slab_args(m, m.qkv_p, H, S, m.qkv_w, H);
        a.slabs_out = &sink; if (m.fp8) { a.Wp8 = step_stub(); a.wscale = (const float*)step_stub(); }
        p.rope_fused = gemm_plan(m.dtype, a, tune).slabs <= STEP_ROPE_FUSED_MAX_SLABS;
    }
    if (fused) return p;

    // ---- tile schedule ----
    p.chunk_rope = table_ok && S >= STEP_CHUNK_ROPE_MIN_ROWS && !sw.no_chunk_rope;
    // The last layer's hidden states are read at a few rows only: its o_proj and MLP run on those rows through the weight-streaming kernels.  (Not for the fused schedule: there
    // every GEMM is bound by the weights it streams, not by its rows -- the gate is `!fused`, not a row count.)
    p.sparse_last = s.n_need > 0 && s.n_need <= STEP_NEED_MAX && S > STEP_SPARSE_LAST_ABOVE && row_ok && !sw.full_last_layer && !s.hidden_out && !s.dyn &&
                    step_can_slab(m, step_slab_args(m, m.o_p, q_w, s.n_need, H, q_w), tune) && step_can_slab(m, step_slab_args(m, m.down_p, I, s.n_need, H, I), tune);
    // The SwiGLU product has ONE reader, down_proj: piece-major when the automatic dispatch runs gate_up on the plain ring and down_proj on the ring (every bf16 chunk of >= 512 rows)
    GemmArgs down = step_tile_args(m, m.down_p, I, true, H, S, H, I, EPI_RESID);
    if (!m.fp8 && !sw.no_pm) {
        const GemmArgs up = step_tile_args(m, m.gu_p, H, false, I, S, 2 * I, H, EPI_SWIGLU);
        p.mlp_pm = gemm_plan(m.dtype, up, tune).ring_auto == RING_AUTO_PLAIN && gemm_plan(m.dtype, down, tune).ring_auto != RING_AUTO_NONE;
    }
    // A split-K down_proj (long K, under one block wave of tiles: every chunk) leaves its fp32 slabs to ONE pass that sums them, adds the residual stream and normalises
    if (row_ok && !sw.no_slab_norm) {
        int sink = 0;
        down.ring_slabs_out = &sink; down.x_pm = p.mlp_pm ? 1 : 0; if (m.fp8) { down.Wp8 = step_stub(); down.wscale = (const float*)step_stub(); }
        p.down_slab_norm = gemm_plan(m.dtype, down, tune).ring_slabs > 1;
    }
    return p;
}
