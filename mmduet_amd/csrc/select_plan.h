// select_plan.h -- how logits rows become tokens, and nothing else.  Three pure host functions: no GPU header, no runtime call, no environment; they compile with the host
// C++17 compiler alone (tests/test_select_plan_host.py runs the table of tests/select_regimes.py through them without a GPU).
//   select_plan()    one block of logits rows: which kernels choose the tokens, what they read, what follows them.  select_enqueue (model.hip) launches what it says.
//   generate_plan()  what a generate call decides once, behind its first token: captured or eager steps, which descriptors are posted when, who grows the penalty list,
//                    the key of the captured step.
//   round_blocks()   the sampling segments of a scheduler round ordered into its three blocks of logits rows, each block's recording rows as its tail.
// mmd_op_select_last_plan reads the answers back.  What a response in progress owns -- the constraint set and its limits, the EOS ids it stops on, how its penalty list and
// records grow, what a token read back does to its counters -- is response_plan.h's, not decided here.
#pragma once
#include <stdio.h>
#include "step_plan.h"

// ---- the thresholds ------------------------------------------------------------------------------------------------
constexpr int SELECT_MAX_V = 1 << 18;             // the chain's kernels (scores, filters, records) index a row's slices up to this vocabulary
constexpr int SELECT_ROUND_MAX_ROWS = 32;         // rows of one launch, sampling segments of one round (MMD_ROUND_MAX_SAMPLERS of common.h: model.hip asserts the two agree)
//            STEP_ROW_MAX_H, STEP_TABLE_HEAD_DIM (step_plan.h): the captured step is the fused schedule's, its attention kernel reads *dyn at head_dim 128

// ---- one block of logits rows --------------------------------------------------------------------------------------------
struct SelectRows {
    bool sampled = false;              // a draw (temperature / top-k / top-p) stands where the arg-max stood
    bool constrained = false;          // the rows have constraint descriptors
    bool record = false;               // log-probability records are written
    int n = 1;                         // rows
    bool single = false;               // the context's one-row generate path (logits_ws, row / constraint descriptor 0, tok_dev), not a multi-row block
    bool dyn = false;                  // the step is being captured into the decode graph
    int V = 0, top_k = 0; float top_p = 1.f;
};
enum { SEL_ARGMAX = 0,                 // penalty + arg-max over the raw logits (single: the two-stage kernel; a block: the batched one)
       SEL_CONS_ARGMAX = 1,            // the chain's scores with nothing filtered, then their first maximal index
       SEL_DRAW = 2 };                 // the sampling chain
constexpr int SELECT_PLAN_FIELDS = 10;
struct SelectPlan {
    int rc = MMD_OK; const char* error = nullptr;          // rc != MMD_OK: the arguments are refused with this message
    int kind = SEL_ARGMAX;
    bool single = false;
    bool any_k = false, any_p = false; // SEL_DRAW: which of the chain's filter kernels the launch needs
    bool needs_row = false;            // the launches read SampleRow descriptors
    bool needs_cons = false;           // ... and ConstraintRow descriptors
    bool record = false;               // launch_logprob_rows follows the choice
    bool scores_after_argmax = false;  // SEL_ARGMAX with records: the unfiltered scores run behind the arg-max, for the record alone
    bool record_greedy = false;        // the record's sampling_logprob comes from the unfiltered scores (the `greedy` flag of launch_logprob_rows)
    bool advance = false;              // a single step: launch_advance_state follows (the state the next step reads lives on the device)
    void fields(int* out) const {      // what mmd_op_select_last_plan reports
        const int v[SELECT_PLAN_FIELDS] = {kind, single, any_k, any_p, needs_row, needs_cons, record, scores_after_argmax, record_greedy, advance};
        for (int i = 0; i < SELECT_PLAN_FIELDS; ++i) out[i] = v[i];
    }
};
static inline SelectPlan select_plan(const SelectRows& r) {
    SelectPlan p;
    if (r.V > SELECT_MAX_V) {
        p.rc = MMD_ERANGE;
        if (r.sampled) { p.error = "sampling handles vocabularies up to 2^18 entries"; return p; }
        if (r.constrained) { p.error = "constraints handle vocabularies up to 2^18 entries"; return p; }
        if (r.record) { p.error = "log-probabilities handle vocabularies up to 2^18 entries"; return p; }
        p.rc = MMD_OK;
    }
    p.kind = r.sampled ? SEL_DRAW : r.constrained ? SEL_CONS_ARGMAX : SEL_ARGMAX;
    p.single = r.single;
    p.any_k = r.sampled && r.top_k > 0 && r.top_k < r.V;
    p.any_p = r.sampled && r.top_p < 1.f;
    p.needs_row = r.sampled || r.record || r.constrained;
    p.needs_cons = r.constrained;
    p.record = r.record;
    p.scores_after_argmax = p.kind == SEL_ARGMAX && r.record;
    p.record_greedy = r.record && !r.sampled;
    p.advance = r.single && (r.sampled || r.dyn);          // the sampled step reads the penalty list's length through *step_dev on the eager route too
    return p;
}

// ---- one generate call, behind its first token -------------------------------------------------------------------------
struct GraphGate {                     // what the captured step asks of the context
    bool no_graph = false;             // MMDUET_GRAPH=0 / mmd_set_graph
    bool no_fuse = false;              // MMDUET_NO_FUSE=1: no fused schedule to capture
    bool prof_on = false;              // per-kernel timing wants the launches one by one
    int dtype = MMD_BF16;
    bool qkv_p = false;                // the packed qkv matrix exists (the weight-streaming GEMVs)
    int H = 0, d = 0;
};
struct GenerateShape {
    bool sampled = false, constrained = false, record = false;
    bool pen = false;                  // repetition penalty on
    int max_new = 0;
    bool first_is_eos = false;         // the prompt step's token ended the response
    int V = 0, top_k = 0; float top_p = 1.f;
    int lp_top = -1;                   // alternatives per record (keys the captured step)
    unsigned cons_gen = 0;             // generation of the context's constraint set (on <-> off)
    GraphGate gate;
};
constexpr int GENERATE_PLAN_FIELDS = 11;
struct GeneratePlan {
    bool can_graph = false;            // steps 1.. replay one captured step
    bool upload_state = false;         // StepState goes to the device before step 1
    // Row descriptor 0 (the draw's row when sampled, else the arg-max's T = 1 row; the prompt step's SelectPlan::needs_row posts the static form before the prompt's choice):
    bool post_row_dynamic = false;     //   once before step 1, reading the list length through &step_dev->n_prev
    bool post_row_each_eager_step = false;     //   before every eager step, the list length in the descriptor
    bool post_cons_dynamic = false;    // constraint descriptor 0 likewise: once, reading the step through &step_dev->step ...
    bool post_cons_each_eager_step = false;    //   ... or before every eager step with the step's number
    bool host_appends_penalty = false; // steps 1..: the host copies the token behind the list (otherwise advance_state_kernel grows it).  The prompt's token is always the host's
    bool pen_key_is_value = false;     // the captured step's penalty key: the value itself (it rides in a kernel argument) or on / off (the value is in the row descriptor)
    int key_sel = 0, key_lp = -1; unsigned key_cons_gen = 0;          // ... and: the filter kernels (any_k | any_p << 1), the records' top_n, the constraint generation
    void fields(int* out) const {
        const int v[GENERATE_PLAN_FIELDS] = {can_graph, upload_state, post_row_dynamic, post_row_each_eager_step, post_cons_dynamic, post_cons_each_eager_step, host_appends_penalty,
                                             pen_key_is_value, key_sel, key_lp, (int)key_cons_gen};
        for (int i = 0; i < GENERATE_PLAN_FIELDS; ++i) out[i] = v[i];
    }
};
static inline GeneratePlan generate_plan(const GenerateShape& s) {
    GeneratePlan p;
    const GraphGate& g = s.gate;
    const bool more = !s.first_is_eos && s.max_new > 1;
    // bf16 + fused schedule: replay a captured hipGraph of the whole step (~255 kernels of 5-50 us) instead of pacing it by host launch latency
    p.can_graph = more && !g.no_graph && !g.no_fuse && !g.prof_on && g.dtype == MMD_BF16 && g.qkv_p && g.H <= STEP_ROW_MAX_H && g.d == STEP_TABLE_HEAD_DIM;
    const bool on_device = p.can_graph || (s.sampled && more);          // the steps read position / list length / step from *step_dev
    p.upload_state = on_device;
    p.post_row_dynamic = s.sampled ? more : (s.record || s.constrained) && p.can_graph;
    p.post_row_each_eager_step = more && !s.sampled && (s.record || s.constrained) && !p.can_graph;
    p.post_cons_dynamic = s.constrained && on_device;
    p.post_cons_each_eager_step = more && s.constrained && !on_device;
    p.host_appends_penalty = more && s.pen && !on_device;
    p.pen_key_is_value = !s.sampled;
    SelectRows r; r.sampled = s.sampled; r.V = s.V; r.top_k = s.top_k; r.top_p = s.top_p;
    const SelectPlan sel = select_plan(r);
    p.key_sel = (sel.any_k ? 1 : 0) | (sel.any_p ? 2 : 0);
    p.key_lp = s.record ? s.lp_top : -1;
    p.key_cons_gen = s.constrained ? s.cons_gen : 0;
    return p;
}

// ---- the sampling segments of a round -------------------------------------------------------------------------------------
struct RoundSeg {
    bool feed = false, sample = false; // MMD_SEG_FEED, MMD_SEG_SAMPLE
    bool sampling = false;             // the segment's sampler draws (mmd_sampler_set_sampling)
    bool constrained = false;          // ... has constraints on
    int rows = 1;
    int sampler = -1;                  // which sampler, as an index into the caller's own array (two segments with the same sampler carry the same index)
    int top_k = 0; float top_p = 1.f;
    bool record = false;               // the segment's sampler records log-probabilities (mmd_sampler_set_logprobs) ...
    int lp_top = -1;                   // ... with this many alternatives
};
constexpr int ROUND_BLOCKS_FIELDS = 6;
constexpr int ROUND_RECORD_FIELDS = 4;
struct RoundBlocks {
    int rc = MMD_OK; char error[96] = {0};
    int order[SELECT_ROUND_MAX_ROWS] = {0};          // the sampling segments in the order of their logits rows: plain arg-max | constrained arg-max | sampled; inside a block the
                                                     // rows that record nothing first, the recording ones last, each group in segment order
    int n_plain = 0, n_greedy = 0, n_sample = 0;          // rows [0, n_plain) | [n_plain, n_greedy) | [n_greedy, n_sample)
    bool any_k = false, any_p = false; // over the sampled block
    bool any_cons_sampled = false;     // a sampled row is constrained: the block's launch takes constraint descriptors (empty ones for the other rows)
    int V = 0;
    int rec0[3] = {0, 0, 0};           // per kind: the block's recording rows are its tail [rec0[kind], row0(kind) + rows(kind)); an empty tail starts at the block's end
    int lp_top_max = -1;               // the largest lp_top among the recording rows (-1: no row records)
    void fields(int* out) const {
        const int v[ROUND_BLOCKS_FIELDS] = {n_plain, n_greedy, n_sample, any_k, any_p, any_cons_sampled};
        for (int i = 0; i < ROUND_BLOCKS_FIELDS; ++i) out[i] = v[i];
    }
    int row0(int kind) const { return kind == SEL_ARGMAX ? 0 : kind == SEL_CONS_ARGMAX ? n_plain : n_greedy; }
    int rows(int kind) const { return kind == SEL_ARGMAX ? n_plain : kind == SEL_CONS_ARGMAX ? n_greedy - n_plain : n_sample - n_greedy; }
    int rec_rows(int kind) const { return row0(kind) + rows(kind) - rec0[kind]; }
    void record_fields(int* out) const {          // what mmd_op_round_last_record reports: recording rows per block, the largest top_n
        const int v[ROUND_RECORD_FIELDS] = {rec_rows(SEL_ARGMAX), rec_rows(SEL_CONS_ARGMAX), rec_rows(SEL_DRAW), lp_top_max};
        for (int i = 0; i < ROUND_RECORD_FIELDS; ++i) out[i] = v[i];
    }
    // the launches of one block: the filters any of its rows needs, constraint descriptors when any sampled row has a set, the record's launches (over the tail alone) when
    // the block has a tail
    SelectPlan plan(int kind) const {
        SelectRows r;
        r.sampled = kind == SEL_DRAW; r.constrained = kind == SEL_CONS_ARGMAX || (kind == SEL_DRAW && any_cons_sampled); r.n = rows(kind); r.V = V;
        r.record = rec_rows(kind) > 0;
        SelectPlan p = select_plan(r);
        if (kind == SEL_DRAW) { p.any_k = any_k; p.any_p = any_p; }
        return p;
    }
};
static inline int round_kind(const RoundSeg& s) { return s.sampling ? SEL_DRAW : s.constrained ? SEL_CONS_ARGMAX : SEL_ARGMAX; }
static inline RoundBlocks round_blocks(const RoundSeg* segs, int n, int V) {
    RoundBlocks b; b.V = V;
    int count[3] = {0, 0, 0}, quiet[3] = {0, 0, 0}, seen[SELECT_ROUND_MAX_ROWS], total = 0;
    for (int j = 0; j < n; ++j) {
        const RoundSeg& s = segs[j];
        if (s.feed && s.rows != 1) { b.rc = MMD_EINVAL; snprintf(b.error, sizeof(b.error), "a feed segment is one row (segment %d has %d)", j, s.rows); return b; }
        if (!s.sample) continue;
        if (total >= SELECT_ROUND_MAX_ROWS) { b.rc = MMD_ERANGE; snprintf(b.error, sizeof(b.error), "more than %d sampling segments", SELECT_ROUND_MAX_ROWS); return b; }
        for (int k = 0; k < total; ++k) if (seen[k] == s.sampler) { b.rc = MMD_EINVAL; snprintf(b.error, sizeof(b.error), "a sampler may appear once per round"); return b; }
        seen[total++] = s.sampler; ++count[round_kind(s)];
        if (!s.record) ++quiet[round_kind(s)];
    }
    int at[3] = {0, count[SEL_ARGMAX], count[SEL_ARGMAX] + count[SEL_CONS_ARGMAX]};          // where the next row that records nothing goes ...
    b.n_plain = at[SEL_CONS_ARGMAX]; b.n_greedy = at[SEL_DRAW]; b.n_sample = total;
    for (int k = 0; k < 3; ++k) b.rec0[k] = at[k] + quiet[k];
    int rec_at[3] = {b.rec0[0], b.rec0[1], b.rec0[2]};          // ... and the next recording one
    for (int j = 0; j < n; ++j) {
        const RoundSeg& s = segs[j];
        if (!s.sample) continue;
        if (s.record) { b.order[rec_at[round_kind(s)]++] = j; if (s.lp_top > b.lp_top_max) b.lp_top_max = s.lp_top; }
        else b.order[at[round_kind(s)]++] = j;
        if (!s.sampling) continue;
        SelectRows r; r.sampled = true; r.V = V; r.top_k = s.top_k; r.top_p = s.top_p;
        const SelectPlan p = select_plan(r);
        b.any_k |= p.any_k; b.any_p |= p.any_p; b.any_cons_sampled |= s.constrained;
    }
    return b;
}
