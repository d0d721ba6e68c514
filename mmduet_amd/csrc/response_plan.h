// response_plan.h -- the state of a response in progress, and nothing else: the validated constraint set, the EOS rule, how the penalty list and the log-probability records
// grow, and what one returned token does to the counters.  Pure host functions: no GPU header, no runtime call, no environment; they compile with the host C++17 compiler
// alone (tests/test_response_plan_host.py walks tests/response_cases.py through them without a GPU).  Two owners share every rule here: the context, for the generate calls
// (mmd_greedy_generate / mmd_sample_generate), and a sampler, for its scheduler rounds (mmd_round_multi); model.hip's `Response` holds the buffers for either.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "../../include/mmduet.h"

// ---- the limits (include/mmduet.h states them; common.h sizes the device descriptors with them) ---------------------------
constexpr int CONS_MAX_TABLE = 256, CONS_MAX_EOS = 8;          // biased / suppressed ids and EOS ids of one constraint set
constexpr int LP_MAX_TOP = 8;                                  // alternatives of one log-probability record

// ---- constraints -------------------------------------------------------------------------------------------------------
// a validated constraint set on the host (DESIGN.md "Constraints"): the table sorted by id, ids unique
struct ConsSet { bool on = false; int n = 0, n_eos = 0, min_new = 0; int64_t eos[CONS_MAX_EOS] = {}; int32_t ids[CONS_MAX_TABLE] = {}; float bias[CONS_MAX_TABLE] = {}; };
struct ConsSetResult { int rc = MMD_OK; char error[192] = {0}; ConsSet set; };          // rc != MMD_OK: the set is refused with this message (the first failing check)
// limits checked when a set is given, not per token (include/mmduet.h): <= 8 EOS ids and <= 256 unique table ids, all in [0, V); bias finite or -inf; min_new >= 0; the
// suppressed ids and the EOS ids together must leave a token.  n_eos = min_new = n = 0 is "off".  The table is sorted by id for the kernel's binary search.
// (The native twin of mmduet_amd/constraints.py::merge.)
static inline ConsSetResult constraint_set(int V, const int64_t* eos_ids, int n_eos, int min_new, const int32_t* ids, const float* bias, int n) {
    ConsSetResult r;
#define CONS_REFUSE(...) do { r.rc = MMD_EINVAL; snprintf(r.error, sizeof(r.error), __VA_ARGS__); return r; } while (0)
    if (n_eos < 0 || n < 0 || (n_eos > 0 && !eos_ids) || (n > 0 && (!ids || !bias))) CONS_REFUSE("bad constraint arguments");
    if (n_eos > CONS_MAX_EOS) CONS_REFUSE("at most %d EOS ids, got %d", CONS_MAX_EOS, n_eos);
    if (n > CONS_MAX_TABLE) CONS_REFUSE("at most %d biased / suppressed ids, got %d", CONS_MAX_TABLE, n);
    if (min_new < 0) CONS_REFUSE("min_new_tokens %d is negative", min_new);
    ConsSet& s = r.set;
    for (int k = 0; k < n_eos; ++k) {
        if (eos_ids[k] < 0 || eos_ids[k] >= V) CONS_REFUSE("EOS id %lld outside the vocabulary of %d", (long long)eos_ids[k], V);
        s.eos[k] = eos_ids[k];
    }
    std::vector<std::pair<int32_t, float>> t((size_t)n);
    for (int k = 0; k < n; ++k) {
        if (ids[k] < 0 || ids[k] >= V) CONS_REFUSE("table id %d outside the vocabulary of %d", ids[k], V);
        if (bias[k] != bias[k] || bias[k] == INFINITY) CONS_REFUSE("the bias of id %d is %s: finite or -inf only", ids[k], bias[k] != bias[k] ? "NaN" : "+inf");
        t[k] = {ids[k], bias[k]};
    }
    std::sort(t.begin(), t.end(), [](const std::pair<int32_t, float>& a, const std::pair<int32_t, float>& b) { return a.first < b.first; });
    for (int k = 1; k < n; ++k) if (t[k].first == t[k - 1].first) CONS_REFUSE("table id %d is listed twice", t[k].first);
    long long covered = 0;
    for (int k = 0; k < n; ++k) { s.ids[k] = t[k].first; s.bias[k] = t[k].second; if (t[k].second == -INFINITY) ++covered; }
    for (int k = 0; k < n_eos; ++k) {
        bool dup = false;
        for (int j = 0; j < k; ++j) dup |= s.eos[j] == s.eos[k];
        for (int j = 0; j < n; ++j) dup |= s.ids[j] == s.eos[k] && s.bias[j] == -INFINITY;
        if (!dup) ++covered;
    }
    if ((n > 0 || n_eos > 0) && covered >= V) CONS_REFUSE("the suppressed ids and the EOS ids cover the whole vocabulary of %d: no token could be returned", V);
#undef CONS_REFUSE
    s.n = n; s.n_eos = n_eos; s.min_new = min_new; s.on = n > 0 || n_eos > 0 || min_new > 0;
    return r;
}

// ---- the EOS ids of a response -------------------------------------------------------------------------------------------
// the set's ids when it has any, otherwise the call's / sampler's own eos_id when it lies in [0, V), otherwise none.  The device descriptor (cons_fill_row, model.hip) is
// filled from the same answer, so the kernels' mask and the host's stop test cannot disagree.
struct ResponseEos { int n = 0; int64_t ids[CONS_MAX_EOS] = {}; };
static inline ResponseEos response_eos(const ConsSet& s, int64_t eos_id, int V) {
    ResponseEos e;
    if (s.n_eos > 0) { e.n = s.n_eos; for (int k = 0; k < s.n_eos; ++k) e.ids[k] = s.eos[k]; }
    else if (eos_id >= 0 && eos_id < V) { e.n = 1; e.ids[0] = eos_id; }
    return e;
}
static inline bool response_is_eos(const ResponseEos& e, int64_t tok) { for (int k = 0; k < e.n; ++k) if (e.ids[k] == tok) return true; return false; }

// ---- growth ----------------------------------------------------------------------------------------------------------------
// a buffer of `cap` entries that must hold `need`: unchanged when it does, otherwise doubled from its capacity (from `first` when there is none yet) until it does
static inline int grow_capacity(int cap, int need, int first) {
    if (need <= cap) return cap;
    int n = cap > 0 ? cap : first;
    while (n < need) n *= 2;
    return n;
}
// the first sizes.  The context's penalty list holds every id generated so far in the video and starts at MODEL_PREV_CAP (16384, model_plan.h: a workspace entry); a
// sampler's list holds one stream's.  The context's records are sized for a generate call's max_new, a sampler's for a response's
constexpr int RESPONSE_SAMPLER_PREV_FIRST = 1024, RESPONSE_CTX_RECORDS_FIRST = 1024, RESPONSE_SAMPLER_RECORDS_FIRST = 256;
// what the two owners reserve before a response: the list for the ids handed in plus every token it may return (a sampler: plus the slot behind the list, which receives
// every drawn token and counts only when the token is not EOS); the records for max_new tokens
static inline int generate_prev_need(int n_prev, int max_new) { return n_prev + max_new; }
static inline int sampler_prev_need(int n_prev, int max_new) { return n_prev + max_new + 1; }
static inline int sampler_records_need(int max_new) { return max_new > 0 ? max_new : 1; }

// ---- the counters ------------------------------------------------------------------------------------------------------------
struct ResponseCount {
    int step = 0;                      // tokens returned so far in this response
    int lp_n = 0;                      // records valid
    int n_prev = 0;                    // entries of the penalty list that count
    int max_new = 0;
    bool ended = false;                // EOS, or max_new tokens returned
};
// One token read back (models/modeling_live.py:66-72): EOS is neither fed back nor penalised, so it is neither appended nor counted; records count every token, EOS
// included; the response ends on EOS or with its max_new-th token.  -> the token joins the penalty list (as entry n_prev - 1).
// prev_cap: the list's capacity.  A generate call never reaches it: it reserves generate_prev_need() = n_prev + max_new entries and returns at most max_new tokens.  A
// sampler does when its rounds go on behind max_new tokens (nothing stops a caller; `ended` only reports): the list then stays at its capacity, the kernels append nothing.
static inline bool response_note_token(ResponseCount& r, bool is_eos, bool pen, bool record, int prev_cap) {
    r.step += 1;
    if (record) r.lp_n += 1;
    const bool joins = pen && !is_eos && r.n_prev < prev_cap;
    if (joins) r.n_prev += 1;
    if (is_eos || r.step >= r.max_new) r.ended = true;
    return joins;
}
