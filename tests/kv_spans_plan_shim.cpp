// C entries around kv_plan_spans() (mmduet_amd/csrc/kv_plan.h) for tests/test_kv_spans_host.py: built with the host C++ compiler alone, never part of the library.
#include "../mmduet_amd/csrc/kv_plan.h"
#include <string.h>

#define KVSP_CONSTANTS(F) F(KV_DROP) F(KV_OPS) F(KV_DROP_SPANS) F(KV_SPANS_PER_LAUNCH) F(KV_LAUNCH_NONE) F(KV_LAUNCH_DROP) F(KV_LAUNCH_DROP_SHIFT) F(KV_LAUNCH_COMPACT) \
    F(KV_LAUNCH_COMPACT_SHIFT) F(KV_F_SHIFT) F(MMD_OK) F(MMD_EINVAL) F(MMD_ERANGE)
#define F(name) #name,
static const char* const constant_names[] = { KVSP_CONSTANTS(F) };
#undef F
#define F(name) (long long)name,
static const long long constant_values[] = { KVSP_CONSTANTS(F) };
#undef F
extern "C" int kvsp_constants() { return (int)(sizeof(constant_names) / sizeof(constant_names[0])); }
extern "C" const char* kvsp_constant_name(int i) { return i >= 0 && i < kvsp_constants() ? constant_names[i] : ""; }
extern "C" long long kvsp_constant(int i) { return i >= 0 && i < kvsp_constants() ? constant_values[i] : 0; }

static KvGeom geom_of(const long long* geom) { KvGeom g; g.layers = (int)geom[0]; g.kv_heads = (int)geom[1]; g.head_dim = (int)geom[2]; g.elem_bytes = (int)geom[3]; return g; }
static KvState state_of(const long long* state) {
    KvState s; s.len = state[0]; s.pos_off = state[1]; s.cap = state[2]; s.mapped = state[3]; s.stash_from = state[4]; s.stash_to = state[5];
    return s;
}
static void message(char* err, int err_len, const char* text) { if (err_len > 0) { strncpy(err, text, (size_t)err_len - 1); err[err_len - 1] = 0; } }

// geom: {layers, kv_heads, head_dim, element bytes};  state: {len, pos_off, cap, mapped, stash_from, stash_to};  spans: [n][2] (null is passed on as it is)
// head: {rc, nothing, launch, pitch_bytes, spans, dropped, launches, after: len, pos_off, cap, mapped, stash_from, stash_to}
// launches: per launch KVSP_LAUNCH_WORDS values {dst0, len_in, len_end, nseg, (src, count) x KV_SPANS_PER_LAUNCH}, at most max_launches of them  -> launches planned
enum { KVSP_HEAD_WORDS = 13, KVSP_LAUNCH_WORDS = 4 + 2 * KV_SPANS_PER_LAUNCH };
extern "C" int kvsp_head_words() { return KVSP_HEAD_WORDS; }
extern "C" int kvsp_launch_words() { return KVSP_LAUNCH_WORDS; }
extern "C" int kvsp_plan(const long long* geom, const long long* state, const long long* spans, int n, int flags, long long* head, long long* launches, int max_launches, char* err,
                         int err_len) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the span list is passed on as it is");
    const KvSpansPlan p = kv_plan_spans(geom_of(geom), state_of(state), reinterpret_cast<const int64_t*>(spans), n, flags);
    const long long h[KVSP_HEAD_WORDS] = {p.rc, p.nothing, p.launch, p.pitch_bytes, p.spans, p.dropped, (long long)p.launches.size(), p.after.len, p.after.pos_off, p.after.cap, p.after.mapped,
                                          p.after.stash_from, p.after.stash_to};
    for (int i = 0; i < KVSP_HEAD_WORDS; ++i) head[i] = h[i];
    for (size_t l = 0; l < p.launches.size() && (int)l < max_launches; ++l) {
        const KvCompact& c = p.launches[l];
        long long* o = launches + l * KVSP_LAUNCH_WORDS;
        o[0] = c.dst0; o[1] = c.len_in; o[2] = c.len_end; o[3] = c.nseg;
        for (int i = 0; i < KV_SPANS_PER_LAUNCH; ++i) { o[4 + 2 * i] = i < c.nseg ? c.seg[i].src : 0; o[5 + 2 * i] = i < c.nseg ? c.seg[i].count : 0; }
    }
    message(err, err_len, p.error);
    return (int)p.launches.size();
}
// kv_plan(KV_DROP) over one span, to hold a one-span list against: out = {rc, nothing, launch, t0, t1, pitch_bytes, after_len, after_pos_off}
extern "C" void kvsp_drop(const long long* geom, const long long* state, long long a, long long b, int flags, long long* out, char* err, int err_len) {
    const KvPlan p = kv_plan(KV_DROP, geom_of(geom), state_of(state), a, b, nullptr, KV_BUF_OK, flags);
    const long long v[8] = {p.rc, p.nothing, p.launch, p.t0, p.t1, p.pitch_bytes, p.after.len, p.after.pos_off};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    message(err, err_len, p.error);
}
