// C entries around kv_plan() and the growth functions (mmduet_amd/csrc/kv_plan.h) for tests/test_kv_plan_host.py: built with the host C++ compiler alone, never part of the
// library.
#include "../mmduet_amd/csrc/kv_plan.h"
#include <string.h>

// what a plan reports, in this order (the test reads the names from here: one list)
#define KV_SHIM_FIELDS(F) F(nothing, p.nothing) F(reserve, p.reserve) F(stash_bytes, p.stash_bytes) F(launch, p.launch) F(k_off, p.k_off) F(k_bytes, p.k_bytes) F(v_off, p.v_off) \
    F(v_bytes, p.v_bytes) F(k_cols, p.k_cols) F(v_cols, p.v_cols) F(pitch4, p.pitch4) F(k_other4, p.k_other4) F(v_other4, p.v_other4) F(copy_rows, p.copy_rows) F(t0, p.t0) F(t1, p.t1) \
    F(pitch_bytes, p.pitch_bytes) F(after_len, p.after.len) F(after_pos_off, p.after.pos_off) F(after_cap, p.after.cap) F(after_mapped, p.after.mapped) \
    F(after_stash_from, p.after.stash_from) F(after_stash_to, p.after.stash_to)
#define F(name, expr) #name,
static const char* const field_names[] = { KV_SHIM_FIELDS(F) };
#undef F
// the enums, by name, so that the table's own numbers can be checked against the header's
#define KV_SHIM_CONSTANTS(F) F(KV_TRUNCATE) F(KV_RESET) F(KV_STASH) F(KV_UNSTASH) F(KV_DROP) F(KV_EXPORT) F(KV_IMPORT) F(KV_SET_POSITION) F(KV_FORK) F(KV_DEBUG_SET_LEN) F(KV_DEBUG_READ) \
    F(KV_OPS) F(KV_BUF_OK) F(KV_BUF_MISSING) F(KV_BUF_MISALIGNED) F(KV_LAUNCH_NONE) F(KV_ROWS_OUT) F(KV_ROWS_IN) F(KV_LAUNCH_DROP) F(KV_CANON_GATHER) F(KV_CANON_SCATTER) \
    F(KV_MAX_RESERVATIONS) F(KV_VIRTUAL_TOKENS_DEFAULT)
#define F(name) #name,
static const char* const constant_names[] = { KV_SHIM_CONSTANTS(F) };
#undef F
#define F(name) (long long)name,
static const long long constant_values[] = { KV_SHIM_CONSTANTS(F) };
#undef F
extern "C" int kv_shim_fields() { return (int)(sizeof(field_names) / sizeof(field_names[0])); }
extern "C" const char* kv_shim_field_name(int i) { return i >= 0 && i < kv_shim_fields() ? field_names[i] : ""; }
extern "C" int kv_shim_constants() { return (int)(sizeof(constant_names) / sizeof(constant_names[0])); }
extern "C" const char* kv_shim_constant_name(int i) { return i >= 0 && i < kv_shim_constants() ? constant_names[i] : ""; }
extern "C" long long kv_shim_constant(int i) { return i >= 0 && i < kv_shim_constants() ? constant_values[i] : 0; }

static KvGeom geom_of(const long long* g) { KvGeom k; k.layers = (int)g[0]; k.kv_heads = (int)g[1]; k.head_dim = (int)g[2]; k.elem_bytes = (int)g[3]; return k; }
static KvState state_of(const long long* s) { KvState k; k.len = s[0]; k.pos_off = s[1]; k.cap = s[2]; k.mapped = s[3]; k.stash_from = s[4]; k.stash_to = s[5]; return k; }

// geom: {layers, kv_heads, head_dim, element bytes};  out: {BLK, tok_bytes, rows, pitch_bytes(cap), layer_bytes(cap), arena_bytes(cap)}
extern "C" void kv_geom_shim(const long long* geom, long long cap, long long* out) {
    const KvGeom g = geom_of(geom);
    const long long v[6] = {(long long)KvGeom::BLK, (long long)g.tok_bytes(), (long long)g.rows(), (long long)g.pitch_bytes(cap), (long long)g.layer_bytes(cap), (long long)g.arena_bytes(cap)};
    for (int i = 0; i < 6; ++i) out[i] = v[i];
}
// state, src: {len, pos_off, cap, mapped, stash_from, stash_to} (src: null unless the op is a fork);  out: {rc, the fields above};  err: the refusal's message
extern "C" void kv_plan_shim(int op, const long long* geom, const long long* state, long long a, long long b, const long long* src, int bufs, long long* out, char* err, int err_len) {
    KvState from; if (src) from = state_of(src);
    const KvPlan p = kv_plan(op, geom_of(geom), state_of(state), a, b, src ? &from : nullptr, bufs);
    out[0] = p.rc;
#define F(name, expr) (long long)(expr),
    const long long v[] = { KV_SHIM_FIELDS(F) };
#undef F
    for (int i = 0; i < kv_shim_fields(); ++i) out[1 + i] = v[i];
    if (err_len > 0) { strncpy(err, p.error, (size_t)err_len - 1); err[err_len - 1] = 0; }
}
extern "C" long long kv_initial_tokens_shim(long long asked) { return kv_initial_tokens(asked); }
extern "C" long long kv_vmm_chunk_tokens_shim(long long tok_bytes, long long granularity) { return kv_vmm_chunk_tokens((size_t)tok_bytes, (size_t)granularity); }
// out: room for KV_MAX_RESERVATIONS;  -> how many were written
extern "C" int kv_vmm_reservations_shim(long long initial_tokens, long long requested, long long chunk, long long* out) {
    int64_t tries[KV_MAX_RESERVATIONS];
    const int n = kv_vmm_reservations(initial_tokens, requested, chunk, tries);
    for (int i = 0; i < n; ++i) out[i] = tries[i];
    return n;
}
// out: {the doubling, the second try, the bytes of a row the reallocation carries over for a context of `len` tokens}
extern "C" void kv_grow_shim(const long long* geom, long long cap, long long need, long long len, long long* out) {
    out[0] = kv_grow_doubled(cap, need); out[1] = kv_grow_exact(need); out[2] = (long long)kv_grow_copy_bytes(geom_of(geom), len);
}
