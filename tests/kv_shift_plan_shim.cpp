// C entries around kv_plan() with its flags (mmduet_amd/csrc/kv_plan.h) for tests/test_kv_shift_host.py: built with the host C++ compiler alone, never part of the library.
#include "../mmduet_amd/csrc/kv_plan.h"
#include <string.h>

// what a plan reports, in this order (the test reads the names from here)
#define KVS_FIELDS(F) F(nothing, p.nothing) F(reserve, p.reserve) F(stash_bytes, p.stash_bytes) F(launch, p.launch) F(k_off, p.k_off) F(k_bytes, p.k_bytes) F(v_off, p.v_off) \
    F(v_bytes, p.v_bytes) F(k_cols, p.k_cols) F(v_cols, p.v_cols) F(pitch4, p.pitch4) F(k_other4, p.k_other4) F(v_other4, p.v_other4) F(copy_rows, p.copy_rows) F(t0, p.t0) F(t1, p.t1) \
    F(pitch_bytes, p.pitch_bytes) F(after_len, p.after.len) F(after_pos_off, p.after.pos_off) F(after_cap, p.after.cap) F(after_mapped, p.after.mapped) \
    F(after_stash_from, p.after.stash_from) F(after_stash_to, p.after.stash_to)
#define F(name, expr) #name,
static const char* const field_names[] = { KVS_FIELDS(F) };
#undef F
#define KVS_CONSTANTS(F) F(KV_DROP) F(KV_OPS) F(KV_LAUNCH_NONE) F(KV_LAUNCH_DROP) F(KV_CANON_SCATTER) F(KV_LAUNCH_DROP_SHIFT) F(KV_F_SHIFT) F(MMD_OK) F(MMD_EINVAL) F(MMD_ERANGE)
#define F(name) #name,
static const char* const constant_names[] = { KVS_CONSTANTS(F) };
#undef F
#define F(name) (long long)name,
static const long long constant_values[] = { KVS_CONSTANTS(F) };
#undef F
extern "C" int kvs_fields() { return (int)(sizeof(field_names) / sizeof(field_names[0])); }
extern "C" const char* kvs_field_name(int i) { return i >= 0 && i < kvs_fields() ? field_names[i] : ""; }
extern "C" int kvs_constants() { return (int)(sizeof(constant_names) / sizeof(constant_names[0])); }
extern "C" const char* kvs_constant_name(int i) { return i >= 0 && i < kvs_constants() ? constant_names[i] : ""; }
extern "C" long long kvs_constant(int i) { return i >= 0 && i < kvs_constants() ? constant_values[i] : 0; }

// geom: {layers, kv_heads, head_dim, element bytes};  state: {len, pos_off, cap, mapped, stash_from, stash_to};  flags < 0: kv_plan is called WITHOUT the trailing argument
// out: {rc, the fields above};  err: the refusal's message
extern "C" void kvs_plan(int op, const long long* geom, const long long* state, long long a, long long b, int flags, long long* out, char* err, int err_len) {
    KvGeom g; g.layers = (int)geom[0]; g.kv_heads = (int)geom[1]; g.head_dim = (int)geom[2]; g.elem_bytes = (int)geom[3];
    KvState s; s.len = state[0]; s.pos_off = state[1]; s.cap = state[2]; s.mapped = state[3]; s.stash_from = state[4]; s.stash_to = state[5];
    const KvPlan p = flags < 0 ? kv_plan(op, g, s, a, b, nullptr, KV_BUF_OK) : kv_plan(op, g, s, a, b, nullptr, KV_BUF_OK, flags);
    out[0] = p.rc;
#define F(name, expr) (long long)(expr),
    const long long v[] = { KVS_FIELDS(F) };
#undef F
    for (int i = 0; i < kvs_fields(); ++i) out[1 + i] = v[i];
    if (err_len > 0) { strncpy(err, p.error, (size_t)err_len - 1); err[err_len - 1] = 0; }
}
