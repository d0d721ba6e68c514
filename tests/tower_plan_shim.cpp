// C entry around tower_plan() / tower_projector_plan() (mmduet_amd/csrc/tower_plan.h) for tests/test_tower_plan_host.py: built with the host C++ compiler alone, never part of the library.
#include "../mmduet_amd/csrc/tower_plan.h"
#include <string.h>

// in: the fields below, in this order (the test reads the names from here: one list);  out: {rc, the TOWER_PLAN_FIELDS of the plan};  err: the refusal's message
#define TOWER_SHIM_FIELDS(F) F(dtype) F(tower_f16) F(C) F(heads) F(ipad) F(grid) F(tokens) F(seq) F(layers) F(pool_mode) F(pool_stride) F(class_token) F(pre_ln) F(post_ln) F(act) \
    F(vision_only) F(max_batch) F(fc1_p) F(fc2_p) F(ws_bytes) \
    F(B) F(for_pool) F(full_tower) F(ring_flags) F(ring_max_blocks) F(no_pm) F(ksplit_short)
#define F(name) IN_##name,
enum { TOWER_SHIM_FIELDS(F) IN_COUNT };
#undef F
#define F(name) #name,
static const char* const field_names[] = { TOWER_SHIM_FIELDS(F) };
#undef F
static TowerModel model_of(const long long* in) {
    TowerModel m;
    m.dtype = (int)in[IN_dtype]; m.tower_f16 = (int)in[IN_tower_f16]; m.C = (int)in[IN_C]; m.heads = (int)in[IN_heads]; m.ipad = (int)in[IN_ipad]; m.grid = (int)in[IN_grid];
    m.tokens = (int)in[IN_tokens]; m.seq = (int)in[IN_seq]; m.layers = (int)in[IN_layers]; m.pool_mode = (int)in[IN_pool_mode]; m.pool_stride = (int)in[IN_pool_stride];
    m.class_token = in[IN_class_token] != 0; m.pre_ln = in[IN_pre_ln] != 0; m.post_ln = in[IN_post_ln] != 0; m.act = (int)in[IN_act]; m.vision_only = in[IN_vision_only] != 0;
    m.max_batch = (int)in[IN_max_batch]; m.fc1_p = in[IN_fc1_p] != 0; m.fc2_p = in[IN_fc2_p] != 0; m.splitk_ws_bytes = (size_t)in[IN_ws_bytes];
    return m;
}
extern "C" int tower_plan_shim_fields() { return IN_COUNT; }
extern "C" const char* tower_plan_shim_field_name(int i) { return i >= 0 && i < IN_COUNT ? field_names[i] : ""; }
extern "C" int tower_plan_shim_outputs() { return 1 + TOWER_PLAN_FIELDS; }
extern "C" void tower_plan_shim(const long long* in, int* out, char* err, int err_len) {
    TowerShape s;
    s.B = (int)in[IN_B]; s.for_pool = in[IN_for_pool] != 0; s.full_tower = in[IN_full_tower] != 0; s.ring_flags = (int)in[IN_ring_flags]; s.ring_max_blocks = (int)in[IN_ring_max_blocks];
    GemmTuning tune; tune.gemv_ksplit_short = (int)in[IN_ksplit_short];
    const TowerPlan p = tower_plan(model_of(in), s, in[IN_no_pm] != 0, tune);
    out[0] = p.rc; p.fields(out + 1);
    if (err_len > 0) { strncpy(err, p.error, (size_t)err_len - 1); err[err_len - 1] = 0; }
}
// out3 = {compact, gather, pout}
extern "C" void tower_projector_plan_shim(const long long* in, int all_tokens, int tower_left_compact, int* out3) {
    const TowerProjectorPlan p = tower_projector_plan(model_of(in), all_tokens != 0, tower_left_compact != 0);
    out3[0] = p.compact; out3[1] = p.gather; out3[2] = p.pout;
}
// the named thresholds, for the table's boundary rows: {TOWER_POOL_TAPS, TOWER_HALF_MIN_QUERIES, TOWER_HALF_GEMM_ABOVE}
extern "C" void tower_plan_shim_constants(int* out3) { out3[0] = TOWER_POOL_TAPS; out3[1] = TOWER_HALF_MIN_QUERIES; out3[2] = TOWER_HALF_GEMM_ABOVE; }
