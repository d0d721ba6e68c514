// C entry around step_plan() (mmduet_amd/csrc/step_plan.h) for tests/test_step_plan_host.py: built with the host C++ compiler alone, never part of the library.
#include "../mmduet_amd/csrc/step_plan.h"
#include <string.h>

// in: the fields below, in this order (the test reads the names from here: one list);  seg_rows: IN_NSEG row counts;  out: {rc, the STEP_PLAN_FIELDS of the plan};  err: the refusal's message
#define STEP_SHIM_FIELDS(F) F(DTYPE) F(H) F(I) F(NH) F(NKV) F(D) F(QKV_W) F(LAYERS) F(QKV_P) F(O_P) F(GU_P) F(DOWN_P) F(FP8) F(ATTN_WS) F(WS_BYTES) \
    F(S) F(NSEG) F(N_NEED) F(HIDDEN_OUT) F(DYN) F(KSPLIT_SHORT) \
    F(NO_FUSE) F(NO_PM) F(NO_CHAIN) F(NO_SLAB_NORM) F(FULL_LAST_LAYER) F(NO_ROPE_FUSE) F(NO_MULTI_FUSE) F(NO_MULTI_ATTN) F(NO_CHUNK_ROPE)
#define F(name) IN_##name,
enum { STEP_SHIM_FIELDS(F) IN_COUNT };
#undef F
#define F(name) #name,
static const char* const field_names[] = { STEP_SHIM_FIELDS(F) };
#undef F
extern "C" int step_plan_shim_fields() { return IN_COUNT; }
extern "C" const char* step_plan_shim_field_name(int i) { return i >= 0 && i < IN_COUNT ? field_names[i] : ""; }
extern "C" int step_plan_shim_outputs() { return 1 + STEP_PLAN_FIELDS; }
extern "C" void step_plan_shim(const long long* in, const int* seg_rows, int* out, char* err, int err_len) {
    StepModel m;
    m.dtype = (int)in[IN_DTYPE]; m.H = (int)in[IN_H]; m.I = (int)in[IN_I]; m.nh = (int)in[IN_NH]; m.nkv = (int)in[IN_NKV]; m.d = (int)in[IN_D]; m.qkv_w = (int)in[IN_QKV_W];
    m.layers = (int)in[IN_LAYERS]; m.qkv_p = in[IN_QKV_P] != 0; m.o_p = in[IN_O_P] != 0; m.gu_p = in[IN_GU_P] != 0; m.down_p = in[IN_DOWN_P] != 0; m.fp8 = in[IN_FP8] != 0;
    m.attn_ws = in[IN_ATTN_WS] != 0; m.splitk_ws_bytes = (size_t)in[IN_WS_BYTES];
    StepShape s;
    s.S = (int)in[IN_S]; s.seg_rows = seg_rows; s.nseg = (int)in[IN_NSEG]; s.n_need = (int)in[IN_N_NEED]; s.hidden_out = in[IN_HIDDEN_OUT] != 0; s.dyn = in[IN_DYN] != 0;
    StepSwitches sw;
    sw.no_fuse = in[IN_NO_FUSE] != 0; sw.no_pm = in[IN_NO_PM] != 0; sw.no_chain = in[IN_NO_CHAIN] != 0; sw.no_slab_norm = in[IN_NO_SLAB_NORM] != 0;
    sw.full_last_layer = in[IN_FULL_LAST_LAYER] != 0; sw.no_rope_fuse = in[IN_NO_ROPE_FUSE] != 0; sw.no_multi_fuse = in[IN_NO_MULTI_FUSE] != 0;
    sw.no_multi_attn = in[IN_NO_MULTI_ATTN] != 0; sw.no_chunk_rope = in[IN_NO_CHUNK_ROPE] != 0;
    GemmTuning tune; tune.gemv_ksplit_short = (int)in[IN_KSPLIT_SHORT];
    const StepPlan p = step_plan(m, s, sw, tune);
    out[0] = p.rc; p.fields(out + 1);
    if (err_len > 0) { strncpy(err, p.error ? p.error : "", (size_t)err_len - 1); err[err_len - 1] = 0; }
}
