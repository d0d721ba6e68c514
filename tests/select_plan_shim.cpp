// C entries around select_plan() / generate_plan() / round_blocks() (mmduet_amd/csrc/select_plan.h) for tests/test_select_plan_host.py: built with the host C++ compiler
// alone, never part of the library.
#include "../mmduet_amd/csrc/select_plan.h"
#include <string.h>

// the integer inputs of each entry, in this order (the test reads the names from here: one list); top_p travels beside them as a double
#define SELECT_SHIM_FIELDS(F) F(SAMPLED) F(CONSTRAINED) F(RECORD) F(N) F(SINGLE) F(DYN) F(V) F(TOP_K)
#define GENERATE_SHIM_FIELDS(F) F(SAMPLED) F(CONSTRAINED) F(RECORD) F(PEN) F(MAX_NEW) F(FIRST_IS_EOS) F(V) F(TOP_K) F(LP_TOP) F(CONS_GEN) \
    F(NO_GRAPH) F(NO_FUSE) F(PROF_ON) F(DTYPE) F(QKV_P) F(H) F(D)
#define ROUND_SHIM_FIELDS(F) F(FEED) F(SAMPLE) F(SAMPLING) F(CONSTRAINED) F(ROWS) F(SAMPLER) F(TOP_K)
#define F(name) S_##name,
enum { SELECT_SHIM_FIELDS(F) S_COUNT };
#undef F
#define F(name) G_##name,
enum { GENERATE_SHIM_FIELDS(F) G_COUNT };
#undef F
#define F(name) R_##name,
enum { ROUND_SHIM_FIELDS(F) R_COUNT };
#undef F
#define F(name) #name,
static const char* const select_names[] = { SELECT_SHIM_FIELDS(F) };
static const char* const generate_names[] = { GENERATE_SHIM_FIELDS(F) };
static const char* const round_names[] = { ROUND_SHIM_FIELDS(F) };
#undef F
// which: 0 select, 1 generate, 2 round
extern "C" int select_shim_fields(int which) { return which == 0 ? (int)S_COUNT : which == 1 ? (int)G_COUNT : (int)R_COUNT; }
extern "C" const char* select_shim_field_name(int which, int i) {
    if (i < 0 || i >= select_shim_fields(which)) return "";
    return which == 0 ? select_names[i] : which == 1 ? generate_names[i] : round_names[i];
}
extern "C" int select_shim_outputs(int which) { return which == 0 ? SELECT_PLAN_FIELDS : which == 1 ? GENERATE_PLAN_FIELDS : ROUND_BLOCKS_FIELDS; }
extern "C" int select_shim_round_max() { return SELECT_ROUND_MAX_ROWS; }
static void put_error(char* err, int err_len, const char* msg) { if (err_len > 0) { strncpy(err, msg ? msg : "", (size_t)err_len - 1); err[err_len - 1] = 0; } }

// out: {rc, the SELECT_PLAN_FIELDS};  err: the refusal's message
extern "C" void select_plan_shim(const long long* in, double top_p, int* out, char* err, int err_len) {
    SelectRows r;
    r.sampled = in[S_SAMPLED] != 0; r.constrained = in[S_CONSTRAINED] != 0; r.record = in[S_RECORD] != 0; r.n = (int)in[S_N]; r.single = in[S_SINGLE] != 0; r.dyn = in[S_DYN] != 0;
    r.V = (int)in[S_V]; r.top_k = (int)in[S_TOP_K]; r.top_p = (float)top_p;
    const SelectPlan p = select_plan(r);
    out[0] = p.rc; p.fields(out + 1);
    put_error(err, err_len, p.error);
}
// out: the GENERATE_PLAN_FIELDS
extern "C" void generate_plan_shim(const long long* in, double top_p, int* out) {
    GenerateShape s;
    s.sampled = in[G_SAMPLED] != 0; s.constrained = in[G_CONSTRAINED] != 0; s.record = in[G_RECORD] != 0; s.pen = in[G_PEN] != 0; s.max_new = (int)in[G_MAX_NEW];
    s.first_is_eos = in[G_FIRST_IS_EOS] != 0; s.V = (int)in[G_V]; s.top_k = (int)in[G_TOP_K]; s.top_p = (float)top_p; s.lp_top = (int)in[G_LP_TOP]; s.cons_gen = (unsigned)in[G_CONS_GEN];
    s.gate.no_graph = in[G_NO_GRAPH] != 0; s.gate.no_fuse = in[G_NO_FUSE] != 0; s.gate.prof_on = in[G_PROF_ON] != 0; s.gate.dtype = (int)in[G_DTYPE]; s.gate.qkv_p = in[G_QKV_P] != 0;
    s.gate.H = (int)in[G_H]; s.gate.d = (int)in[G_D];
    generate_plan(s).fields(out);
}
// in: n segments of R_COUNT integers, top_p: one per segment;  out: {rc, the ROUND_BLOCKS_FIELDS}, order: the n_sample segment indices;  plans: the SELECT_PLAN_FIELDS of
// the three blocks' plans, kind by kind
extern "C" void round_blocks_shim(const long long* in, const double* top_p, int n, int V, int* out, int* order, int* plans, char* err, int err_len) {
    RoundSeg* segs = new RoundSeg[n > 0 ? n : 1];
    for (int j = 0; j < n; ++j) {
        const long long* a = in + (size_t)j * R_COUNT; RoundSeg& s = segs[j];
        s.feed = a[R_FEED] != 0; s.sample = a[R_SAMPLE] != 0; s.sampling = a[R_SAMPLING] != 0; s.constrained = a[R_CONSTRAINED] != 0; s.rows = (int)a[R_ROWS]; s.sampler = (int)a[R_SAMPLER];
        s.top_k = (int)a[R_TOP_K]; s.top_p = (float)top_p[j];
    }
    const RoundBlocks b = round_blocks(segs, n, V);
    delete[] segs;
    out[0] = b.rc; b.fields(out + 1);
    for (int i = 0; i < b.n_sample; ++i) order[i] = b.order[i];
    for (int k = 0; k < 3; ++k) b.plan(k).fields(plans + k * SELECT_PLAN_FIELDS);
    put_error(err, err_len, b.error);
}
