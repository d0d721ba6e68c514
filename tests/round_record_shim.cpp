// C entry around round_blocks() with the recording fields of RoundSeg (mmduet_amd/csrc/select_plan.h) for tests/test_round_record_plan_host.py: built with the host C++
// compiler alone, never part of the library.  tests/select_plan_shim.cpp stays the entry without them.
#include "../mmduet_amd/csrc/select_plan.h"
#include <string.h>

// the integer inputs of a segment, in this order (the test reads the names from here: one list); top_p travels beside them as a double
#define RECORD_SHIM_FIELDS(F) F(FEED) F(SAMPLE) F(SAMPLING) F(CONSTRAINED) F(ROWS) F(SAMPLER) F(TOP_K) F(RECORD) F(LP_TOP)
#define F(name) R_##name,
enum { RECORD_SHIM_FIELDS(F) R_COUNT };
#undef F
#define F(name) #name,
static const char* const record_names[] = { RECORD_SHIM_FIELDS(F) };
#undef F
extern "C" int record_shim_fields() { return (int)R_COUNT; }
extern "C" const char* record_shim_field_name(int i) { return i < 0 || i >= (int)R_COUNT ? "" : record_names[i]; }
extern "C" int record_shim_outputs(int which) { return which == 0 ? SELECT_PLAN_FIELDS : which == 1 ? ROUND_BLOCKS_FIELDS : ROUND_RECORD_FIELDS; }
extern "C" int record_shim_round_max() { return SELECT_ROUND_MAX_ROWS; }

// in: n segments of R_COUNT integers, top_p: one per segment; defaults != 0: the two recording fields are left as RoundSeg declares them, whatever `in` holds.
// out: {rc, the ROUND_BLOCKS_FIELDS};  order: the n_sample segment indices;  plans: the SELECT_PLAN_FIELDS of the three blocks' plans, kind by kind;  rec0: the three tails'
// first rows;  record: the ROUND_RECORD_FIELDS;  err: the refusal's message
extern "C" void round_record_shim(const long long* in, const double* top_p, int n, int V, int defaults, int* out, int* order, int* plans, int* rec0, int* record, char* err, int err_len) {
    RoundSeg* segs = new RoundSeg[n > 0 ? n : 1];
    for (int j = 0; j < n; ++j) {
        const long long* a = in + (size_t)j * R_COUNT; RoundSeg& s = segs[j];
        s.feed = a[R_FEED] != 0; s.sample = a[R_SAMPLE] != 0; s.sampling = a[R_SAMPLING] != 0; s.constrained = a[R_CONSTRAINED] != 0; s.rows = (int)a[R_ROWS]; s.sampler = (int)a[R_SAMPLER];
        s.top_k = (int)a[R_TOP_K]; s.top_p = (float)top_p[j];
        if (!defaults) { s.record = a[R_RECORD] != 0; s.lp_top = (int)a[R_LP_TOP]; }
    }
    const RoundBlocks b = round_blocks(segs, n, V);
    delete[] segs;
    out[0] = b.rc; b.fields(out + 1);
    for (int i = 0; i < b.n_sample; ++i) order[i] = b.order[i];
    for (int k = 0; k < 3; ++k) { b.plan(k).fields(plans + k * SELECT_PLAN_FIELDS); rec0[k] = b.rec0[k]; }
    b.record_fields(record);
    if (err_len > 0) { strncpy(err, b.error, (size_t)err_len - 1); err[err_len - 1] = 0; }
}
