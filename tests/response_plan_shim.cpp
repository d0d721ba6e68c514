// C entries around mmduet_amd/csrc/response_plan.h for tests/test_response_plan_host.py: built with the host C++ compiler alone, never part of the library.
// With -DRESPONSE_PLAN_MAIN the file is a stand-alone program: it reads the table the test wrote (one question per line), asks the same entries and prints one answer per
// line -- the form in which the test runs the header under the address and undefined-behaviour sanitizers.
#include "../mmduet_amd/csrc/response_plan.h"
#include "../mmduet_amd/csrc/model_plan.h"          // MODEL_PREV_CAP: the first size of the context's penalty list
#include <string.h>

// {CONS_MAX_EOS, CONS_MAX_TABLE, LP_MAX_TOP, the four first sizes: context list, sampler list, context records, sampler records}
extern "C" void response_shim_constants(int* out) {
    const int v[7] = {CONS_MAX_EOS, CONS_MAX_TABLE, LP_MAX_TOP, MODEL_PREV_CAP, RESPONSE_SAMPLER_PREV_FIRST, RESPONSE_CTX_RECORDS_FIRST, RESPONSE_SAMPLER_RECORDS_FIRST};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
}
// meta: {rc, on, n, n_eos, min_new};  eos_out [CONS_MAX_EOS], ids_out / bias_out [CONS_MAX_TABLE]: the accepted set;  err: the refusal's message
extern "C" void constraint_set_shim(int V, const int64_t* eos, int n_eos, int min_new, const int32_t* ids, const float* bias, int n, int* meta, int64_t* eos_out, int32_t* ids_out,
                                    float* bias_out, char* err, int err_len) {
    const ConsSetResult r = constraint_set(V, eos, n_eos, min_new, ids, bias, n);
    const int m[5] = {r.rc, r.set.on, r.set.n, r.set.n_eos, r.set.min_new};
    for (int i = 0; i < 5; ++i) meta[i] = m[i];
    for (int k = 0; k < CONS_MAX_EOS; ++k) eos_out[k] = r.set.eos[k];
    for (int k = 0; k < CONS_MAX_TABLE; ++k) { ids_out[k] = r.set.ids[k]; bias_out[k] = r.set.bias[k]; }
    if (err_len > 0) { strncpy(err, r.error, (size_t)err_len - 1); err[err_len - 1] = 0; }
}
// the ids a response stops on, for a set with these EOS ids and the call's own eos_id: -> their number, out [CONS_MAX_EOS];  stops [n_probe]: response_is_eos of each probe
extern "C" int response_eos_shim(const int64_t* set_eos, int n_eos, int64_t eos_id, int V, int64_t* out, const int64_t* probe, int n_probe, int* stops) {
    ConsSet s; s.n_eos = n_eos; s.on = n_eos > 0;
    for (int k = 0; k < n_eos; ++k) s.eos[k] = set_eos[k];
    const ResponseEos e = response_eos(s, eos_id, V);
    for (int k = 0; k < CONS_MAX_EOS; ++k) out[k] = e.ids[k];
    for (int i = 0; i < n_probe; ++i) stops[i] = response_is_eos(e, probe[i]);
    return e.n;
}
extern "C" int grow_capacity_shim(int cap, int need, int first) { return grow_capacity(cap, need, first); }
// {generate_prev_need, sampler_prev_need, sampler_records_need}
extern "C" void response_needs_shim(int n_prev, int max_new, int* out) { out[0] = generate_prev_need(n_prev, max_new); out[1] = sampler_prev_need(n_prev, max_new); out[2] = sampler_records_need(max_new); }
// count: {step, lp_n, n_prev, max_new, ended}, updated;  -> the token joins the penalty list
extern "C" int response_note_shim(int* count, int is_eos, int pen, int record, int prev_cap) {
    ResponseCount c; c.step = count[0]; c.lp_n = count[1]; c.n_prev = count[2]; c.max_new = count[3]; c.ended = count[4] != 0;
    const bool joins = response_note_token(c, is_eos != 0, pen != 0, record != 0, prev_cap);
    count[0] = c.step; count[1] = c.lp_n; count[2] = c.n_prev; count[3] = c.max_new; count[4] = c.ended;
    return joins;
}

#ifdef RESPONSE_PLAN_MAIN
#include <stdlib.h>
#include <fstream>
#include <sstream>
#include <string>
// lines of the table:
//   C name V n_eos null_eos min_new n null_tab  eos ids ...  table ids ...  biases ...      (max(count, 0) values each; none for a null list)
//   E name n_eos eos ... eos_id V n_probe probes ...
//   G cap need first
//   N name max_new prev_cap n_prev pen record n  is_eos ...
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s TABLE\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int c7[7]; response_shim_constants(c7);
    printf("K"); for (int v : c7) printf(" %d", v); printf("\n");
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string kind, name; ls >> kind;
        if (kind == "C") {
            int V, n_eos, null_eos, min_new, n, null_tab; ls >> name >> V >> n_eos >> null_eos >> min_new >> n >> null_tab;
            std::vector<int64_t> eos((size_t)(null_eos || n_eos < 0 ? 0 : n_eos)); std::vector<int32_t> ids((size_t)(null_tab || n < 0 ? 0 : n)); std::vector<float> bias(ids.size());
            for (auto& v : eos) { long long x; ls >> x; v = x; }
            for (auto& v : ids) ls >> v;
            for (auto& v : bias) { std::string t; ls >> t; v = strtof(t.c_str(), nullptr); }
            int meta[5]; int64_t eo[CONS_MAX_EOS]; int32_t io[CONS_MAX_TABLE]; float bo[CONS_MAX_TABLE]; char err[256];
            // (exact-size heap arrays: a read past the counts is the sanitizer's to report)
            constraint_set_shim(V, null_eos ? nullptr : eos.data(), n_eos, min_new, null_tab ? nullptr : ids.data(), null_tab ? nullptr : bias.data(), n, meta, eo, io, bo, err, (int)sizeof(err));
            printf("C %s %d %d %d %d %d |", name.c_str(), meta[0], meta[1], meta[2], meta[3], meta[4]);
            if (meta[0] == MMD_OK) {
                for (int k = 0; k < meta[3]; ++k) printf(" %lld", (long long)eo[k]);
                printf(" |");
                for (int k = 0; k < meta[2]; ++k) { uint32_t b; memcpy(&b, &bo[k], 4); printf(" %d:%08x", io[k], b); }
            }
            printf(" | %s\n", err);
        } else if (kind == "E") {
            int n_eos, V, n_probe; long long eos_id; ls >> name >> n_eos;
            std::vector<int64_t> eos((size_t)n_eos); for (auto& v : eos) { long long x; ls >> x; v = x; }
            ls >> eos_id >> V >> n_probe;
            std::vector<int64_t> probe((size_t)n_probe); for (auto& v : probe) { long long x; ls >> x; v = x; }
            int64_t out[CONS_MAX_EOS]; std::vector<int> stops((size_t)n_probe);
            const int n = response_eos_shim(eos.data(), n_eos, eos_id, V, out, probe.data(), n_probe, stops.data());
            printf("E %s %d |", name.c_str(), n);
            for (int k = 0; k < n; ++k) printf(" %lld", (long long)out[k]);
            printf(" |");
            for (int v : stops) printf(" %d", v);
            printf("\n");
        } else if (kind == "G") {
            int cap, need, first; ls >> cap >> need >> first;
            printf("G %d\n", grow_capacity_shim(cap, need, first));
        } else if (kind == "N") {
            int max_new, prev_cap, n_prev, pen, record, n; ls >> name >> max_new >> prev_cap >> n_prev >> pen >> record >> n;
            int count[5] = {0, 0, n_prev, max_new, 0};
            printf("N %s", name.c_str());
            for (int i = 0; i < n; ++i) {
                int e; ls >> e;
                const int joins = response_note_shim(count, e, pen, record, prev_cap);
                printf(" %d,%d,%d,%d,%d", count[0], count[1], count[2], count[4], joins);
            }
            printf("\n");
        } else if (!kind.empty()) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
#endif
