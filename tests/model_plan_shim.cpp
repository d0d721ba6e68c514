// C entry around model_dims() / weight_plan() / workspace_plan() (mmduet_amd/csrc/model_plan.h) for tests/test_model_plan_host.py: built with the host C++ compiler alone, never
// part of the library.  The plans leave as one JSON text; the configuration arrives as the mmd_config the ABI defines.
#include "../mmduet_amd/csrc/model_plan.h"
#include <string.h>

static std::string num(long long v) { return std::to_string(v); }
static std::string str(const std::string& s) { return "\"" + s + "\""; }          // (no name or message of the plan holds a quote or a backslash)

// -> the length of the text (written when it fits `cap`, with its terminator).  step_state_bytes: what model.hip passes as sizeof(StepState)
extern "C" int model_plan_shim_dump(const mmd_config* cfg, long long step_state_bytes, char* out, int cap) {
    const ModelDims d = model_dims(cfg);
    std::string j = "{\"rc\": " + num(d.rc) + ", \"error\": " + str(d.error);
    if (d.rc == MMD_OK) {
        j += ", \"dims\": {\"vit_grid\": " + num(d.vit_grid) + ", \"vit_tokens\": " + num(d.vit_tokens) + ", \"vit_seq\": " + num(d.vit_seq) + ", \"vit_kpad\": " + num(d.vit_kpad) +
             ", \"vit_ipad\": " + num(d.vit_ipad) + ", \"qkv_w\": " + num(d.qkv_w) + "}";
        const WeightPlan w = weight_plan(*cfg, d);
        j += ", \"weight_bytes\": " + num(w.weight_bytes(*cfg)) + ", \"phantom_elems\": " + num(w.phantom_elems) + ", \"weights\": [";
        for (size_t i = 0; i < w.entries.size(); ++i) {
            const WeightEntry& e = w.entries[i];
            j += std::string(i ? ", " : "") + "{\"scope\": " + num(e.scope) + ", \"layer\": " + num(e.layer) + ", \"field\": " + str(e.field) + ", \"field2\": " + str(e.field2 ? e.field2 : "") +
                 ", \"op\": " + num(e.op) + ", \"N\": " + num(e.N) + ", \"K\": " + num(e.K) + ", \"N2\": " + num(e.N2) + ", \"zero\": " + num(e.zero) + ", \"pack\": " + num(e.pack) +
                 ", \"fp8\": " + num(e.fp8) + ", \"counted\": " + num(e.counted) + ", \"release\": " + num(e.release) + ", \"refusal\": " + str(e.refusal) + ", \"src\": [";
            for (size_t k = 0; k < e.src.size(); ++k) j += std::string(k ? ", " : "") + "[" + str(e.src[k].name) + ", " + num(e.src[k].numel) + "]";
            j += "]}";
        }
        const WorkspacePlan s = workspace_plan(*cfg, d, (size_t)step_state_bytes);
        j += "], \"splitk_bytes\": " + num((long long)s.splitk_bytes) + ", \"attn_bytes\": " + num((long long)s.attn_bytes) + ", \"v_splitk_bytes\": " + num((long long)s.v_splitk_bytes) +
             ", \"v_attn_bytes\": " + num((long long)s.v_attn_bytes) + ", \"v_h32_rows\": " + num(s.v_h32_rows) + ", \"prev_cap\": " + num(s.prev_cap) + ", \"workspaces\": [";
        for (size_t i = 0; i < s.entries.size(); ++i)
            j += std::string(i ? ", " : "") + "[" + str(s.entries[i].field) + ", " + num((long long)s.entries[i].bytes) + ", " + num(s.entries[i].pinned) + "]";
        j += "]";
    }
    j += "}";
    if ((int)j.size() < cap) memcpy(out, j.c_str(), j.size() + 1);
    return (int)j.size();
}

// the check mmd_finalize_weights makes of what was loaded: `n` tensors (canonical name, elements) -> rc, the message in err
extern "C" int model_plan_shim_check(const mmd_config* cfg, const char* const* names, const long long* numels, int n, char* err, int err_len) {
    const ModelDims d = model_dims(cfg);
    if (d.rc) return d.rc;
    const WeightRefusal r = weight_plan_check(weight_plan(*cfg, d), [&](const std::string& name) {
        for (int i = 0; i < n; ++i) if (name == names[i]) return numels[i];
        return -1LL;
    });
    if (err_len > 0) { strncpy(err, r.error.c_str(), (size_t)err_len - 1); err[err_len - 1] = 0; }
    return r.rc;
}

extern "C" void model_plan_shim_canon(const char* name, char* out, int cap) { if (cap > 0) { strncpy(out, canon_name(name).c_str(), (size_t)cap - 1); out[cap - 1] = 0; } }
// bit 0: a packed copy is made; bit 1: the row-major original is released
extern "C" int model_plan_shim_packs(int dtype, long long N, long long K) { return (weight_packs(dtype, N, K) ? 1 : 0) | (weight_releases(dtype, N, K) ? 2 : 0); }
// {model_splitk_bytes at max_step_tokens, MODEL_ATTN_WS_BYTES, MODEL_TOWER_WS_BYTES, MODEL_PREV_CAP}
extern "C" void model_plan_shim_constants(int max_step_tokens, long long* out4) {
    mmd_config g{}; g.max_step_tokens = max_step_tokens;
    out4[0] = (long long)model_splitk_bytes(g); out4[1] = (long long)MODEL_ATTN_WS_BYTES; out4[2] = (long long)MODEL_TOWER_WS_BYTES; out4[3] = MODEL_PREV_CAP;
}
