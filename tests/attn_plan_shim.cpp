// C entry around attn_plan() / attn_plan_decode_multi() (mmduet_amd/csrc/attn_plan.h) for tests/test_attn_plan_host.py: built with the host C++ compiler alone, never part
// of the library.
#include "../mmduet_amd/csrc/attn_plan.h"

// in: the fields below, in this order (pointers as integers: the planner looks at null / non-null / alignment only);  out: the plan, then -- chunk form -- its table
enum { IN_DTYPE, IN_S, IN_NH, IN_NKV, IN_D, IN_N_CTX, IN_CAUSAL, IN_BATCH, IN_VARIANT, IN_LDQ, IN_LDO, IN_K_HS, IN_K_TS, IN_V_HS, IN_V_TS, IN_V_TRANSPOSED, IN_Q_BSTRIDE, IN_KV_BSTRIDE,
       IN_O_BSTRIDE, IN_Q, IN_K, IN_V, IN_WS, IN_WS_BYTES, IN_DYN, IN_DYN_SPLITS, IN_QKV_SLABS, IN_N_SLABS, IN_SEGS, IN_NSEG, IN_DECODE_RING, IN_VIT_RING, IN_MULTI, IN_COUNT };
enum { OUT_FIELDS = 25 };
extern "C" int attn_plan_shim_fields() { return IN_COUNT; }
extern "C" int attn_plan_shim_outputs() { return OUT_FIELDS; }
extern "C" int attn_plan_shim_tab() { return CHUNK_TAB; }
extern "C" int attn_plan_shim_units() { return CHUNK_UNITS; }
// out[OUT_FIELDS]; tab_start[CHUNK_TAB + 1], tab_b0 / tab_b1[CHUNK_UNITS] are written for the chunk form only
extern "C" void attn_plan_shim(const long long* in, int* out, int* tab_start, int* tab_b0, int* tab_b1) {
    AttnArgs a = {};
    a.q = (const void*)in[IN_Q]; a.ldq = in[IN_LDQ]; a.K = (const void*)in[IN_K]; a.V = (const void*)in[IN_V];
    a.k_hs = in[IN_K_HS]; a.k_ts = in[IN_K_TS]; a.v_hs = in[IN_V_HS]; a.v_ts = in[IN_V_TS]; a.v_transposed = (int)in[IN_V_TRANSPOSED]; a.ldo = in[IN_LDO];
    a.S = (int)in[IN_S]; a.nh = (int)in[IN_NH]; a.nkv = (int)in[IN_NKV]; a.d = (int)in[IN_D]; a.n_ctx = in[IN_N_CTX]; a.causal = (int)in[IN_CAUSAL];
    a.batch = (int)in[IN_BATCH]; a.q_bstride = in[IN_Q_BSTRIDE]; a.kv_bstride = in[IN_KV_BSTRIDE]; a.o_bstride = in[IN_O_BSTRIDE];
    a.ws = (float*)in[IN_WS]; a.ws_bytes = (size_t)in[IN_WS_BYTES]; a.variant = (int)in[IN_VARIANT];
    a.dyn = (const StepState*)in[IN_DYN]; a.dyn_splits = (int)in[IN_DYN_SPLITS];
    a.qkv_slabs = (const float*)in[IN_QKV_SLABS]; a.n_slabs = (int)in[IN_N_SLABS]; a.segs = (const StepState*)in[IN_SEGS]; a.nseg = (int)in[IN_NSEG];
    AttnTuning tune; tune.decode_ring = in[IN_DECODE_RING] != 0; tune.vit_ring = in[IN_VIT_RING] != 0;
    const AttnPlan pl = in[IN_MULTI] ? attn_plan_decode_multi(a) : attn_plan((int)in[IN_DTYPE], a, tune);
    const long long off = pl.ws_ml_off;
    const int v[OUT_FIELDS] = {pl.form, pl.kernel, pl.splits, pl.kv_per_split, pl.block_rows, pl.gx, pl.gy, pl.gz, pl.threads, pl.lds, pl.dp, pl.nc, pl.dvt, pl.exact ? 1 : 0, pl.f16 ? 1 : 0,
                               pl.rt, pl.nslot, pl.waves, pl.merge, pl.merge_gx, pl.merge_rows, pl.nb, (int)(off >> 31), (int)(off & 0x7fffffff), pl.form == 8 ? pl.tab.qblocks : 0};
    for (int i = 0; i < OUT_FIELDS; ++i) out[i] = v[i];
    if (pl.form == 8) {
        for (int i = 0; i <= CHUNK_TAB; ++i) tab_start[i] = pl.tab.start[i];
        for (int i = 0; i < pl.tab.qblocks * a.nkv; ++i) { tab_b0[i] = pl.tab.b0[i]; tab_b1[i] = pl.tab.b1[i]; }
    }
}
