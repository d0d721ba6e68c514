// C entry around gemm_plan() (mmduet_amd/csrc/gemm_plan.h) for tests/test_gemm_plan_host.py: built with the host C++ compiler alone, never part of the library.
#include "../mmduet_amd/csrc/gemm_plan.h"

// in: the fields below, in this order (pointers as integers: the planner looks at null / non-null / alignment only);  out: the plan
enum { IN_DTYPE, IN_M, IN_N, IN_K, IN_EPI, IN_OUT_F32, IN_VARIANT, IN_LDX, IN_LDW, IN_LDR, IN_LDY, IN_X, IN_W, IN_WP, IN_WP8, IN_WSCALE, IN_BIAS, IN_R, IN_Y, IN_WS, IN_WS_BYTES,
       IN_SLABS_OUT, IN_RING_SLABS_OUT, IN_CHAIN /* 0 none, 1 consumer, 2 producer */, IN_X_PM, IN_Y_PM, IN_NO_GEMV, IN_RING_FLAGS, IN_RING_MAX_BLOCKS, IN_KSPLIT_SHORT, IN_COUNT };
extern "C" int gemm_plan_shim_fields() { return IN_COUNT; }
extern "C" void gemm_plan_shim(const long long* in, int* out) {
    static int sink[4];
    GemmArgs a;
    a.X = (const void*)in[IN_X]; a.ldx = in[IN_LDX]; a.W = (const void*)in[IN_W]; a.ldw = in[IN_LDW]; a.Wp = (const void*)in[IN_WP]; a.Wp8 = (const void*)in[IN_WP8];
    a.wscale = (const float*)in[IN_WSCALE]; a.bias = (const void*)in[IN_BIAS]; a.R = (const void*)in[IN_R]; a.ldr = in[IN_LDR]; a.Y = (void*)in[IN_Y]; a.ldy = in[IN_LDY];
    a.M = (int)in[IN_M]; a.N = (int)in[IN_N]; a.K = (int)in[IN_K]; a.epi = (int)in[IN_EPI]; a.out_f32 = (int)in[IN_OUT_F32]; a.variant = (int)in[IN_VARIANT];
    a.splitk_ws = (float*)in[IN_WS]; a.splitk_ws_bytes = (size_t)in[IN_WS_BYTES];
    a.slabs_out = in[IN_SLABS_OUT] ? &sink[0] : nullptr; a.ring_slabs_out = in[IN_RING_SLABS_OUT] ? &sink[1] : nullptr;
    GemvChain ch;
    if (in[IN_CHAIN] == 1) ch.xn_h = &sink[2];
    if (in[IN_CHAIN] == 2) ch.fin_h = &sink[3];
    a.chain = in[IN_CHAIN] ? &ch : nullptr;
    a.x_pm = (int)in[IN_X_PM]; a.y_pm = (int)in[IN_Y_PM]; a.no_gemv = (int)in[IN_NO_GEMV]; a.ring_flags = (int)in[IN_RING_FLAGS]; a.ring_max_blocks = (int)in[IN_RING_MAX_BLOCKS];
    GemmTuning tune; tune.gemv_ksplit_short = (int)in[IN_KSPLIT_SHORT];
    const GemmPlan pl = gemm_plan((int)in[IN_DTYPE], a, tune);
    const int v[] = {pl.kernel, pl.tiles, pl.splits, pl.blocks, pl.mt, pl.nt, pl.wn, pl.prof_class, pl.reduce ? 1 : 0, pl.slabs, pl.ring_slabs, pl.ring_auto, pl.w_from, pl.chain,
                     pl.gx, pl.gy, pl.kt_per_block, pl.bn, pl.bm};
    for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}
