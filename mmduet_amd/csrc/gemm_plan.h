// gemm_plan.h -- the GEMM dispatch decision of the library, and nothing else: which kernel runs, in which instantiation, over which grid and with how many K splits.
// One pure host function, gemm_plan(): no GPU header, no runtime call, no environment; it compiles with the host C++17 compiler alone (tests/test_gemm_plan_host.py runs the
// regime table of tests/gemm_regimes.py through it without a GPU).  launch_gemm evaluates it once per GEMM and launches what it says; callers that need the answer
// before they launch (gemm_can_slab, gemm_ring_auto, the profiler class of the model's gemm()) ask the same function.  Every threshold of the dispatch lives here.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/mmduet.h"

constexpr int MMD_F16 = 2;             // internal launcher dtype, never a context dtype: 2-byte IEEE half activations / weights, fp32 accumulate and statistics

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// ---- epilogues of the GEMM family ------------------------------------------------------------------------------
enum { EPI_NONE = 0, EPI_GELU_TANH = 1, EPI_GELU_ERF = 2, EPI_RESID = 3, EPI_SWIGLU = 4 };
enum { GEMM_AUTO = 0, GEMM_GENERIC = 1, GEMM_SKINNY = 2, GEMM_LARGE = 3, GEMM_BIG = 4, GEMM_SLAB = 5, GEMM_RING256 = 6, GEMM_RING256_SPLIT = 7,
       GEMM_RINGX = 16 /* + 1: 4-wave 256x128 blocks, + 2: 32x32x16 MFMA, + 4: split K */,
       GEMM_STREAM = 8 /* gemm_stream_kernel (32 < M <= 256, slabs or SwiGLU) */ };

// Decode chain of the weight-streaming GEMV (M <= 16, bf16): the residual add + RMSNorm between two GEMVs costs a launch and a cold, dependent
// load chain of its own (5.5 us + a kernel boundary, twice per layer at decode).  Instead
//   * the PRODUCER (o_proj / down_proj) owns an n-tile over all of K (one 16-wave block per tile, K split over the waves, LDS reduce) and folds
//     its result into the residual stream itself: h = rnd(rnd(x W^T) + h), leaving that tile's per-row sum of h^2 in ssq[m][tile];
//   * the CONSUMER (qkv / gate_up) never reads a normalised activation: every lane builds its X fragment as rnd(gamma * rnd(h * inv)),
//     inv = rsqrt(sum(ssq[m][:]) / K + eps) summed in a fixed order (deterministic; same rounding points as slab_resid_rmsnorm_kernel).
constexpr int GEMV_SSQ_STRIDE = 256;   // floats per row in ssq (n-tiles of 16 columns: N <= 4096)
constexpr int GEMV_CHAIN_ROWS = 4;     // rows a consumer keeps in LDS, 1024 k per wave (plan_gemv16 refuses the rest)
struct GemvChain {
    const void* xn_h = nullptr; const void* xn_gamma = nullptr; const float* xn_ssq = nullptr; float xn_eps = 0.f;     // consumer side
    void* fin_h = nullptr; float* fin_ssq = nullptr;                                                                     // producer side
};
struct GemmArgs {
    const void* X; int64_t ldx;      // [M,K]
    const void* W; int64_t ldw;      // [N,K]  (nn.Linear layout); may be null when only Wp exists
    const void* Wp = nullptr;        // same matrix, MFMA-fragment-major (launch_pack_w); enables the weight-streaming skinny kernel
    const void* Wp8 = nullptr;       // fp8 e4m3 copy of the (unscaled) weights, fragment-major in 64-k pairs (launch_pack_w8): the weight-streaming
                                     // kernels (M <= 64) read this one -- half the bytes; W / Wp then hold bf16(q), bit-identical values
    const float* wscale = nullptr;   // per-output-channel scale of a quantised matrix: Y = (X . q^T) * wscale[n] (+ bias ...)
    const void* bias;                // [N] or null (ctx dtype)
    const void* R; int64_t ldr;      // residual [M,N] (EPI_RESID)
    void* Y; int64_t ldy;            // [M,N] (or [M,N/2] for SWIGLU); ctx dtype, or fp32 if out_f32
    int M, N, K;
    int epi; int out_f32;
    int variant;
    float* splitk_ws; size_t splitk_ws_bytes;   // fp32 partial slabs
    int no_gemv = 0;                            // A/B switch: use the LDS-staged skinny kernel also for M <= 16
    int* ring_slabs_out = nullptr;              // if set: a split-K tile GEMM (ring / 128-row) leaves its [splits][M][N] fp32 slabs in splitk_ws and reports the count here
                                                // (0 = the GEMM ran unsplit and applied its epilogue itself); the caller consumes them with launch_slab_resid_rmsnorm
    int* slabs_out = nullptr;                   // if set (packed skinny path only): leave [splits][M][N] fp32 slabs in splitk_ws, no
                                                // epilogue, and return the split count here; a fused consumer kernel reduces them
    int ring_flags = 16;                        // ring GEMM instantiation the auto dispatch uses (16 = 8 waves, 256 x 256, early refill; 17 = 4 waves, 256 x 128)
    int ring_max_blocks = 0;                    // > 0: cap on the persistent grid (co-residency experiments: leave CU resources to another stream)
    const GemvChain* chain = nullptr;           // gemv16 path only (M <= 16, packed bf16 / fp8 weights); see GemvChain
    int* plan_out = nullptr;                    // if set: int[4] = {kernel (GEMM_K_*), output tiles, K splits, blocks launched}
    int x_pm = 0, y_pm = 0;                     // X is / Y becomes a PIECE-MAJOR activation ([M/16][K/32] pieces of 16 rows x 32 elements, gemm_ringx_kernel): ring GEMMs only -- ask gemm_ring_auto first
    int f16 = 0;                                // operands, bias, residual and output are IEEE half (launch_gemm(MMD_F16, ...): the fp16 vision tower; ring / big kernels only)
};
// which kernel the dispatcher chose (mmd_op_gemm_last_plan; parity tests assert the production kernel really ran)
enum { GEMM_K_TILE64 = 0, GEMM_K_TILE128 = 1, GEMM_K_SKINNY = 2, GEMM_K_GEMV16 = 3, GEMM_K_BIG64 = 4, GEMM_K_BIG128 = 5, GEMM_K_RING256 = 6, GEMM_K_RING128X2 = 7, GEMM_K_STREAM = 8 };

// what the decision depends on besides its arguments
struct GemmTuning {
    int gemv_ksplit_short = 2;       // K slabs of the GEMV at short K and few n-tiles (MMDUET_GEMV_KSPLIT_SHORT, clamped to 1..4)
};

enum { GEMM_PLAN_INVALID = -1,       // no kernel takes these arguments: launch_gemm returns an invalid-value error
       GEMM_PLAN_EMPTY = -2 };       // M or N is 0: nothing to launch
enum { GEMM_W_ROWMAJOR = 0, GEMM_W_PACKED = 1, GEMM_W_PACKED8 = 2 };          // the W a kernel reads: GemmArgs::W, Wp or Wp8
enum { GEMV_PLAIN = 0, GEMV_CONSUMER = 1, GEMV_PRODUCER = 2 };                // chain form of the GEMV (GemvChain)
enum { RING_AUTO_NONE = 0, RING_AUTO_PLAIN = 1, RING_AUTO_SPLIT = 2 };

// Everything a launcher needs: it maps these integers to a template instantiation and launches, and computes nothing itself.
struct GemmPlan {
    int kernel = GEMM_PLAN_INVALID;  // GEMM_K_*, or GEMM_PLAN_INVALID / GEMM_PLAN_EMPTY
    int tiles = 0, splits = 1, blocks = 0;      // with `kernel`: what mmd_op_gemm_last_plan reports
    int gx = 0, gy = 1;              // grid without the split dimension (blocks = gx * gy * splits)
    int prof_class = MMD_K_GEMM_TILE;           // profiler class of the kernel that runs: MMD_K_GEMM_SKINNY (weight-streaming kernels, the 64-row tile kernel at M <= 64) or MMD_K_GEMM_TILE
    int w_from = GEMM_W_ROWMAJOR;
    int mt = 0, nt = 0, wn = 0;      // instantiation: 16-row groups (skinny, stream), n-tiles per wave (skinny, GEMV, stream), column-group width (stream: waves; ring: 4 = 256 x 256 tiles on 8 waves, 2 = 256 x 128 on 4)
    int kt_per_block = 0;            // skinny / stream: 32-deep k-tiles per block of a split
    int kper = 0;                    // GemmP::kper: K elements per split (generic tile kernel); start-up stagger of the second-slot blocks in ~4 us units (ring)
    int bn = 0, bm = 0;              // block tile of gemm_big_kernel
    int chain = GEMV_PLAIN;
    int f16 = 0;                     // IEEE-half forms of the ring / big kernels
    int ring_auto = RING_AUTO_NONE;  // the AUTOMATIC dispatch chose the 8-wave ring, in its plain or its split-K form (what a piece-major operand needs)
    bool reduce = false;             // a splitk_reduce_kernel launch follows (the slabs are not left to the caller)
    int slabs = 0;                   // weight-streaming kernels with GemmArgs::slabs_out: what *slabs_out receives
    int ring_slabs = 0;              // what *ring_slabs_out receives: the slabs a split-K ring / big GEMM leaves to the caller, else 0
    bool valid() const { return kernel >= 0; }
};

// gemm_stream_kernel: 32 < M <= 256, packed bf16 weights, slab output (fused consumers) or the SwiGLU epilogue.  K must be a whole number of steps.
static inline bool stream_ok(int dtype, const GemmArgs& a) {
    if (dtype != MMD_BF16 || a.f16 || !a.Wp || a.M <= 32 || a.M > 256 || (a.N % 16) != 0 || (a.ldx % 8) != 0 || ((uintptr_t)a.X % 16) != 0 || a.out_f32) return false;
    if (a.Wp8 && a.M <= 64) return false;                                  // fp8 builds keep the 1-byte skinny kernel where it exists
    if ((long long)a.M * a.ldx * 2 >= (1ll << 32)) return false;            // X addressed as base + 32-bit offset
    const int ksb = a.M <= 128 ? 4 : 2;          // k-tiles per step of the instantiation that serves this M
    if ((a.K % (ksb * 32)) != 0) return false;
    if (a.epi == EPI_SWIGLU) return (a.N % 32) == 0 && !a.slabs_out;
    if (a.slabs_out) return a.splitk_ws != nullptr && a.epi == EPI_NONE && (size_t)a.M * a.N * sizeof(float) <= a.splitk_ws_bytes;          // (even ONE slab must fit)
    // epilogue in place (unfused schedule, several streams per forward): the same K split into the workspace, then the serial slab reduce applies bias / residual / activation --
    // slab for slab what the fused consumers do, so both schedules produce the same bits
    return a.splitk_ws != nullptr && (a.N % 4) == 0 && (a.ldy % 4) == 0 && (a.epi != EPI_RESID || (a.ldr % 4) == 0);
}
// Launch geometry of gemm_stream_kernel<MT, NT, ..., WN> with KSB k-tiles per step: `want_split` K splits (0: about one block per CU and a bit), trimmed to whole steps,
// >= 6 steps per block and the workspace.  (Also what the configuration sweep of a debug build fills its launches with.)
static inline void stream_geometry(GemmPlan& pl, const GemmArgs& a, int MT, int NT, int KSB, int WN, int want_split) {
    const int KT = a.K >> 5, ntiles = a.N >> 4;
    const int bx = cdiv(ntiles, WN * NT);
    int ksplit = 1;
    if (a.slabs_out || (a.epi != EPI_SWIGLU && a.splitk_ws)) {
        ksplit = want_split > 0 ? want_split : cdiv(288, bx);                                            // ~ one block per CU and a bit: every CU streams
        const int maxs = KT / (KSB * 6); if (ksplit > maxs) ksplit = maxs;  // >= 6 steps per block (the pipeline is NB - 1 steps deep)
        if (ksplit > 16) ksplit = 16;
        if (ksplit < 1) ksplit = 1;
        while (ksplit > 1 && (size_t)ksplit * a.M * a.N * sizeof(float) > a.splitk_ws_bytes) --ksplit;
    }
    const int ktper = (int)round_up(cdiv(KT, ksplit), KSB);
    ksplit = cdiv(KT, ktper);
    pl.kernel = GEMM_K_STREAM; pl.tiles = ntiles; pl.splits = ksplit; pl.blocks = bx * ksplit; pl.gx = bx; pl.gy = 1;
    pl.w_from = GEMM_W_PACKED; pl.mt = MT; pl.nt = NT; pl.wn = WN; pl.kt_per_block = ktper;
    pl.slabs = ksplit;
    pl.reduce = !a.slabs_out && ksplit > 1;          // epilogue in place: the serial slab reduce (slab 0, 1, 2, ... -- the fused consumers' order)
}
// Decomposition of a streaming GEMM over the 256 CUs.  A CU streams ~25 GB/s whatever runs on it, so the launch is as long as its busiest CU: 296 four-wave blocks
// (gate_up at WN = 4) take two block rounds for 1.16 rounds of work -- 63 us where 237 five-pair blocks take 46 (tools/bench_gemm.py stream, profiles/r04_stream_sweep.txt).
// Pick the column-group width WN (n-tile slots per block = waves) and the K split that minimise   rounds x (W bytes + 0.5 X bytes per block) + slab bytes / 256
// under: whole K steps per block, >= 6 steps per block when K is split (the pipeline is NB - 1 steps deep), slabs within the workspace.
struct StreamPlan { int wn, ksplit; };
static inline StreamPlan stream_plan(const GemmArgs& a, int NT, int MT, int KSB, bool can_split) {
    const int KT = a.K >> 5, ntiles = a.N >> 4;
    StreamPlan best{4, 1}; double best_cost = 1e30;
    for (int wn = 4; wn <= 8; ++wn) {
        const int bx = cdiv(ntiles, wn * NT);
        for (int ks = 1; ks <= (can_split ? 16 : 1); ++ks) {
            const int ktper = (int)round_up(cdiv(KT, ks), KSB);
            if (cdiv(KT, ktper) != ks) continue;                                            // (this split count rounds to another one)
            if (ks > 1 && ktper < 6 * KSB) break;
            if (ks > 1 && (size_t)ks * a.M * a.N * sizeof(float) > a.splitk_ws_bytes) break;
            const int rounds = cdiv((long long)bx * ks, 256);
            const double wb = (double)wn * NT * ktper * 1024, xb = (double)MT * 16 * ktper * 64;
            const double slab = can_split ? (double)ks * a.M * a.N * 8.0 / 256.0 : 0.0;
            const double cost = rounds * (wb + 0.5 * xb) + slab;
            if (cost < best_cost * 0.999) { best_cost = cost; best = StreamPlan{wn, ks}; }
        }
    }
    return best;
}
// the instantiation that serves M rows: MT 16-row groups, NT n-tiles per wave, KSB = WK x KS k-tiles per step (launch_stream holds the WK / KS / NB of each)
static inline GemmPlan plan_stream(const GemmArgs& a) {
    const bool two = a.epi == EPI_SWIGLU || (a.N >> 4) >= 4096;
    const int MT = a.M <= 64 ? 4 : (a.M <= 128 ? 8 : 16), NT = two ? 2 : 1;
    const int KSB = a.M <= 64 ? 4 : (a.M <= 128 ? (two ? 2 : 4) : (two ? 1 : 2));
    const StreamPlan sp = stream_plan(a, NT, MT, KSB, a.slabs_out != nullptr || (a.epi != EPI_SWIGLU && a.splitk_ws != nullptr));
    GemmPlan pl;
    stream_geometry(pl, a, MT, NT, KSB, sp.wn, sp.ksplit);
    return pl;
}

// the weight-streaming GEMV, M <= 16
static inline GemmPlan plan_gemv16(const GemmArgs& a, const GemmTuning& tune) {
    const int KT = a.K >> 5, ntiles = a.N >> 4;
    int ksplit = 1;
    if (a.slabs_out && ntiles < 512 && KT >= 256 && a.splitk_ws) {          // long K, few n-tiles (down_proj): 2-4 K slabs
        ksplit = cdiv(768, ntiles); if (ksplit > 4) ksplit = 4;
        while (ksplit > 1 && (size_t)ksplit * a.M * a.N * sizeof(float) > a.splitk_ws_bytes) --ksplit;
    }
    else if (a.slabs_out && ntiles < 512 && a.splitk_ws) {
        // short K, few n-tiles (qkv, o at decode): one block per n-tile is latency-bound (8.0 / 6.4 us for 33 / 26 MB); two K slabs halve each wave's
        // dependent load chain: 6.7 / 5.3 us (fp8: 6.0 / 5.2 -> 4.7 / 4.1); the slab consumers sum them for free.  MMDUET_GEMV_KSPLIT_SHORT overrides (1..4)
        const int ks_short = tune.gemv_ksplit_short;
        ksplit = ks_short < 1 ? 1 : (ks_short > 4 ? 4 : ks_short);
        while (ksplit > 1 && (size_t)ksplit * a.M * a.N * sizeof(float) > a.splitk_ws_bytes) --ksplit;
    }
    const bool two = a.epi == EPI_SWIGLU || (ntiles % 2 == 0 && ntiles >= 2048);
    const bool chain = a.chain && (a.chain->xn_h || a.chain->fin_h);          // (GemmArgs::chain is a host struct of the arguments: the one pointer the planner looks behind)
    // what the chain forms of the kernel cannot take (step_plan keeps the model inside; any other caller is refused here, before a launch):
    //   * producer: ssq has GEMV_SSQ_STRIDE n-tile entries per row;
    //   * consumer: a wave keeps GEMV_CHAIN_ROWS rows x 1024 k of ITS K range in LDS and normalises them in two passes of 512 (the kernel's ranges: K tiles -- fp8: pairs of
    //     tiles -- over the splits, then over the 4 waves, both rounded up).
    if (chain && a.chain->fin_h && a.N > 16 * GEMV_SSQ_STRIDE) return GemmPlan();
    if (chain && !a.chain->fin_h) {
        const int kg = a.Wp8 ? 2 : 1, k_wave = cdiv(cdiv(KT / kg, ksplit), 4) * 32 * kg;
        if (a.M > GEMV_CHAIN_ROWS || k_wave > 1024) return GemmPlan();
    }
    GemmPlan pl;
    pl.kernel = GEMM_K_GEMV16; pl.tiles = ntiles; pl.w_from = a.Wp8 ? GEMM_W_PACKED8 : GEMM_W_PACKED;
    if (chain && a.chain->fin_h) {
        // producer: one 16-wave block per n-tile, K split over the waves (no slabs, no second kernel)
        pl.splits = 1; pl.gx = ntiles; pl.nt = 1; pl.chain = GEMV_PRODUCER; pl.slabs = 0;
    } else {
        pl.splits = ksplit; pl.gx = two ? ntiles / 2 : ntiles; pl.nt = two ? 2 : 1; pl.chain = chain ? GEMV_CONSUMER : GEMV_PLAIN; pl.slabs = ksplit;
    }
    pl.blocks = pl.gx * pl.splits;
    return pl;
}

// the LDS-staged skinny kernel, MT 16-row groups (16 < M <= 32; fp8 weights up to 64 rows)
static inline GemmPlan plan_skinny(const GemmArgs& a, int MT) {
    const int KT = a.K >> 5, ntiles = a.N >> 4;
    const int NT = (a.epi == EPI_SWIGLU || ntiles >= 4096) ? 2 : 1;
    int nblocks = cdiv(ntiles, 4 * NT);
    int splits = 1;
    if (nblocks < 512 && a.epi != EPI_SWIGLU && a.splitk_ws) {
        splits = cdiv(512, nblocks);
        int maxs = KT / 16; if (maxs < 1) maxs = 1;              // >= 512 k per split
        if (splits > maxs) splits = maxs;
        if (splits > 8) splits = 8;
        while (splits > 1 && (size_t)splits * a.M * a.N * sizeof(float) > a.splitk_ws_bytes) --splits;
    }
    int ktper = (int)round_up(cdiv(KT, splits), 4);
    splits = cdiv(KT, ktper);
    GemmPlan pl;
    pl.kernel = GEMM_K_SKINNY; pl.tiles = ntiles; pl.splits = splits; pl.blocks = nblocks * splits; pl.gx = nblocks;
    pl.w_from = a.Wp8 ? GEMM_W_PACKED8 : GEMM_W_PACKED; pl.mt = MT; pl.nt = NT; pl.kt_per_block = ktper;
    pl.slabs = splits;
    pl.reduce = !a.slabs_out && splits > 1;
    return pl;
}

// 160-row tiles of the 64-column form (plain / residual epilogue, bf16: a chunk's qkv / o_proj): when they take fewer block rounds per CU.  A CU holds three 128 x 64 blocks
// (48 KB of LDS each) or two 160 x 64 ones (56 KB); a CU's time ~ blocks it runs x rows per block.
static inline bool big_bm160(const GemmArgs& a, int BN) {
    if (BN != 64 || a.f16 || (a.epi != EPI_NONE && a.epi != EPI_RESID) || a.M < 512) return false;
    const long long t128 = (long long)(a.N / 64) * cdiv(a.M, 128), t160 = (long long)(a.N / 64) * cdiv(a.M, 160);
    if (t160 > 512) return false;                                          // (a third block per CU would have to wait for a slot)
    return (double)cdiv(t160, 256) * 160.0 < (double)cdiv(t128, 256) * 128.0 * 0.97;
}
// gemm_big_kernel<BN>: 128 (or 160) x BN block tiles
static inline GemmPlan plan_big(const GemmArgs& a, int BN) {
    GemmPlan pl;
    pl.kernel = BN == 128 ? GEMM_K_BIG128 : GEMM_K_BIG64; pl.w_from = GEMM_W_PACKED; pl.bn = BN; pl.f16 = a.f16;
    if (big_bm160(a, BN)) {
        const int tiles = (a.N / 64) * cdiv(a.M, 160);
        pl.tiles = tiles; pl.splits = 1; pl.blocks = tiles; pl.gx = a.N / 64; pl.gy = cdiv(a.M, 160); pl.bm = 160;
        return pl;
    }
    const int tiles = (a.N / BN) * cdiv(a.M, 128);
    int splits = 1;
    if (tiles < 320 && a.K >= 8192 && a.epi != EPI_SWIGLU && a.splitk_ws && !a.f16) {      // long K, under one block per CU (down_proj): split K
        splits = 3;                                                                // (measured: splitting K = 3584 GEMMs costs more than it fills)
        if (tiles <= 64) splits = 4;
        while (splits > 1 && (size_t)splits * a.M * a.N * sizeof(float) > a.splitk_ws_bytes) --splits;
    } else if (tiles < 128 && a.K >= 2048 && a.epi != EPI_SWIGLU && a.splitk_ws && !a.f16) {
        // a handful of rows (65 <= M <= ~256: a few frames per forward, several streams' decode rows): 56-72 tiles cannot pull the weights out of HBM (a CU streams ~25 GB/s);
        // split K so that ~one block per CU streams.  round 3, 15 k context: an M = 98 step 8.5 -> see profiles/r03_decode_experiments.md
        splits = 256 / tiles; if (splits > 4) splits = 4; if (splits < 1) splits = 1;
        while (splits > 1 && (size_t)splits * a.M * a.N * sizeof(float) > a.splitk_ws_bytes) --splits;
    }
    pl.tiles = tiles; pl.splits = splits; pl.blocks = tiles * splits; pl.gx = a.N / BN; pl.gy = cdiv(a.M, 128); pl.bm = 128;
    if (splits > 1) {
        if (a.ring_slabs_out) pl.ring_slabs = splits;          // the caller folds the slabs itself (reduce + residual + RMSNorm in one pass)
        else pl.reduce = true;
    }
    return pl;
}

// the ring GEMM addresses its operands as uniform base + 32-bit byte offset
static inline bool ring_size_ok(const GemmArgs& a) { return (long long)a.M * a.ldx * 2 < (1ll << 32) && (long long)a.N * a.K * 2 < (1ll << 32); }
// enough 256^2 tiles for the persistent ring: >= 400 (1.6 block waves of the 256 CUs), or close to whole waves from 0.75 of one up (4096^2: 256 tiles = one
// wave, 1.36 PF against 0.94 for the 128-row kernel; 300 tiles would leave the second wave at 17 % and stay with the 128-row kernel)
static inline bool ring_tiles_ok(long long t) { return t >= 400 || (t >= 192 && (double)t / (double)(cdiv((int)t, 256) * 256) >= 0.9); }
static inline bool big_packed_ok(int dtype, const GemmArgs& a, int BN) {
    return dtype == MMD_BF16 && a.Wp != nullptr && a.M > 64 && (a.N % BN) == 0 && (a.K % 64) == 0 && (a.ldx % 8) == 0 &&
           ((uintptr_t)a.X % 16) == 0 && !a.out_f32 && (a.ldy % 4) == 0 && ((uintptr_t)a.Y % 8) == 0 &&
           (a.epi != EPI_RESID || ((a.ldr % 4) == 0 && ((uintptr_t)a.R % 8) == 0)) && (a.bias == nullptr || ((uintptr_t)a.bias % 8) == 0);
}

// packed-W skinny path usable?  bf16, M <= 64, N % 16 == 0, K % 32 == 0, 16-byte aligned rows of X
static inline bool skinny_packed_ok(int dtype, const GemmArgs& a) {
    return dtype == MMD_BF16 && a.Wp != nullptr && a.M <= 64 && (a.N % 16) == 0 && (a.K % 32) == 0 && (a.ldx % 8) == 0 &&
           ((uintptr_t)a.X % 16) == 0 && (a.epi != EPI_SWIGLU || (a.N % 32) == 0);
}

// K splits of the split-K ring for t256 output tiles.  Up to half a block wave of tiles: as many splits as fit one wave (down_proj of a chunk: 70 tiles x 3).  Between half a
// wave and the plain ring's threshold (down_proj of several streams' merged chunks: M = 2548 -> 140 tiles, which left 116 CUs idle for the whole K on the plain ring and ran at
// 0.28 of peak on the 128-row kernel) the split count comes from a small cost model: rounds of 256 blocks x K / sp steps of ~25 ns per unit of K, plus the fp32 slabs' write + read
// at ~5 TB/s (140 tiles: 3 splits = 420 items in two rounds of K / 3 -- two thirds of the unsplit time).
static inline int ring_split_choice(const GemmArgs& a) {
    const int t256 = cdiv(a.M, 256) * cdiv(a.N, 256);
    int sp = 256 / t256; if (sp < 1) sp = 1;
    if (t256 > 128) {
        double best = 1e30; int bsp = 1;
        for (int s = 1; s <= 8; ++s) {
            if (s > 1 && (a.K / s < 1024 || (size_t)s * a.M * a.N * sizeof(float) > a.splitk_ws_bytes)) break;
            const double rounds = (double)cdiv(t256 * s, 256);
            const double cost = rounds * ((double)a.K / s) * 0.025 + (s > 1 ? (double)s * a.M * a.N * 8.0 / 5e6 : 0.0);
            if (cost < best * 0.97) { best = cost; bsp = s; }          // (a finer split has to buy 3 %)
        }
        return bsp;
    }
    while (sp > 1 && a.K / sp < 1024) --sp;
    while (sp > 1 && (size_t)sp * a.M * a.N * sizeof(float) > a.splitk_ws_bytes) --sp;
    return sp;
}
// gemm_ringx_kernel.  flags: 16 = 8 waves, 256 x 256 tiles, three-slot ring, refill DMAs in the first rows of a step (every tower / projector GEMM, gate_up and split-K down of a
// chunk); 17 = 4 waves, 256 x 128 tiles, two blocks per CU (a chunk's qkv / o_proj where 256 x 256 tiles cannot fill the device).  The flag values of the alternatives that lost their
// A/B and were removed (late refill, 32x32x16 MFMA, four slots: header of gemm_ringx_kernel) give an invalid plan.
static inline GemmPlan plan_ring(const GemmArgs& a, int flags, int splits) {
    GemmPlan pl;
    int WN = 4;                                                              // the fp16 tower runs the production 8-wave instantiation
    if (!a.f16) switch (flags & 27) {
        case 16: WN = 4; break;
        case 17: WN = 2; break;
        default: return pl;
    }
    if (a.f16 && a.epi != EPI_NONE && a.epi != EPI_GELU_TANH && a.epi != EPI_RESID) return pl;          // the IEEE-half form has the plain / GELU(tanh) / residual epilogues
    if (a.f16) splits = 1;
    while (splits > 1 && (a.epi == EPI_SWIGLU || !a.splitk_ws || (size_t)splits * a.M * a.N * sizeof(float) > a.splitk_ws_bytes)) --splits;
    const int BN = 64 * WN;
    const int tiles = cdiv(a.N, BN) * cdiv(a.M, 256);
    const int slots = WN == 2 ? 512 : 256;                      // resident blocks: two 4-wave blocks per CU (72 KB rings), else one
    // ring_max_blocks: > 0 caps the persistent grid (tower share); < 0 (the overlap experiments of round 4, tools/probes/dropped/overlap_sweep.sh): NON-persistent, one tile per block, so that the
    // dispatcher can place another stream's blocks at every tile end
    const int cap = a.ring_max_blocks < 0 ? tiles : (a.ring_max_blocks > 0 && a.ring_max_blocks < slots ? a.ring_max_blocks : slots);
    pl.kernel = WN == 2 ? GEMM_K_RING128X2 : GEMM_K_RING256; pl.w_from = GEMM_W_PACKED; pl.wn = WN; pl.f16 = a.f16;
    pl.gx = splits > 1 || tiles <= cap ? tiles : cap;
    pl.tiles = tiles; pl.splits = splits; pl.blocks = pl.gx * splits;
    // start-up stagger of the second-slot blocks in ~4 us units: about half a tile (K/32 steps of ~0.75 us) -- see the kernel
    pl.kper = splits > 1 ? 0 : ((a.K / 32) * 10) / 100 + 1;
    if (splits > 1) {
        if (a.ring_slabs_out) pl.ring_slabs = splits;
        else pl.reduce = true;
    }
    return pl;
}

// the generic tile kernels (any dtype, row-major W): 64-row tiles with a K split for skinny shapes, 128-row tiles for large ones
static inline GemmPlan plan_tile(const GemmArgs& a, bool skinny, bool large) {
    int splits = 1;
    if (skinny) {
        int blocks = cdiv(a.N, 64) * cdiv(a.M, 64);
        int want = cdiv(512, blocks);
        int maxs = a.K / 256; if (maxs < 1) maxs = 1;
        splits = want < maxs ? want : maxs;
        if (splits > 16) splits = 16;
        if (a.splitk_ws == nullptr) splits = 1;
        while (splits > 1 && (size_t)splits * a.M * a.N * sizeof(float) > a.splitk_ws_bytes) --splits;
    }
    int kper = (int)round_up(cdiv(a.K, splits), 32);
    splits = cdiv(a.K, kper);
    GemmPlan pl;
    pl.kper = kper;
    const int B = large ? 128 : 64;
    pl.kernel = large ? GEMM_K_TILE128 : GEMM_K_TILE64; pl.gx = cdiv(a.N, B); pl.gy = cdiv(a.M, B);
    pl.tiles = pl.gx * pl.gy; pl.splits = large ? 1 : splits; pl.blocks = pl.tiles * pl.splits;
    pl.reduce = !large && splits > 1;
    return pl;
}

// the branch order of the dispatch; `a.f16` already says whether the operands are IEEE half
static inline GemmPlan plan_kernel(bool two_byte, const GemmArgs& a, const GemmTuning& tune) {
    const GemmPlan invalid;
    const int variant = a.variant;
    const bool skinny = (variant == GEMM_SKINNY) || (variant == GEMM_AUTO && a.M <= 64);
    const bool large = (variant == GEMM_LARGE) || (variant == GEMM_AUTO && a.M >= 256 && a.N >= 128);
    if (two_byte) {
        // the weight-streaming regime above the GEMV's 16 rows: per-frame steps, short chunks (gemm_stream_kernel); slab consumers or the SwiGLU epilogue
        if ((variant == GEMM_AUTO || variant == GEMM_SKINNY || variant == GEMM_STREAM) && stream_ok(MMD_BF16, a)) return plan_stream(a);
        if (variant == GEMM_STREAM) return invalid;
        const bool ring_ok = big_packed_ok(MMD_BF16, a, 16) && (a.N % 32) == 0 && ring_size_ok(a);
        // 256^2 tiles pay once there are ~1.5 block waves of them (every ViT / projector GEMM, gate_up of a >= 600-row chunk)
        if (variant == GEMM_RING256 || (variant == GEMM_AUTO && a.M >= 512 && ring_ok && ring_tiles_ok((long long)cdiv(a.M, 256) * cdiv(a.N, 256)))) {
            if (!ring_ok) return invalid;
            GemmPlan pl = plan_ring(a, a.ring_flags, 1);
            if (variant == GEMM_AUTO) pl.ring_auto = RING_AUTO_PLAIN;
            return pl;
        }
        // long K with under one block wave of 256^2 tiles (down_proj of a chunk): split K across grid.z so ~one block per CU runs a
        // long steady state (1.05 PF at M = 1274 against 0.84 PF for the 128-row kernel's 3-way split); K = 3584 shapes lose to it
        const bool ring_split_ok = ring_ok && a.epi != EPI_SWIGLU && a.splitk_ws != nullptr;
        if (!a.f16 && (variant == GEMM_RING256_SPLIT || (variant == GEMM_AUTO && a.M >= 512 && a.K >= 8192 && ring_split_ok))) {
            if (variant == GEMM_RING256_SPLIT && !ring_ok) return invalid;
            const int sp = ring_split_choice(a);
            if (variant == GEMM_RING256_SPLIT || sp >= 2) {
                GemmPlan pl = plan_ring(a, 16, sp);
                if (variant == GEMM_AUTO) pl.ring_auto = RING_AUTO_SPLIT;
                return pl;
            }
        }
        if (variant >= GEMM_RINGX && variant < GEMM_RINGX + 128) {          // forced ring variants (A/B and parity of every instantiation)
            if (!ring_ok) return invalid;
            const int flags = variant - GEMM_RINGX;
            int sp = 1;
            if (flags & 4) {
                const int slots = (flags & 1) ? 512 : 256, tl = cdiv(a.M, 256) * cdiv(a.N, (flags & 1) ? 128 : 256);
                sp = slots / tl; if (sp < 1) sp = 1;
                while (sp > 1 && a.K / sp < 1024) --sp;
                if (sp < 2) sp = 2;
            }
            return plan_ring(a, flags, sp);
        }
        const bool want_big = variant == GEMM_BIG || (variant == GEMM_AUTO && a.M > 64);
        if (want_big) {
            int bn = 0;
            // 128-wide tiles need ~1.5 block waves to keep two blocks per CU busy; below that 64-wide tiles (3 blocks/CU) win
            // by 8-10 % (measured at M = 980 / 1274, K = 3584); long-K shapes keep 128 and split K instead
            const long long t128 = (long long)cdiv(a.M, 128) * (a.N / 128);
            if (big_packed_ok(MMD_BF16, a, 128) && (t128 >= 400 || (a.K >= 8192 && t128 >= 224))) bn = 128;
            else if (big_packed_ok(MMD_BF16, a, 64)) bn = 64;
            // mid-M (a chunk's qkv / o_proj): once some CU would carry three or more 128-row blocks, one 256x128 ring tile per CU (4-wave ring, flags 17) is the
            // shorter schedule.  Per-CU cost in units of one 128x64 block at two per CU (17.5 us at K = 3584), fitted to tools/probes/midm_ring4w_sweep.py:
            // n blocks of 128x64 cost max(1.83, n), of 128x128 max(2.29, 1.77 n), a 256x128 ring tile 2.95 (M = 1323 qkv 75 -> 51 us, M = 1911 o 63 -> 58 us)
            if (bn && variant == GEMM_AUTO && !a.f16 && a.M >= 512 && a.K >= 1024 && (a.N % 128) == 0 && big_packed_ok(MMD_BF16, a, 16) && ring_size_ok(a)) {
                const long long mt128 = cdiv(a.M, 128);
                const double nb = bn == 64 ? (double)cdiv(mt128 * (a.N / 64), 256) : (double)cdiv(t128, 256);
                const double cbig = bn == 64 ? (nb > 1.83 ? nb : 1.83) : (1.77 * nb > 2.29 ? 1.77 * nb : 2.29);
                const double cr4 = 2.95 * (double)cdiv((long long)cdiv(a.M, 256) * (a.N / 128), 256);
                if (cr4 < 0.8 * cbig)          // (only where the model predicts >= 20 %: inside the model, with each layer's weights cold, the 2-8 % cases of the sweep measured -0.3 %)
                    return plan_ring(a, 17, 1);
            }
            if (bn) return plan_big(a, bn);
            if (variant == GEMM_BIG) return invalid;
        }
        if (a.f16) return invalid;          // IEEE-half operands exist in the ring / big kernels only (the tower's shapes: M >= 65, N % 64 == 0, K % 64 == 0, packed weights)
        if (skinny && skinny_packed_ok(MMD_BF16, a)) {
            if (a.slabs_out && !a.splitk_ws) return invalid;          // slabs need somewhere to go
            if (a.M <= 16 && !a.no_gemv) return plan_gemv16(a, tune);
            if (a.chain) return invalid;          // the decode chain exists in the GEMV kernel only
            return plan_skinny(a, a.M <= 16 ? 1 : (a.M <= 32 ? 2 : 4));
        }
    }
    if (a.slabs_out) return invalid;          // slab mode exists only on the packed skinny path
    if (a.chain) return invalid;
    if (a.W == nullptr) return invalid;       // only the packed copy exists but the shape needs the generic path
    return plan_tile(a, skinny, large);
}

// The dispatch decision for launch_gemm(dtype, a, ...).  Pure: every pointer of `a` counts as null / non-null / aligned only (`chain` excepted: its two form fields are read).
static inline GemmPlan gemm_plan(int dtype, const GemmArgs& a, const GemmTuning& tune) {
    if (dtype == MMD_F16 && !a.f16) { GemmArgs h = a; h.f16 = 1; return gemm_plan(dtype, h, tune); }          // 2-byte storage either way; the kernels' F16 forms read the bits as IEEE half
    GemmPlan pl;
    if (a.M <= 0 || a.N <= 0) { pl.kernel = GEMM_PLAN_EMPTY; return pl; }
    pl = plan_kernel(dtype != MMD_F32, a, tune);
    if (!pl.valid()) return pl;
    // a piece-major operand exists for the ring kernel only, where the automatic dispatch chooses it (the caller asks gemm_ring_auto first) ...
    if ((a.x_pm || a.y_pm) && (pl.ring_auto == RING_AUTO_NONE || a.wscale || (a.x_pm && (a.K % 32)) || (a.y_pm && ((a.epi == EPI_SWIGLU ? a.N / 2 : a.N) % 32)))) return GemmPlan();
    // ... and a piece-major OUTPUT for its plain form only: the split-K form leaves fp32 slabs and splitk_reduce writes Y row-major
    if (a.y_pm && pl.ring_auto != RING_AUTO_PLAIN) return GemmPlan();
    const bool streaming = pl.kernel == GEMM_K_GEMV16 || pl.kernel == GEMM_K_SKINNY || pl.kernel == GEMM_K_STREAM;
    pl.prof_class = streaming || (pl.kernel == GEMM_K_TILE64 && a.M <= 64) ? MMD_K_GEMM_SKINNY : MMD_K_GEMM_TILE;
    return pl;
}
