// attn_plan.h -- the attention dispatch decision of the library, and nothing else: which kernel runs, in which instantiation, over which grid, with how many key splits,
// and which merge launch follows.  Two pure host functions, attn_plan() and attn_plan_decode_multi(): no GPU header, no runtime call, no environment; they compile with the
// host C++17 compiler alone (tests/test_attn_plan_host.py runs the regime table of tests/attn_regimes.py through them without a GPU).  launch_attention /
// launch_attention_decode_multi (attn.hip) evaluate them once per launch and launch what they say.  Every threshold and every rejection of the dispatch lives here.
#pragma once
#include "gemm_plan.h"          // cdiv, round_up, MMD_F16

struct StepState;               // (common.h) the planner only tests the pointers for null

struct AttnArgs {
    const void* q; int64_t ldq;      // [S, nh*d] row stride ldq
    const void* K; const void* V;    // element (kv head h, token t, e) at K + h*k_hs + t*k_ts + e
    int64_t k_hs, k_ts, v_hs, v_ts;  // arena: hs = cap*d, ts = d ; fused ViT qkv rows: hs = d, ts = 3C
    int v_transposed;                // V arena stored transposed in 64-token blocks (see attn.hip); v_ts unused then
    void* out; int64_t ldo;          // [S, nh*d]
    int S, nh, nkv, d;
    int64_t n_ctx;                   // keys before this step; total keys = n_ctx + S
    int causal;
    int batch; int64_t q_bstride, kv_bstride, o_bstride;   // ViT: batch of independent sequences (elements)
    float* ws; size_t ws_bytes;      // split-KV partials
    int variant;
    const StepState* dyn; int layer; int dyn_splits;   // graph mode (attn_gqa128 only)
    // decode steps (rows <= 64, attn_gqa128<1> only): q / k / v are still the qkv projection's fp32 K-slabs.  The attention kernel itself reduces
    // them (+ bias), applies RoPE from the step's (cos, sin) table, builds its q fragments in registers and -- the block whose key range holds a new
    // position -- appends that token's K row / V column to the arena before staging the tile: no slab_rope_append launch, no q buffer.
    const float* qkv_slabs = nullptr; int n_slabs = 0; const void* qkv_bias = nullptr; const void* rope_tab = nullptr;   // slabs [n][slab_rows][(nh+2nkv)*d] (this step's first row); tab float2 [S][d/2]
    int slab_rows = 0;               // rows of one slab = the projection's M (0: S); larger than S when one GEMV served several streams' rows (mmd_round_multi)
    const StepState* segs = nullptr; int nseg = 0;   // launch_attention_decode_multi: the streams' (context length, capacity, arena base), device
    int* plan_out = nullptr;         // if set: int[2] = {form, key splits} of this launch (mmd_op_attention_last_form; {0, 1}: no kernel takes the arguments)
};

// what the decision depends on besides its arguments: the two A/B switches
struct AttnTuning {
    bool decode_ring = true;         // decode geometry on the four-slot ring (MMDUET_ATTN_DECODE_RING=0: the two-slot form)
    bool vit_ring = true;            // d = 72 non-causal on attn_d72_ring_kernel (MMDUET_VIT_ATTN_RING=0: the register-staged attn_rowmajor_kernel<3, 5>)
};

enum { ATTN_PLAN_INVALID = -1,       // no kernel takes these arguments: the launcher returns an invalid-value error
       ATTN_PLAN_EMPTY = -2 };       // S <= 0: nothing to launch
enum { ATTN_K_SIMPLE = 0, ATTN_K_MFMA = 1, ATTN_K_ROWMAJOR = 2, ATTN_K_D72_RING = 3, ATTN_K_GQA128 = 4, ATTN_K_GQA128_W1 = 5, ATTN_K_GQA128_CHUNK = 6 };
enum { ATTN_MERGE_NONE = 0, ATTN_MERGE_GENERIC = 1 /* attn_combine_kernel<DP> */, ATTN_MERGE_ROWS = 2 /* attn_combine128_rows_kernel */, ATTN_MERGE_128 = 3 /* attn_combine128_kernel */,
       ATTN_MERGE_CHUNK = 4 /* attn_combine128_chunk_kernel */ };

// unit geometry of attn_gqa128_chunk_kernel (attn_chunk.h): start[bx] = key tiles of the units 0 .. bx - 1 of one kv head (start[qblocks] = tiles per kv head); built here once
// per launch, rides in the kernel argument (the attention kernel and the merge read it with scalar loads: recomputing it per wave cost the merge 280 us at 35 k rows)
constexpr int CHUNK_TAB = 128, CHUNK_UNITS = 512;
struct ChunkTab { int qblocks; int start[CHUNK_TAB + 1]; unsigned short b0[CHUNK_UNITS], b1[CHUNK_UNITS]; };          // b0 / b1[kvh * qblocks + bx]: first / last block that shares the unit

// Everything a launcher needs: it maps these integers to a template instantiation and launches, and computes nothing itself.
struct AttnPlan {
    int form = ATTN_PLAN_INVALID;    // 1 .. 9 as mmd_op_attention_last_form reports it (tests/test_gpu_stress_attention.py lists them), or ATTN_PLAN_INVALID / ATTN_PLAN_EMPTY
    int kernel = ATTN_K_SIMPLE;      // ATTN_K_*
    int dp = 0;                      // attn_mfma_kernel<DP> and its attn_combine_kernel<DP>
    int nc = 0, dvt = 0; bool exact = false, f16 = false;          // attn_rowmajor_kernel<NC, DVT, F16, EXACT>; f16 also: attn_d72_ring_kernel<F16>
    bool f32 = false;                // attn_simple_kernel<float> (else <bf16_t>)
    int rt = 0, nslot = 0, waves = 0;                              // attn_gqa128_kernel<RT, NSLOT, WAVES>
    int gx = 0, gy = 1, gz = 1, threads = 0, lds = 0;              // grid, block, dynamic LDS bytes
    int splits = 1, kv_per_split = 0, block_rows = 0;              // AttnP::splits (chunk form: the most parts a unit may have) / kv_per_split / block_rows
    long long ws_ml_off = -1;        // floats from AttnArgs::ws to the (m, l) statistics behind the partials (AttnP::ws_ml; ws_o = ws); -1: the kernel writes no partials
    int merge = ATTN_MERGE_NONE, merge_gx = 0, merge_rows = 0;     // the merge launch that follows, its grid and its row-count argument
    int nb = 0;                      // chunk form: blocks of the contiguous decomposition (= gx; the merge kernel's second argument)
    ChunkTab tab;                    // chunk form only (left unset otherwise)
    bool valid() const { return form > 0; }
};

// ---- shared pieces ------------------------------------------------------------------------------------------------------------------------------------------
// the workspace clamp: `n` fp32 partials of `width` floats plus (m, l) for each of rows_all rows
static inline bool attn_ws_fits(int n, size_t rows_all, int width, size_t ws_bytes) { return (size_t)n * rows_all * (width + 2) * sizeof(float) <= ws_bytes; }
static inline int attn_ws_clamp(int n, int least, size_t rows_all, int width, size_t ws_bytes) {
    while (n > least && !attn_ws_fits(n, rows_all, width, ws_bytes)) --n;
    return n;
}
// split-KV choice of the GQA-128 kernels by a small cost model (units: one key tile of one resident block, ~2.6 us with two 128-row blocks per CU): the grid runs in rounds of
// `resident` blocks, a block costs its tiles plus ~2 tiles of prologue / epilogue, and the merge kernel reads splits x rows x 520 B.  Never below 2 tiles per split.
// Measured against it at S = 49 / 392 / 1274, n = 15 k (two-slot form, resident 512): picks 42 / 5 / 7 splits (33 / 152 / 440 us; the old fixed target of 576 blocks gave
// 42 / 202 / 485 us).  (A 256-row block's tile costs about what two resident 128-row blocks' tiles do: swept 1.0 .. 2.6, flat.)
static inline int attn_max_splits(int tiles) { int maxs = tiles / 2; if (maxs < 1) maxs = 1; if (maxs > 64) maxs = 64; return maxs; }
static inline int attn_cost_splits(int blocks, int tiles, double rows_all, int maxs, int resident) {
    int splits = 1; double best = 1e30;
    for (int sp = 1; sp <= maxs; ++sp) {
        const double rounds = (double)cdiv((long long)blocks * sp, resident);
        const double cost = rounds * ((double)cdiv(tiles, sp) + 2.0) + (sp > 1 ? sp * rows_all * 6.7e-5 + 1.5 : 0.0);
        if (cost < best - 1e-9) { best = cost; splits = sp; }
    }
    return splits;
}

// ---- attn_gqa128_chunk_kernel: host side of the kernel's integer formulas -----------------------------------------------------------------------------------
// key tiles per unit, total, and the most blocks that share one unit
static inline int chunk_unit_tiles_host(int rows_total, int G, long long n_ctx, int S, int causal, int bx) {
    const int last_row = (bx * 256 + 255 < rows_total - 1) ? bx * 256 + 255 : rows_total - 1;
    const long long n_tot = n_ctx + S;
    long long lim = causal ? n_ctx + (long long)(last_row / G) + 1 : n_tot;
    if (lim > n_tot) lim = n_tot;
    return (int)((lim + 63) >> 6);
}
static inline int chunk_block_of_host(long long W, int nb, long long tile) {
    int b = (int)((tile * nb) / W);
    while (b + 1 < nb && (W * (b + 1)) / nb <= tile) ++b;
    while (b > 0 && (W * b) / nb > tile) --b;
    return b;
}
// linear tiles per block of the contiguous decomposition (the dispatcher's criterion: short ranges pay a q load / pipeline fill / partial per segment)
static inline long long chunk_tiles_total(const AttnArgs& a) {
    const int G = a.nh / a.nkv, rows_total = a.S * G, qblocks = cdiv(rows_total, 256);
    long long W1 = 0;
    for (int b = 0; b < qblocks; ++b) W1 += chunk_unit_tiles_host(rows_total, G, a.n_ctx, a.S, a.causal, b);
    return W1 * a.nkv;
}
// the contiguous (stream-K) decomposition; false (pl untouched but for its table): it does not fit -- table sizes, parts per unit, workspace
static inline bool plan_gqa128_chunk(AttnPlan& pl, const AttnArgs& a) {
    const int G = a.nh / a.nkv, rows_total = a.S * G, qblocks = cdiv(rows_total, 256);
    if (qblocks > CHUNK_TAB || qblocks * a.nkv > CHUNK_UNITS) return false;
    ChunkTab& tab = pl.tab; tab.qblocks = qblocks; tab.start[0] = 0;
    long long W1 = 0; int tmax = 0;
    for (int b = 0; b < qblocks; ++b) { const int t = chunk_unit_tiles_host(rows_total, G, a.n_ctx, a.S, a.causal, b); W1 += t; if (t > tmax) tmax = t; tab.start[b + 1] = (int)W1; }
    for (int b = qblocks + 1; b <= CHUNK_TAB; ++b) tab.start[b] = (int)W1;
    const long long W = W1 * a.nkv;
    int nb = 256; if (W < nb) nb = (int)W;
    const int nrows_all = a.nkv * rows_total;
    for (int k = 0; k < a.nkv; ++k)
        for (int b = 0; b < qblocks; ++b) {
            const long long us = (long long)k * W1 + tab.start[b];
            tab.b0[k * qblocks + b] = (unsigned short)chunk_block_of_host(W, nb, us);
            tab.b1[k * qblocks + b] = (unsigned short)chunk_block_of_host(W, nb, us + (tab.start[b + 1] - tab.start[b]) - 1);
        }
    // without a workspace every unit must be whole: one block per unit; with one, bound the parts per unit by the workspace
    const int parts_max = (int)(tmax / (W / nb)) + 2;
    if (!a.ws || parts_max > 64 || !attn_ws_fits(parts_max, (size_t)nrows_all, 128, a.ws_bytes)) return false;
    pl.form = 8; pl.kernel = ATTN_K_GQA128_CHUNK;
    pl.gx = nb; pl.gy = 1; pl.gz = 1; pl.threads = 512; pl.lds = 4 * 32768; pl.nb = nb;
    pl.splits = parts_max; pl.kv_per_split = 0;
    pl.ws_ml_off = (long long)((size_t)parts_max * nrows_all * 128);
    pl.merge = ATTN_MERGE_CHUNK; pl.merge_gx = cdiv(nrows_all, 4); pl.merge_rows = nrows_all;
    return true;
}

// ---- attn_gqa128_w1_kernel (attn_w1.h) ----------------------------------------------------------------------------------------------------------------------
// geometry for `rows_total` stacked rows per kv head: the fewest row blocks (<= 256 rows each), balanced in whole 16-row tiles; key splits by the cost model with one
// block per CU resident.  (The cost model may pick up to tiles / 2 <= 64 splits; the workspace trims its CHOICE here, where the grid forms trim the search range.)
static inline void plan_gqa128_w1(AttnPlan& pl, const AttnArgs& a) {
    const int G = a.nh / a.nkv, rows_total = a.S * G;
    const int row_tiles = cdiv(rows_total, 16);
    const int qblocks = cdiv(row_tiles, 16);
    const int block_rows = cdiv(row_tiles, qblocks) * 16;
    const long long n_tot = a.n_ctx + a.S;
    const int tiles = cdiv(n_tot, 64);
    const int blocks = qblocks * a.nkv;
    int splits = attn_cost_splits(blocks, tiles, (double)a.nkv * rows_total, attn_max_splits(tiles), 256);
    if (!a.ws) splits = 1;
    splits = attn_ws_clamp(splits, 1, (size_t)a.nkv * rows_total, 128, a.ws_bytes);
    const int per = cdiv(tiles, splits) * 64;
    splits = cdiv(n_tot, per);
    const int nrows_all = a.nkv * rows_total;
    pl.form = 5; pl.kernel = ATTN_K_GQA128_W1;
    pl.gx = qblocks; pl.gy = a.nkv; pl.gz = splits; pl.threads = 512; pl.lds = 4 * 32768;
    pl.splits = splits; pl.kv_per_split = per; pl.block_rows = block_rows;
    pl.ws_ml_off = (long long)((size_t)splits * nrows_all * 128);
    if (splits > 1) { pl.merge = ATTN_MERGE_128; pl.merge_gx = cdiv(nrows_all, 4); pl.merge_rows = nrows_all; }
}

// ---- attn_gqa128_kernel<RT, NSLOT, WAVES>: the (row block, kv head, key split) grid forms, and the chunk rule ------------------------------------------------
static inline void plan_gqa128(AttnPlan& pl, const AttnArgs& a, const AttnTuning& tune, int RT) {
    const int G = a.nh / a.nkv, rows_total = a.S * G;
    // chunks (>= 1024 rows per kv head): 256-row blocks, one per CU, four-slot ring
    const bool chunk8 = RT == 2 && rows_total >= 1024;
    const int qblocks = cdiv(rows_total, chunk8 ? 256 : 64 * RT);
    const int resident = chunk8 ? 256 : 512;                       // blocks the chip holds at once
    const long long n_tot = a.n_ctx + a.S;
    const int blocks = qblocks * a.nkv;
    const int tiles = cdiv(n_tot, 64);
    int splits = 1;
    if (a.dyn) {
        splits = a.dyn_splits;                                     // fixed grid under graph replay; empty splits write (m = -inf, l = 0)
    } else if (rows_total <= 16 && a.ws) {
        splits = 64;                                               // decode: same key ranges as the graph-replayed form -> identical bits
        if (splits > tiles) splits = tiles;
    } else if (a.ws) {
        const int maxs = attn_ws_clamp(attn_max_splits(tiles), 1, (size_t)a.nkv * rows_total, 128, a.ws_bytes);
        splits = attn_cost_splits(blocks, tiles, (double)a.nkv * rows_total, maxs, resident);
    }
    // chunks: the contiguous (stream-K) decomposition of attn_chunk.h where the (unit, key split) grid is a bad fit -- it needs splits to fill the chip (each split is one more
    // fp32 partial per row) or leaves a fifth of it idle -- and a block's range is long enough to carry its per-segment costs (>= 14 tiles; 40+ units).  Measured against
    // the grid form over S = 147 .. 1911, 0 .. 30 k keys (profiles/r05_attention_chunk.md): 1.04 - 1.39 x where this rule takes it, the grid form elsewhere.
    if (chunk8 && a.variant == 0 && !a.dyn && a.ws && blocks >= 40) {
        const double eff = (double)blocks * splits / ((double)cdiv((long long)blocks * splits, resident) * resident);
        if (chunk_tiles_total(a) / 256 >= 14 && !(splits == 1 && eff >= 0.8) && plan_gqa128_chunk(pl, a)) return;          // (it does not fit: the grid form)
    }
    const int per = cdiv(tiles, splits) * 64;
    if (!a.dyn) splits = cdiv(n_tot, per);
    const int nrows_all = a.nkv * rows_total;
    pl.form = RT == 1 ? 3 : 4; pl.kernel = ATTN_K_GQA128;
    pl.gx = qblocks; pl.gy = a.nkv; pl.gz = splits;
    pl.splits = splits; pl.kv_per_split = per;
    pl.ws_ml_off = (long long)((size_t)splits * nrows_all * 128);
    if (RT == 1 && qblocks == 1 && a.nkv * splits <= 256 && rows_total <= 16 && tune.decode_ring) {
        pl.rt = 1; pl.nslot = 4; pl.waves = 4; pl.threads = 256; pl.lds = 4 * 32768;          // decode geometry (one query block per kv head, at most one block per CU): the four-slot ring
    } else if (chunk8) {
        pl.rt = 2; pl.nslot = 4; pl.waves = 8; pl.threads = 512; pl.lds = 4 * 32768;
    } else {
        pl.rt = RT; pl.nslot = 2; pl.waves = 4; pl.threads = 256; pl.lds = 2 * 32768;
    }
    if (splits > 1) {
        pl.merge_rows = nrows_all;
        if (nrows_all <= 64 && splits <= 64) { pl.merge = ATTN_MERGE_ROWS; pl.merge_gx = nrows_all; }
        else { pl.merge = ATTN_MERGE_128; pl.merge_gx = cdiv(nrows_all, 4); }
    }
}

// ---- attn_mfma_kernel<DP>: any head_dim <= 128 (DP = its multiple of 32), 64-row blocks, key splits towards 512 blocks -----------------------------------------
static inline void plan_mfma(AttnPlan& pl, const AttnArgs& a) {
    const int DP = a.d <= 32 ? 32 : (a.d <= 64 ? 64 : (a.d <= 96 ? 96 : 128));
    const int G = a.nh / a.nkv, rows_total = a.S * G, qtiles = cdiv(rows_total, 64), by = a.nkv * a.batch, blocks = qtiles * by;
    const long long n_tot = a.n_ctx + a.S;
    int splits = 1;
    if (blocks < 256) {
        int want = cdiv(512, blocks);
        int maxs = (int)(n_tot / 256); if (maxs < 1) maxs = 1;
        splits = want < maxs ? want : maxs;
        if (splits > 64) splits = 64;
        if (a.ws == nullptr) splits = 1;
        splits = attn_ws_clamp(splits, 1, (size_t)by * rows_total, DP, a.ws_bytes);
    }
    const int per = (int)round_up(cdiv(n_tot, splits), 32);
    splits = cdiv(n_tot, per);
    const int nrows_all = by * rows_total;
    pl.form = 2; pl.kernel = ATTN_K_MFMA; pl.dp = DP;
    pl.gx = qtiles; pl.gy = by; pl.gz = splits; pl.threads = 256; pl.lds = 0;
    pl.splits = splits; pl.kv_per_split = per;
    pl.ws_ml_off = (long long)((size_t)splits * nrows_all * DP);
    if (splits > 1) { pl.merge = ATTN_MERGE_GENERIC; pl.merge_gx = nrows_all; pl.merge_rows = nrows_all; }
}

// ---- the dispatch ---------------------------------------------------------------------------------------------------------------------------------------------
static inline void plan_attention(AttnPlan& pl, int dtype, const AttnArgs& a, const AttnTuning& tune) {
    const bool f16 = dtype == MMD_F16;          // the fp16 vision tower: the row-major kernel only
    bool can_mfma = (dtype == MMD_BF16 || f16) && (a.d % 8) == 0 && a.d <= 128 && (a.ldq % 8) == 0 && (a.k_ts % 8) == 0 && (a.v_ts % 8) == 0 &&
                    (a.k_hs % 8) == 0 && (a.v_hs % 8) == 0 && (a.kv_bstride % 8) == 0 && (a.q_bstride % 8) == 0;
    int variant = a.variant;
    const bool can_gqa128 = can_mfma && a.d == 128 && a.v_transposed && a.batch == 1 && a.k_ts == 128;
    // token-major K/V rows (ViT fused qkv): the transpose-read kernel; it keeps a whole sequence per (head, batch) block
    const bool can_rowmajor = can_mfma && !a.v_transposed && a.n_ctx + a.S < (1 << 30) && (a.o_bstride % 4) == 0 && (a.ldo % 4) == 0 &&
                              (a.n_ctx + a.S) * (a.k_ts > a.v_ts ? a.k_ts : a.v_ts) < (1ll << 31);          // (its staging loads address a sequence with 32-bit element offsets)
    if (variant == 0) variant = can_gqa128 ? 3 : (can_rowmajor && a.S >= 64 ? 4 : (can_mfma ? 2 : 1));
    if (a.qkv_slabs && variant != 3) return;
    if (f16 && variant != 4) return;
    if (variant == 4) {
        if (!can_rowmajor) return;
        pl.form = 6; pl.kernel = ATTN_K_ROWMAJOR; pl.f16 = f16;
        pl.gx = cdiv(a.S, 128); pl.gy = a.nh; pl.gz = a.batch; pl.threads = 256; pl.lds = 0;
        pl.splits = 1; pl.kv_per_split = 0;
        if (a.d <= 32) { pl.nc = 1; pl.dvt = 2; return; }
        if (a.d <= 64) { pl.nc = 2; pl.dvt = 4; return; }
        if (a.d == 72 && !a.causal && (a.k_ts % 8) == 0 && (a.v_ts % 8) == 0 && (a.k_hs % 8) == 0 && (a.v_hs % 8) == 0 && (a.kv_bstride % 8) == 0 &&
            ((uintptr_t)a.K % 16) == 0 && ((uintptr_t)a.V % 16) == 0 && ((uintptr_t)a.q % 16) == 0 && (a.ldq % 8) == 0 && (a.q_bstride % 8) == 0 && a.n_ctx + a.S > 0 && tune.vit_ring) {
            // SigLIP-so400m, bidirectional: K / V tiles by LDS-DMA into two slots, four blocks per CU
            pl.form = 7; pl.kernel = ATTN_K_D72_RING; pl.lds = 2 * 2 * 10 * 512 * 2;
            return;
        }
        if (a.d > 64 && a.d <= 80) { pl.nc = 3; pl.dvt = 5; pl.exact = true; return; }          // SigLIP-so400m: 72 -> five 16-wide output tiles, known at compile time
        if (a.d <= 96) { pl.nc = 3; pl.dvt = 6; return; }
        pl.nc = 4; pl.dvt = 8;
        return;
    }
    if (variant == 2 && !can_mfma) return;
    if (variant == 6) {          // the chunk kernel's contiguous decomposition, forced (attn_chunk.h)
        if (!can_gqa128 || a.qkv_slabs || a.dyn || a.S * (a.nh / a.nkv) < 256) return;
        plan_gqa128_chunk(pl, a);
        return;
    }
    if (variant == 5) {          // software-pipelined waves, balanced row blocks (attn_w1.h)
        if (!can_gqa128 || a.qkv_slabs || a.dyn) return;
        plan_gqa128_w1(pl, a);
        return;
    }
    if (variant == 3) {
        if (!can_gqa128) return;
        const int rows_total = a.S * (a.nh / a.nkv);
        if (a.qkv_slabs && (rows_total > 64 || a.k_ts != 128 || a.n_slabs < 1 || a.n_slabs > 4)) return;        // the fused q/k/v preparation lives in the decode form only
        // per-frame steps and short chunks over a long context (17 .. 768 stacked rows per kv head, >= 64 key tiles): attn_gqa128_w1_kernel -- two balanced row blocks of whole
        // 16-row tiles instead of three 128-row blocks, one block per CU on the four-slot ring (S = 49 over 15 k keys: 31.6 -> 27.7 us incl. the merge; below 4 k keys its
        // longer pipeline fill loses 2-20 %, from 1 k rows up the 256-row phase-split form is 8 % faster: profiles/r05_attn_small_s.md)
        if (a.variant == 0 && !a.qkv_slabs && !a.dyn && rows_total > 16 && rows_total <= 768 && a.n_ctx + a.S >= 4096 && a.ws) { plan_gqa128_w1(pl, a); return; }
        plan_gqa128(pl, a, tune, rows_total <= 64 ? 1 : 2);
        return;
    }
    if (variant == 1) {
        if (a.d > 128) return;
        pl.form = 1; pl.kernel = ATTN_K_SIMPLE; pl.f32 = dtype == MMD_F32;
        pl.gx = a.S; pl.gy = a.nh; pl.gz = a.batch; pl.threads = 64; pl.lds = 0;
        pl.splits = 1; pl.kv_per_split = 0;
        return;
    }
    plan_mfma(pl, a);
}

// The dispatch decision for launch_attention(dtype, a, ...).  Pure: every pointer of `a` counts as null / non-null / aligned only.
static inline AttnPlan attn_plan(int dtype, const AttnArgs& a, const AttnTuning& tune) {
    AttnPlan pl;
    if (a.S <= 0) pl.form = ATTN_PLAN_EMPTY;
    else plan_attention(pl, dtype, a, tune);
    return pl;
}

// ... and for launch_attention_decode_multi(a, ...) (form 9): decode rows of SEVERAL streams in one launch, grid.x = stream, each stream's keys cut into the same number of
// splits so that nseg x nkv x splits blocks fill the chip once (one stream alone: 64 splits of ~4 tiles at 15 k keys; four streams: 16 splits of ~15 tiles -- a quarter of
// the launches, partial rows and merge work per token).  bf16, head_dim 128, S x G <= 16.
static inline AttnPlan attn_plan_decode_multi(const AttnArgs& a) {
    AttnPlan pl;
    const int G = a.nh / a.nkv, rows_total = a.S * G;
    if (a.nseg < 1 || a.nseg > 64 || !a.segs || a.d != 128 || !a.v_transposed || a.k_ts != 128 || rows_total > 16 || !a.ws || a.nseg * a.nkv > 256) return pl;
    if (a.qkv_slabs && (a.n_slabs < 1 || a.n_slabs > 4)) return pl;
    int splits = 256 / (a.nseg * a.nkv);
    if (splits > 64) splits = 64;
    if (splits < 2) splits = 2;                    // (the merge kernel writes the output: at least two partials keep one code path; > 32 streams per round never occur)
    const int nrows_all = a.nkv * rows_total;
    splits = attn_ws_clamp(splits, 2, (size_t)a.nseg * nrows_all, 128, a.ws_bytes);
    if (!attn_ws_fits(splits, (size_t)a.nseg * nrows_all, 128, a.ws_bytes) || a.nseg * a.nkv * splits > 512) return pl;
    pl.form = 9; pl.kernel = ATTN_K_GQA128; pl.rt = 1; pl.nslot = 4; pl.waves = 4;
    pl.gx = a.nseg; pl.gy = a.nkv; pl.gz = splits; pl.threads = 256; pl.lds = 4 * 32768;
    pl.splits = splits; pl.kv_per_split = 0;       // (per stream, computed in the kernel from its own context length -- the dyn path)
    pl.ws_ml_off = (long long)((size_t)a.nseg * splits * nrows_all * 128);
    pl.merge = ATTN_MERGE_ROWS; pl.merge_gx = a.nseg * nrows_all; pl.merge_rows = nrows_all;
    return pl;
}
