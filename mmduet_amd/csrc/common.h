// common.h -- shared device helpers and the internal launcher interface of libmmduet_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/mmduet.h"
#include "gemm_plan.h"          // GemmArgs, GemmPlan and the dispatch decision (host-only: no GPU header), cdiv / round_up, MMD_F16
#include "attn_plan.h"          // AttnArgs, AttnPlan and the attention dispatch decision (host-only too)
#include "response_plan.h"      // CONS_MAX_TABLE / CONS_MAX_EOS / LP_MAX_TOP: the limits of a response's constraint set and records (host-only too)

typedef uint16_t bf16_t;   // raw bfloat16 storage

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(2))) short s16x2_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

#define WAVE 64

__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {            // round-to-nearest-even (v_cvt_pk_bf16_f32)
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(bf16_t, b);
}
// ---- fp16 storage of the vision tower (config tower_dtype = fp16: the reference runs the tower under torch.cuda.amp.autocast(), models/modeling_live.py:28) ----
typedef _Float16 f16_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_t;
__device__ __forceinline__ float h2f(uint16_t r) { return (float)__builtin_bit_cast(_Float16, r); }
__device__ __forceinline__ uint16_t f2h(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }          // round-to-nearest-even (v_cvt_f16_f32)
// raw 16-bit storage <-> float for kernels that move 2-byte elements as integer vectors
template <bool F16> __device__ __forceinline__ float raw2f(uint16_t r) { if constexpr (F16) return h2f(r); else return __uint_as_float(((uint32_t)r) << 16); }
template <typename T> __device__ __forceinline__ float to_f(T v);
template <> __device__ __forceinline__ float to_f<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f<bf16_t>(bf16_t v) { return bf2f(v); }
template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t from_f<bf16_t>(float v) { return f2bf(v); }
template <> __device__ __forceinline__ float to_f<f16_t>(f16_t v) { return (float)v; }
template <> __device__ __forceinline__ f16_t from_f<f16_t>(float v) { return (f16_t)v; }
template <bool F16> __device__ __forceinline__ uint16_t f2raw(float f) { if constexpr (F16) return f2h(f); else return f2bf(f); }
// one MFMA of the 2-byte GEMM / attention kernels: operands travel as raw 16-byte fragments, the instruction decides what the bits mean (same rate, same layouts)
template <bool F16> __device__ __forceinline__ f32x4_t mfma16(const bf16x8_t& a, const bf16x8_t& b, const f32x4_t& c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// round a float through the storage type (the rounding points of eager bf16 execution)
template <typename T> __device__ __forceinline__ float rnd(float v) { return to_f<T>(from_f<T>(v)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float gelu_tanh_f(float x) {
    const float k = 0.7978845608028654f;   // sqrt(2/pi)
    return 0.5f * x * (1.0f + tanhf(k * (x + 0.044715f * x * x * x)));
}
__device__ __forceinline__ float gelu_erf_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.7071067811865476f)); }
__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + __expf(-x)); }
// fast forms for the bf16 path (error <= 2e-7 abs, far below bf16 resolution): raw v_exp_f32 / v_rcp_f32
__device__ __forceinline__ float gelu_tanh_fast(float x) {
    // 0.5 x (1 + tanh(u)) = x sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3):  2u log2(e) = x (A + B x^2).  Seven vector instructions (two transcendental) where the
    // 1 - 2 / (exp(2u) + 1) form took eleven -- the GELU epilogue is a fifth of fc1's tile time (K = 1152: 36 slices of MFMAs, then 128 elements per lane) --, and no
    // cancellation for very negative x; saturates correctly at +-inf (exp2 -> inf: rcp -> 0; exp2 -> 0: x).
    const float A = 2.3022081983f, B = 0.10294324f;            // 2 sqrt(2/pi) log2(e), A * 0.044715
    const float z = x * fmaf(x * x, B, A);
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-z));
}
__device__ __forceinline__ float gelu_erf_fast(float x) {
    // erf via Abramowitz-Stegun 7.1.26 (|err| <= 1.5e-7)
    float z = fabsf(x) * 0.7071067811865476f;
    float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * z);
    float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    float er = 1.0f - poly * __builtin_amdgcn_exp2f(-z * z * 1.4426950408889634f);
    er = x < 0.f ? -er : er;
    return 0.5f * x * (1.0f + er);
}
template <typename T> __device__ __forceinline__ float gelu_tanh_t(float x) { if constexpr (sizeof(T) == 2) return gelu_tanh_fast(x); else return gelu_tanh_f(x); }
template <typename T> __device__ __forceinline__ float gelu_erf_t(float x) { if constexpr (sizeof(T) == 2) return gelu_erf_fast(x); else return gelu_erf_f(x); }
template <typename T> __device__ __forceinline__ float silu_t(float x) {
    if constexpr (sizeof(T) == 2) return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-x * 1.4426950408889634f)); else return silu_f(x);
}

static inline size_t dtype_size(int dt) { return dt == MMD_F32 ? 4 : 2; }

// device-resident state of a graph-captured decode step (updated by the last kernel of the graph)
struct StepState { long long n_ctx; long long cap; void* K; void* V; int n_prev; int step; long long pos_off; };          // step: index of the decode step within its generate call (the slot of its log-probability record); pos_off: RoPE position of slot n_ctx minus n_ctx (tokens dropped by mmd_kv_drop)

// ---- the GEMM family (arguments, epilogues, kernel ids and the dispatch decision: gemm_plan.h) ---------------------------
const GemmTuning& gemm_tuning();          // the process's GemmTuning (MMDUET_GEMV_KSPLIT_SHORT, read once)
GemmPlan gemm_plan_for(int dtype, const GemmArgs& a);          // gemm_plan with the process's GemmTuning: what launch_gemm(dtype, a, ...) would launch
bool gemm_can_slab(int dtype, const GemmArgs& a);          // would a weight-streaming kernel leave X . W^T as fp32 K slabs in splitk_ws (GemmArgs::slabs_out)?
bool gemm_ring_auto(int dtype, const GemmArgs& a, bool plain_only = false);          // would the automatic dispatch run this GEMM on gemm_ringx_kernel (plain or split-K; plain_only: not the split-K form)?  (what a piece-major operand needs; a piece-major OUTPUT needs the plain form)

// launchers (dtype = mmd_dtype).  All return hipError_t of the launch.
hipError_t launch_gemm(int dtype, const GemmArgs& a, hipStream_t st, const GemmPlan* planned = nullptr);          // planned: gemm_plan_for(dtype, a), if the caller already asked (it is evaluated once per GEMM)
hipError_t launch_pack_w(const void* W, int64_t ldw, int N, int K, void* out, hipStream_t st);   // bf16 only, N%16==0, K%32==0
// fp8 e4m3 (OCP) weights, one scale per output channel: W [N,K] bf16 row-major is REPLACED by bf16(q) (q = rne_fp8(W / scale), scale = amax / 448),
// q8_rowmajor [N,K] bytes and scale [N] fp32 are written;  launch_pack_w8 lays q8 out fragment-major for the streaming kernels (N%16==0, K%64==0)
hipError_t launch_quantize_fp8_rows(void* W_bf16, int N, int K, uint8_t* q8_rowmajor, float* scale, hipStream_t st);
hipError_t launch_pack_w8(const uint8_t* q8_rowmajor, int N, int K, void* out, hipStream_t st);
hipError_t launch_rmsnorm(int dtype, const void* x, const void* w, void* y, int M, int H, float eps, hipStream_t st);
hipError_t launch_layernorm(int dtype, const void* x, const void* w, const void* b, void* y, int M, int H, float eps, hipStream_t st);
hipError_t launch_resid32_layernorm(const void* y16, float* h32, const void* pos16, int period, const void* ln_w, const void* ln_b, void* out16, void* outbf,
                                    int M, int H, float eps, hipStream_t st);          // the autocast tower's fp32 residual stream (ops.hip)
// fused consumers of skinny-GEMM slabs (ops.hip)
hipError_t launch_slab_resid_rmsnorm(const float* slabs, int splits, int M, int H, const void* resid_in, void* h_out, const void* norm_w, float eps,
                                     void* xn_out, hipStream_t st, const float* wscale = nullptr);
int slab_resid_maxs(int splits);          // the instantiation (slabs a thread loads before its first add: 4, 8 or 16) that launch_slab_resid_rmsnorm runs for `splits`
constexpr int OP_PLAN_SLAB_RESID = 32;    // mmd_op_gemm_last_plan after mmd_op_slab_resid_rmsnorm: {this, instantiation, splits, blocks = M} (no GEMM_K_* value)
hipError_t launch_slab_rope_append(const float* slabs, int splits, const void* bias, int S, int nh, int nkv, int d, const float* inv_freq_dev,
                                   int64_t pos0, void* q_out, void* Kc, void* Vc, int64_t cap, hipStream_t st, const StepState* dyn = nullptr, int layer = 0,
                                   int slab_rows = 0, int64_t pos_off = 0);          // slab_rows: rows of one slab when the projection ran over more rows than this stream's S (0 = S); `slabs` points at the stream's first row; pos_off: the RoPE position of row s is pos0 + pos_off + s, its slot pos0 + s (dyn: both from *dyn)
hipError_t launch_rope_table(void* tab, int S, int half, const float* inv_freq_dev, int64_t pos0, hipStream_t st, const StepState* dyn = nullptr);   // float2 [S][half], bf16-rounded; pos0 = the RoPE position of row 0 (dyn: n_ctx + pos_off of *dyn)
struct ConstraintRow;
hipError_t launch_advance_state(StepState* st_dev, const int64_t* tok_dev, int64_t* prev_dev, int prev_cap, int64_t eos, int use_penalty, hipStream_t st,
                                const ConstraintRow* cons_dev = nullptr);          // cons_dev: EOS is membership of its set (read on the device), `eos` is ignored
hipError_t launch_add_rows(int dtype, void* x, const void* add, int M, int H, int period, hipStream_t st);   // x[m,:] += add[m % period,:]
hipError_t launch_rope_append_chunk(const void* qkv, int S, int nh, int nkv, const void* tab, int64_t pos0, void* q_out, void* Kc, void* Vc, int64_t cap, hipStream_t st);   // bf16, d = 128, transposed V, table from launch_rope_table
hipError_t launch_rope_append(int dtype, const void* qkv, int S, int nh, int nkv, int d, const float* inv_freq_dev, int64_t pos0, void* q_out,
                              void* Kc, void* Vc, int64_t cap, int v_transposed, hipStream_t st, int64_t pos_off = 0);          // slot pos0 + s, RoPE position pos0 + pos_off + s
// mmd_kv_drop: in every one of `rows` (layer, kv head) rows of `pitch_bytes`, tokens [to, len) of K (rows of tok_bytes) and of V (transposed 64-token blocks) move down to [from, ...)
hipError_t launch_kv_drop(int dtype, void* K, void* V, int rows, int64_t pitch_bytes, int d, int64_t from, int64_t to, int64_t len, hipStream_t st);
// mmd_kv_drop_shift: the same move, the keys that arrive in [from, len - (to - from)) turned back by to - from positions (pairs (e, e + d/2), angle (float)(to - from) * inv_freq[e])
hipError_t launch_kv_drop_shift(int dtype, void* K, void* V, int rows, int64_t pitch_bytes, int d, int64_t from, int64_t to, int64_t len, const float* inv_freq_dev, hipStream_t st);
// mmd_kv_drop_spans: one owner walk over at most 64 retained segments segs[nseg][2] = (src, count) (HOST memory, passed on by value), segment i moving down to dst0 + the counts
// in front of it; inv_freq_dev non-null: the keys of segment i turned back by src_i - dst_i positions.  len_end: the stream's length behind the launch
hipError_t launch_kv_compact(int dtype, void* K, void* V, int rows, int64_t pitch_bytes, int d, const int64_t* segs, int nseg, int64_t dst0, int64_t len_end, const float* inv_freq_dev,
                             hipStream_t st);
// mmd_kv_export / mmd_kv_import: tokens [t0, t0 + n) of every one of `rows` arena rows (K rows of tokens, V in transposed 64-token blocks) <-> the canonical form
// K_canon, V_canon [rows][n][d], token-major for both.  scatter = 0: arena -> canonical; 1: canonical -> arena slots [t0, t0 + n), no other slot's bytes written.
// All four pointers 16-byte aligned, d * element size a multiple of 16 and at most 1 KiB.
hipError_t launch_kv_canon(int dtype, int scatter, void* K_arena, void* V_arena, int rows, int64_t pitch_bytes, int d, int64_t t0, int64_t n, void* K_canon, void* V_canon,
                           hipStream_t st);
hipError_t launch_transpose_v(int dtype, const void* src, void* dst, int nkv, int64_t cap, int d, hipStream_t st);
hipError_t launch_embed(int dtype, const void* table, const int64_t* ids, int k, int H, int64_t vocab, void* out, hipStream_t st);
hipError_t launch_im2col(int dtype, const void* px, int B, int img, int patch, int grid, int Kpad, void* out, hipStream_t st);
hipError_t launch_gather_rows2(const void* xa, int64_t lda, void* ya, int Wa, const void* xb, int64_t ldb, void* yb, int Wb, const int32_t* rows_host, int n, hipStream_t st);   // n <= 64; rows ride in the kernel argument
hipError_t launch_pool(int dtype, const void* x, void* y, int B, int grid, int H, int mode, int stride, hipStream_t st);
hipError_t launch_gather_pool_rows(int dtype, const void* x, void* y, int B, int grid, int C, int out, hipStream_t st, int64_t ldx = 0);            // the (2 out)^2 tokens per frame a bilinear pool reads, compacted
hipError_t launch_pool_compact_bilinear(int dtype, const void* x, void* y, int B, int grid, int H, int out, hipStream_t st);      // the pool over that compact layout
hipError_t launch_heads(int dtype, const void* hidden, int64_t ldh, const int32_t* rows_dev, int M, const void* W4, int H, float* out,
                        hipStream_t st);
hipError_t launch_argmax_penalty(const float* logits, int V, const int64_t* prev_ids_dev, int n_prev, float penalty, int64_t* out_id,
                                 hipStream_t st, const StepState* dyn, void* scratch512);
// greedy sampling / token feed of several streams at once (mmd_round_multi): per-stream pointers ride in the kernel argument
constexpr int MMD_ROUND_MAX_SAMPLERS = 32;
struct SampleBatch { const int64_t* prev[MMD_ROUND_MAX_SAMPLERS]; int64_t* tok[MMD_ROUND_MAX_SAMPLERS]; int64_t* append[MMD_ROUND_MAX_SAMPLERS]; int n_prev[MMD_ROUND_MAX_SAMPLERS]; float penalty[MMD_ROUND_MAX_SAMPLERS]; };
struct FeedBatch { const int64_t* tok[MMD_ROUND_MAX_SAMPLERS]; int32_t row[MMD_ROUND_MAX_SAMPLERS]; };
hipError_t launch_sample_batch(const float* logits /*[n, V]*/, int V, const SampleBatch& b, int n, int64_t* toks_out_dev, void* scratch, hipStream_t st);
size_t sample_batch_scratch_bytes();
// temperature / top-k / top-p sampling (sample.hip).  One SampleRow per logits row, in DEVICE memory: everything a step's kernels need to know about the row, so a captured
// decode step is replayed unchanged when the parameters change.  n_prev_ptr (the captured step: &StepState::n_prev) overrides n_prev; `advance`: the draw kernel adds 1 to offset.
struct SampleRow {
    const int64_t* prev; const int* n_prev_ptr; int64_t* tok; int64_t* append;
    unsigned long long offset;
    int n_prev, prev_cap; float penalty, temperature; int top_k; float top_p;
    uint32_t seed_lo, seed_hi, lane, advance;
};
constexpr int SMP_MAX_SLICES = 64;
// constrained decoding (DESIGN.md "Constraints"): one ConstraintRow per logits row, in DEVICE memory beside its SampleRow.  The table is (id, bias) sorted by id, ids unique,
// bias finite or -inf (= suppressed);  z_i = mask_i(pen(l_i + b_i)) / T, mask = -inf for a suppressed id and -- while fewer than min_new tokens have been returned -- for the
// EOS ids.  step = tokens returned so far in this response; step_ptr (the captured step: &StepState::step) overrides it.  A row with n = 0, n_eos = 0 is unconstrained.
struct ConstraintRow {
    const int32_t* ids; const float* bias; const int* step_ptr;
    long long eos[CONS_MAX_EOS];
    int n, n_eos, min_new, step;
};
__host__ __device__ inline bool cons_is_eos(const ConstraintRow& c, long long t) { for (int k = 0; k < c.n_eos; ++k) if (c.eos[k] == t) return true; return false; }
// log-probability records (sample.hip): one per token.  lp = log-probability under the model (raw logits), slp = under the distribution the token was taken from, then the
// top_n largest raw logits as ids (-1: the row is shorter) and their lp.  LogprobOut says where row r of a launch records: slot (dyn ? dyn->step : idx0) + r of rec[cap] (a slot
// beyond cap is not written), for the token toks[r]; rec == null: nothing is recorded.  With `rows` (mmd_round_multi: every row belongs to another sampler) row r has a
// destination of its own, in DEVICE memory: rows[r].rec[rows[r].slot] with its own top_n, nothing when rows[r].rec is null or the slot is beyond rows[r].cap; rec / cap / dyn /
// idx0 / top_n of the LogprobOut are then unused.
struct LogprobRec { float lp, slp; float top_lp[LP_MAX_TOP]; int top_id[LP_MAX_TOP]; };
struct LogprobRow { LogprobRec* rec; int slot, cap, top_n; };
struct LogprobOut { LogprobRec* rec; int cap; const StepState* dyn; int idx0; const int64_t* toks; int top_n; const LogprobRow* rows = nullptr; };
size_t sample_topkp_scratch_bytes(int V, int n, bool own_scores);          // n <= MMD_ROUND_MAX_SAMPLERS rows per launch; own_scores: the z rows live in the scratch
hipError_t launch_sample_batch_topkp(const float* logits /*[n, V]*/, int V, int n, SampleRow* rows_dev, bool any_k, bool any_p, const unsigned long long* r_words_dev /* or null: Philox */,
                                     int64_t* toks_out_dev, float* info_out_dev /* [n,4] or null */, float* scores_out_dev /* [n,V] or null */, void* scratch, hipStream_t st,
                                     const LogprobOut* lp = nullptr /* the draw records slp */, const ConstraintRow* cons_dev = nullptr /* [n] or null: no row is constrained */);
size_t logprob_scratch_bytes(int n);
// the chain's scores z = pen(l) / T with nothing filtered (rows with top_k 0, top_p 1): maxima, masses and z stay in `scratch` for launch_logprob_rows(greedy)
hipError_t launch_sample_scores_unfiltered(const float* logits, int V, int n, const SampleRow* rows_dev, float* scores_out_dev /* [n,V] or null */, void* scratch, hipStream_t st,
                                           const ConstraintRow* cons_dev = nullptr);
// the constrained arg-max: first maximal index of the z that launch_sample_scores_unfiltered left in `scratch` (-1: a NaN, or every z is -inf) -> rows[r].tok / .append, toks_out[r]
hipError_t launch_argmax_scores(int V, int n, const SampleRow* rows_dev, float* scores_out_dev, void* scratch, int64_t* toks_out_dev /* or null */, hipStream_t st);
// lp and the top_n of n <= MMD_ROUND_MAX_SAMPLERS rows; greedy: slp too, from what launch_sample_scores_unfiltered left in sample_scratch (same scores_out_dev).  The scores
// may have been launched over more rows than are recorded: over sw_rows rows (0: n), of which the launch's row 0 was row sw_row0
hipError_t launch_logprob_rows(const float* logits, int V, int n, const LogprobOut& o, bool greedy, float* scores_out_dev, void* sample_scratch, void* lp_scratch, hipStream_t st,
                               int sw_rows = 0, int sw_row0 = 0);
// streaming cross entropy over lm_head logit chunks (mmd_lm_nll; ops.hip): fold chunk `logits` [m, nc] (row stride ld, ld % 4 == 0; vocabulary columns [c0, c0 + nc)) into
// state [m, 3] = (max, sum exp, label logit) -- `first`: the state starts empty -- through the one-writer partials part [m, lm_nll_splits(m, nc), 3]; then nll / lse from the state
constexpr int LM_NLL_BLOCKS = 2048, LM_NLL_MAX_SPLITS = 256;          // blocks one chunk's reduce aims at; m * lm_nll_splits(m, nc) <= max(m, LM_NLL_BLOCKS)
int lm_nll_splits(int m, int nc);
hipError_t launch_lm_nll_chunk(const float* logits, int64_t ld, int m, int nc, int64_t c0, const int64_t* labels, int first, float* state, float* part, hipStream_t st);
hipError_t launch_lm_nll_finalize(const float* state, const int64_t* labels, int64_t ignore_index, int m, float* nll, float* lse /* or null */, hipStream_t st);
hipError_t launch_embed_feed(int dtype, const void* table, const FeedBatch& f, int n, int H, int64_t vocab, void* out, hipStream_t st);
hipError_t launch_convert(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, hipStream_t st);
hipError_t launch_copy_rows(int dtype, const void* src, int64_t lds_, void* dst, int64_t ldd, int rows, int cols, hipStream_t st);
hipError_t launch_interleave16(int dtype, const void* a, const void* b, void* out, int rows, int cols, hipStream_t st);
hipError_t launch_pad_cols(int dtype, const void* src, int rows, int cols, void* dst, int cols_pad, hipStream_t st);
hipError_t launch_lora_merge(int dtype, void* W, const float* A, const float* B, int out_f, int in_f, int r, float scale, hipStream_t st);
hipError_t launch_preprocess_im2col(int dtype, const uint8_t* frames, int T, int R, int size, const int32_t* coef, const int32_t* bounds, int ksize,
                                    uint8_t* tmp, int patch, int grid, int Kpad, void* out, hipStream_t st);
hipError_t launch_normalize_frames(int dtype, const void* in, int in_kind /*0 uint8, 1 fp32*/, int B, int R, float rescale, const float* mean, const float* sd, void* out, hipStream_t st);
hipError_t launch_assemble_cls(int dtype, const void* patch, const void* cls, const void* pos, int B, int Tk, int C, void* out, hipStream_t st);
hipError_t launch_quick_gelu(int dtype, void* x, int64_t n, hipStream_t st);
hipError_t launch_letterbox(const uint8_t* src, int T, int H, int W, int new_w, int new_h, int R, int top, int left, const int32_t* xtab,
                            const int32_t* ytab, int area2x, int flip, uint32_t pad, uint8_t* dst, hipStream_t st);
hipError_t launch_preprocess(int dtype, const uint8_t* frames, int T, int R, int size, const int32_t* coef, const int32_t* bounds, int ksize,
                             uint8_t* tmp, void* out, hipStream_t st);

hipError_t launch_attention(int dtype, const AttnArgs& a, hipStream_t st);
hipError_t launch_attention_decode_multi(const AttnArgs& a, hipStream_t st);     // decode rows of a.nseg streams in one launch (attn.hip)
