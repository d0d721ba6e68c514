/*
 * mmduet.h -- C ABI of libmmduet_hip.so: the MI355X-native (gfx950) streaming video-text-duet forward path.
 *
 * The reference (yellow-binary-tree/MMDuet) has no native/FFI interface of its own: its drop-in boundary is the
 * Python duck-type the stream driver uses.  This header is the native layer underneath that
 * Python surface; every entry point names the reference interface it stands in for (paths relative to the reference
 * repository root).  The Python shim that binds it with ctypes is mmduet_amd/_lib.py.
 *
 * Conventions
 *   - all functions return 0 on success or a negative MMD_E* code; mmd_last_error() gives the message.
 *     No C++ exception crosses the ABI.
 *   - pointers are DEVICE pointers unless the parameter is documented as host.
 *   - one hipStream_t per context (mmd_set_stream); calls on one context are not thread-safe -- the Python layer
 *     holds a per-model mutex (the reference's Gradio demo calls the model from two threads, demo/app.py:84-85).
 *   - activation / weight element type is chosen per context (mmd_config.dtype): MMD_BF16 (production) or MMD_F32
 *     (bit-for-bit-class parity runs against the fp32 oracle).  Logit outputs are always fp32, like the reference's
 *     `.float()` (models/live_llava/video_head_live_llava_qwen.py:155,160-161).
 */
#ifndef MMDUET_H
#define MMDUET_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MMD_OK 0
#define MMD_EINVAL (-22)
#define MMD_ENOMEM (-12)
#define MMD_ENOENT (-2)
#define MMD_ERANGE (-34)
#define MMD_EHIP (-5)
#define MMD_EDOM (-33)         /* a NaN among the logits a token was to be taken from -- on EVERY route: plain arg-max, constrained arg-max, draw --, or, under
                                  constraints, no score above -inf.  No token is returned for that step and none is fed back. */

typedef enum { MMD_F32 = 0, MMD_BF16 = 1 } mmd_dtype;
/* storage of the decoder's linear-layer weights (q/k/v/o/gate/up/down): MMD_W_FP8_E4M3 = OCP e4m3fn with one fp32 scale per output
 * channel (BASELINE configs[4], scripts/inference/youcook2.sh:12-14 workload), activations and accumulation unchanged (bf16 / fp32) */
typedef enum { MMD_W_DTYPE = 0, MMD_W_FP8_E4M3 = 1 } mmd_weight_dtype;
/* ADAPTIVE_AVG = adaptive_avg_pool2d to pool_stride x pool_stride tokens (the secondary encoder path, models/vision_live.py:17-24) */
typedef enum { MMD_POOL_BILINEAR = 0, MMD_POOL_AVERAGE = 1, MMD_POOL_MAX = 2, MMD_POOL_ADAPTIVE_AVG = 3 } mmd_pool_mode;

/* Shape of the model.  Mirrors the fields of VideoHeadLiveLlavaQwenConfig (models/live_llava/video_head_live_llava_qwen.py:41-45,
 * models/configuration_live.py:22-36) plus the SigLIP tower shape LLaVA-NeXT hard-codes. */
typedef struct mmd_config {
    int32_t struct_size;          /* = sizeof(mmd_config), ABI guard */
    int32_t dtype;                /* mmd_dtype of weights and activations */
    /* Qwen2 decoder */
    int32_t vocab_size, hidden_size, intermediate_size, num_layers, num_heads, num_kv_heads, head_dim;
    float rope_theta, rms_norm_eps;
    /* SigLIP tower (vit_layers = layers that RUN) */
    int32_t vit_hidden, vit_intermediate, vit_layers, vit_heads, vit_image, vit_patch;
    float vit_ln_eps;
    int32_t vit_post_layernorm;
    /* connector / pooling (models/live_llava/video_head_live_llava_qwen.py:100-119) */
    int32_t pool_mode, pool_stride, frame_num_tokens;
    /* workspace sizing */
    int32_t max_vit_batch;        /* frames per mmd_vit_encode call (reference: 32, test/inference.py:208) */
    int32_t max_step_tokens;      /* max rows of one mmd_llm_step call */
    int32_t weight_dtype;         /* mmd_weight_dtype (bf16 contexts only) */
    /* secondary frame encoders (models/vision_live.py:11-64): a context may carry ONLY a tower -- HF SigLIP-L/16-384 or CLIP-L/14-336 */
    int32_t vision_only;          /* 1: no decoder / projector; the mmd_vision_* entry points below are the product */
    int32_t vit_class_token;      /* CLIP: class embedding prepended (tokens = grid^2 + 1) */
    int32_t vit_pre_layernorm;    /* CLIP: pre_layrnorm after the embeddings */
    int32_t vit_act;              /* 0 gelu_pytorch_tanh (SigLIP), 1 quick_gelu (CLIP) */
    int32_t vit_pool_head;        /* SigLIP: SiglipMultiheadAttentionPoolingHead present (pooler_output, used when frame_token_cls) */
    int32_t tower_f16;            /* 1: the LLaVA SigLIP tower as under torch.cuda.amp.autocast() (models/modeling_live.py:28): fp16 linears / attention matmuls
                                     with fp32 accumulate, LayerNorm / softmax in fp32, and the hidden state between them in FP32 (`fp32 + fp16` promotes), bf16
                                     features to the projector.  2: the same with the residual stream rounded to fp16 after every sublayer (the round-3 form,
                                     ~2 % faster tower).  bf16 contexts only; 0 = tower in the context dtype */
} mmd_config;

typedef struct mmd_ctx mmd_ctx;
typedef struct mmd_stream mmd_stream;

/* ---- context ------------------------------------------------------------------------------------------------ */
/* replaces model construction in build_live (models/modeling_live.py:80-129) */
int mmd_create(const mmd_config* cfg, int device, mmd_ctx** out);
void mmd_destroy(mmd_ctx* ctx);
const char* mmd_last_error(const mmd_ctx* ctx);          /* ctx may be NULL: error of the last failed mmd_create */
int mmd_set_stream(mmd_ctx* ctx, void* hip_stream);      /* hipStream_t used verbatim: NULL = the null stream (torch's default stream).
                                                            Until called, the context runs on a stream of its own. */
void* mmd_get_stream(mmd_ctx* ctx);
int mmd_synchronize(mmd_ctx* ctx);

/* ---- weights -------------------------------------------------------------------------------------------------- */
/* replaces from_pretrained weight materialisation (models/modeling_live.py:96-99).  `name` is the checkpoint name
 * (e.g. "model.layers.3.self_attn.q_proj.weight"); data is row-major in `src_dtype`; on_device != 0 if `data` is a
 * device pointer.  Tensors are converted to the context dtype.  LoRA deltas (models/modeling_live.py:123, peft
 * y = Wx + (alpha/r) B(Ax)) are merged with mmd_merge_lora before mmd_finalize_weights. */
int mmd_load_tensor(mmd_ctx* ctx, const char* name, const void* data, int src_dtype, const int64_t* shape, int rank,
                    int on_device);
int mmd_merge_lora(mmd_ctx* ctx, const char* weight_name, const float* A_host, const float* B_host, int r, float scale);
/* RoPE inverse frequencies theta^(-2i/d), i < head_dim/2 (host fp32).  Optional: the default table is computed in
 * double precision; the Python shim passes the table torch computes with the reference's own expression
 * (transformers qwen2/modeling_qwen2.py:84-85) so that fp32 parity at large positions does not hinge on pow() ulps. */
int mmd_set_rope_inv_freq(mmd_ctx* ctx, const float* inv_freq_host, int n);
int mmd_finalize_weights(mmd_ctx* ctx);                  /* builds fused layouts; fails listing the first missing tensor */
int64_t mmd_weight_bytes(const mmd_ctx* ctx);

/* ---- vision side ---------------------------------------------------------------------------------------------- */
/* Scheduling knob, no effect on results: cap the persistent grid of the tower's / projector's ring GEMMs at `max_blocks` workgroups (0 = one per CU).
 * The driver (mmduet_amd/inference.py) halves the tower's share while a response is being decoded on the other HIP stream: the weight-streaming
 * decode kernels then find free CUs and tower batches hide under the decode burst instead of queueing in front of it. */
int mmd_set_tower_share(mmd_ctx* ctx, int max_blocks);
/* replaces LiveMixin.visual_embed (models/modeling_live.py:26-33): tower -> connector -> pooling.
 * pixel_values [B,3,img,img] in ctx dtype; out [B*frame_num_tokens, hidden] in ctx dtype. */
int mmd_vit_encode(mmd_ctx* ctx, const void* pixel_values, int B, void* out);
/* preprocess + visual_embed in one call: uint8 frames [B,3,R,R] (device) -> out [B*frame_num_tokens, hidden].  The last
 * resampler pass writes the normalised pixels straight into the im2col matrix of the patch-embed GEMM; results are bit-identical to
 * mmd_preprocess_frames followed by mmd_vit_encode. */
int mmd_vit_encode_frames(mmd_ctx* ctx, const uint8_t* frames, int B, int R, void* out);
/* second half of visual_embed for pre-extracted tower features (the reference's offline feature files, data/utils.py:99-117: per-video
 * [T, tokens, C] written from `vision_encode`; visual_embed without a tower starts at the connector, models/modeling_live.py:26-33):
 * tower_features [B, tokens, vit_hidden] (ctx dtype) -> mm_projector -> post_projector_pooling -> out [B*frame_num_tokens, hidden] */
int mmd_connector_pool(mmd_ctx* ctx, const void* tower_features, int B, void* out);
/* ---- secondary encoder path (models/vision_live.py:11-54 `_siglip_vision_encode` / `_clip_vision_encode`) -------------------------------
 * mmd_normalize_frames: torchvision normalize(frames * rescale, mean, std) (:13,:36); frames uint8 (src_kind 0) or fp32 (1) [B,3,R,R] -> ctx dtype.
 * mmd_vision_tower: `vision_model(frames).last_hidden_state` -> out [B, tokens, vit_hidden] (SigLIP: after post_layernorm; CLIP: class token first,
 *   pre_layrnorm, quick_gelu, NO post_layernorm on the sequence).
 * mmd_vision_pool_tokens: adaptive_avg_pool2d of the s x s spatial tokens (class token skipped) to out_h x out_w (:17-24,:40-47) -> [B, out_h*out_w, C].
 * mmd_vision_pool_head: SigLIP pooler_output (probe attention + LayerNorm + MLP, siglip/modeling_siglip.py [3P]) -> [B, C] (:28). */
int mmd_normalize_frames(mmd_ctx* ctx, const void* frames, int src_kind, int B, int R, const float* mean3_host, const float* std3_host, float rescale, void* out);
int mmd_vision_tower(mmd_ctx* ctx, const void* pixel_values, int B, void* out);
int mmd_vision_pool_tokens(mmd_ctx* ctx, const void* feats, int B, int out_h, int out_w, void* out);
int mmd_vision_pool_head(mmd_ctx* ctx, const void* feats, int B, void* out);
/* intermediate taps for parity tests: stage 0 = tower output [B*tokens, vit_hidden], 1 = connector output
 * [B*tokens, hidden]; valid until the next mmd_vit_encode. */
/* The default encode path runs the LAST tower layer and the projector on the tokens the bilinear post_projector_pooling reads ((2 out)^2 of vit_tokens per frame:
 * models/live_llava/video_head_live_llava_qwen.py:100-119 interpolates without antialiasing) -- same values, same arithmetic, rows nobody reads are not computed.  Callers
 * that want vision_encode's full [B, tokens, C] (offline feature extraction, data/utils.py:99-117) or the debug taps switch that off first. */
int mmd_vit_set_full_tower(mmd_ctx* ctx, int on);
int mmd_vit_get_full_tower(const mmd_ctx* ctx);            /* current setting (1 / 0): callers that flip it temporarily restore what they found */
int mmd_vit_debug_tap(mmd_ctx* ctx, int stage, void* out, int64_t out_elems);
/* replaces image_processor.preprocess (test/inference.py:203; LLaVA SigLipImageProcessor): uint8 [T,3,R,R] ->
 * PIL-bicubic resize to img x img (bit-exact with Pillow's 8-bit resampler), x/255, (x-.5)/.5 -> ctx dtype. */
int mmd_preprocess_frames(mmd_ctx* ctx, const uint8_t* frames, int T, int R, void* pixel_values);
/* replaces the per-frame resize + pad + colour flip of load_video (test/datasets.py:52-71, demo/liveinfer.py:32-51):
 * decoded frames uint8 [T,H,W,3] (device) -> cv2.resize(INTER_LINEAR, 8-bit fixed point) to the letterbox size ->
 * cv2.copyMakeBorder(BORDER_CONSTANT, pad_color[3], in SOURCE channel order) -> cv2.cvtColor(BGR2RGB) when flip_channels
 * -> CHW, out uint8 [T,3,R,R].  Geometry (target size and the four pad widths) as the reference computes it. */
int mmd_letterbox_geometry(int W, int H, int R, int* new_w, int* new_h, int* top, int* bottom, int* left, int* right);
int mmd_letterbox_frames(mmd_ctx* ctx, const uint8_t* frames, int T, int H, int W, int R, const uint8_t* pad_color,
                         int flip_channels, uint8_t* out);

/* ---- language side -------------------------------------------------------------------------------------------- */
/* replaces model.get_input_embeddings()(ids) (test/inference.py:236,251,259; models/modeling_live.py:76). ids: device int64 */
int mmd_embed_tokens(mmd_ctx* ctx, const int64_t* ids, int k, void* out);

/* KV arena of one video stream; replaces the DynamicCache / legacy tuple cache handed around as `past_key_values`
 * (test/inference.py:183,239-240; the reference regrows it by torch.cat every step).  O(1) append and O(1) truncate.  The arena is a
 * VIRTUAL address range sized for MMDUET_KV_VIRTUAL_TOKENS (default 4 Mi tokens ~ the 288 GB limit of the 7B model) whose first
 * mmd_kv_capacity tokens are backed by physical pages; growth maps more pages (hipMemCreate / hipMemMap) behind the same addresses --
 * nothing is copied and no second arena ever exists.  (MMDUET_KV_NO_VMM=1: plain allocation, growth by reallocation + copy.) */
int mmd_stream_create(mmd_ctx* ctx, int64_t initial_tokens, mmd_stream** out);
void mmd_stream_destroy(mmd_stream* s);
int64_t mmd_kv_len(const mmd_stream* s);
int64_t mmd_kv_capacity(const mmd_stream* s);             /* tokens backed by memory */
int64_t mmd_kv_stride(const mmd_stream* s);               /* tokens per (layer, kv head) row of the address range */
int mmd_kv_truncate(mmd_stream* s, int64_t new_len);      /* rollback: remove_assistant_turns (test/inference.py:265-269), speculative chunks */
/* set the KV of tokens [from, to) aside / bring it back (length becomes `to`): with remove_assistant_turns (test/inference.py:265-269) a response fired in
 * the middle of a multi-frame chunk overwrites the slots behind it and is then dropped -- the frames already encoded behind it are restored, not recomputed */
int mmd_kv_stash(mmd_stream* s, int64_t from, int64_t to);
int mmd_kv_unstash(mmd_stream* s);
/* Sliding context window: slots [from, to) leave every layer's arena and the tokens behind them move down to [from, len - (to - from)), bit for bit (keys keep
 * the rotation they were written with; nothing is re-rotated).  The length shrinks by to - from, mmd_kv_position stays: tokens written afterwards take slot
 * mmd_kv_len and RoPE position mmd_kv_position = length + everything dropped so far.  One launch on the context's stream, no host synchronisation; pages stay
 * mapped; slots at or above the new length are unspecified.  from == to enqueues nothing, to == length is a truncate that keeps the position.
 * MMD_ERANGE unless 0 <= from <= to <= length, MMD_EINVAL while a stash is held.  mmd_kv_truncate leaves the position offset alone, mmd_stream_reset zeroes it. */
int mmd_kv_drop(mmd_stream* s, int64_t from, int64_t to);
/* The same with SHIFTED positions (DESIGN.md section 5 "Shifted positions"): positions are counted inside the arena.  V and the bookkeeping of the length are those of
 * mmd_kv_drop; the keys of tokens [to, len) arrive in [from, len - (to - from)) turned back by to - from positions -- dims (e, e + head_dim/2) by the angle
 * (float)(to - from) * inv_freq[e], cos / sin in fp32 and not rounded to the context dtype, fp32 products and sums, one rounding to the context dtype -- so that slot t holds
 * the key of position t + offset again: mmd_kv_len and mmd_kv_position BOTH shrink by to - from, the offset earlier plain drops left stays.  Keys in [0, from) are not
 * written.  One launch, no host synchronisation.  Refusals as mmd_kv_drop, and MMD_EINVAL (with a message) unless the context is bf16 or fp32 with an even head_dim whose
 * half is a multiple of 16 bytes.  A refused call changes nothing. */
int mmd_kv_drop_shift(mmd_stream* s, int64_t from, int64_t to);
/* Many spans in one pass (DESIGN.md section 5 "Eviction"): the n spans spans_host[i] = (from_i, to_i), ascending and disjoint, leave every layer's arena; what stays moves
 * down ONCE, bit for bit (shift == 0: the bookkeeping of mmd_kv_drop, the position stays) or with every retained key turned back ONCE by the tokens dropped in front of it
 * (shift != 0: the arithmetic and the bookkeeping of mmd_kv_drop_shift, length and position shrink by the total).  Empty spans are ignored, touching spans are merged; up
 * to 64 spans are one launch, more are one launch per 64.  The list is host memory and is read before the call returns; no host synchronisation.  MMD_ERANGE if a span
 * is outside [0, length] or has to < from; MMD_EINVAL if the spans do not ascend or overlap, while a stash is held, for a null stream, n < 0 or a null list with n > 0, and
 * (shift) for what mmd_kv_drop_shift refuses.  A refused call changes nothing. */
int mmd_kv_drop_spans(mmd_stream* s, const int64_t* spans_host /* [n][2] */, int n, int shift);
int64_t mmd_kv_position(const mmd_stream* s);             /* RoPE position of the next token written: mmd_kv_len + tokens dropped (-1: null stream) */
int mmd_stream_reset(mmd_stream* s);                      /* LiveInferForBenchmark.reset (test/inference.py:169-183: past_key_values = None): length 0, position 0, arena kept */
/* Snapshots: take a stream's context out of its arena, put one in, hold one twice (no reference counterpart: the reference's DynamicCache is a list of torch tensors that
 * callers clone or torch.save themselves).  The CANONICAL FORM is K, V [num_layers][num_kv_heads][n][head_dim] in the context's dtype, token-major for BOTH (keys rotated as
 * they were written; V un-transposed out of the arena's 64-token blocks): it does not depend on the arena's capacity, row pitch or blocking.  The canonical buffers are device
 * pointers, 16-byte aligned.  All four calls are enqueued on the context's stream without synchronising it (growing an arena maps pages on the host, as a step does).
 * mmd_kv_export: tokens [from, to) of every (layer, kv head) row -> K_out / V_out [layers, nkv, to - from, d].  MMD_ERANGE unless 0 <= from <= to <= mmd_kv_len; from == to
 *   enqueues nothing.  Allowed while a stash is held (it only reads).
 * mmd_kv_import: n canonical tokens are appended at slots [len, len + n) and the length grows by n; the arena is grown first, as by a step.  Only those slots are written: in a
 *   V block shared with older tokens the older tokens' bytes are untouched, and slots at or above the new length keep the finite values they had.  MMD_EINVAL while a stash is
 *   held, MMD_ERANGE for n < 0.  The position offset is left alone: the appended tokens keep the rotation they carry, mmd_kv_set_position says where the next one goes.
 * mmd_kv_set_position: the RoPE position of the next token written becomes `position` (mmd_kv_position returns it; the offset is position - len).  MMD_ERANGE if position < len.
 *   Nothing else is checked: the call is accepted while a stash is held, and a position below that of tokens already written (they keep their rotation) is the caller's to avoid.
 * mmd_kv_fork: dst becomes tokens [0, n) of src, with src's position offset: a device-to-device copy in arena form between the two arenas, which may differ in capacity and row
 *   pitch; dst is grown first.  V travels in whole 64-token blocks, so slots >= n of dst hold unspecified finite values.  src is not changed in any byte.  MMD_ERANGE unless
 *   0 <= n <= mmd_kv_len(src); MMD_EINVAL when dst == src, when the streams belong to different contexts, or while dst holds a stash. */
int mmd_kv_export(mmd_stream* s, int64_t from, int64_t to, void* K_out, void* V_out);
int mmd_kv_import(mmd_stream* s, const void* K_in, const void* V_in, int64_t n);
int mmd_kv_set_position(mmd_stream* s, int64_t position);
int mmd_kv_fork(mmd_stream* dst, const mmd_stream* src, int64_t n);
int mmd_kv_debug_set_len(mmd_stream* s, int64_t n);       /* measurement aid: mark n slots live without computing them */

/* replaces VideoHeadLiveLlavaQwenForCausalLM.forward body (models/live_llava/video_head_live_llava_qwen.py:141) ==
 * Qwen2Model.forward for batch 1: embeds [S, hidden] are appended at positions kv_len..kv_len+S-1; hidden_out
 * [S, hidden] receives the post-final-RMSNorm hidden state (may be NULL). */
int mmd_llm_step(mmd_ctx* ctx, mmd_stream* s, const void* embeds, int S, void* hidden_out);
/* informative_head / relevance_head (models/live_llava/video_head_live_llava_qwen.py:160-161): hidden rows [M, hidden] ->
 * out [M,4] fp32 = (informative[0], informative[1], relevance[0], relevance[1]). */
int mmd_video_heads(mmd_ctx* ctx, const void* hidden, int M, float* out);
/* lm_head (models/live_llava/video_head_live_llava_qwen.py:155): hidden rows [M, hidden] -> logits [M, vocab] fp32 */
int mmd_lm_head(mmd_ctx* ctx, const void* hidden, int M, float* logits);
/* teacher-forced scoring, the lm_loss terms of models/live_llava/video_head_live_llava_qwen.py:155,164-170 before their mean:
 * per-row negative log-likelihood of labels under lm_head(hidden) without materialising [M,V] logits:
 * hidden [M,hidden] (device, ctx dtype), labels [M] int64 (device); nll_out [M] fp32 (device, 0 where label == ignore_index),
 * lse_out [M] fp32 or NULL.  chunk_cols: vocabulary columns per pass, 0 = auto.  Enqueued on the context's stream, no synchronisation.
 * A label that is neither ignore_index nor in [0, vocab) gives NaN in its row (it is compared with column indices, never used as an address). */
int mmd_lm_nll(mmd_ctx* ctx, const void* hidden, int M, const int64_t* labels, int64_t ignore_index, int chunk_cols, float* nll_out, float* lse_out);
/* one fused per-frame step for the streaming loop (test/inference.py:239-244): llm_step + heads at the rows listed in
 * head_rows (host int32[n_rows], e.g. the last token of every frame in a chunk); scores_out host fp32 [n_rows,4]
 * (synchronises the stream). */
int mmd_frame_step(mmd_ctx* ctx, mmd_stream* s, const void* embeds, int S, const int32_t* head_rows_host, int n_rows,
                   float* head_logits_host);

/* Multi-stream forms (no reference counterpart: the reference runs one video per process, batch 1; SURVEY.md section 7 names
 * "batch several independent streams per GPU" as the way out of the weight-streaming regime).  Segment j = seg_rows[j]
 * consecutive rows of `embeds`, extending streams[j] (each stream at most once): the GEMMs run ONCE over all rows -- a stream
 * that is generating rides with its single row on the other streams' frame chunks -- RoPE/KV append/attention run per
 * segment on its own arena.  Per-row results equal the single-stream calls up to GEMM accumulation order.
 * mmd_frame_step_multi adds, after the step: the 4 video-head logits at head_rows -> heads_out_host [n,4] (host, ONE
 * sync when n_head_rows > 0), the final hidden state at hidden_rows -> hidden_rows_out [n,hidden] (device, ctx dtype) and,
 * when logits_out != NULL, lm_head over those rows in one pass -> logits_out [n,vocab] fp32 (device). */
int mmd_llm_step_multi(mmd_ctx* ctx, mmd_stream* const* streams, const int32_t* seg_rows, int n_segs, const void* embeds, void* hidden_out);
int mmd_frame_step_multi(mmd_ctx* ctx, mmd_stream* const* streams, const int32_t* seg_rows, int n_segs, const void* embeds,
                         const int32_t* head_rows, int n_head_rows, float* heads_out_host,
                         const int32_t* hidden_rows, int n_hidden_rows, void* hidden_rows_out, float* logits_out);

/* Scheduler rounds with the greedy sampling on the device (the multi-stream form of fast_greedy_generate, models/modeling_live.py:51-77; the offline drivers
 * test/inference.py:257-274 call it once per response).  With several streams per GPU the token loops of all talking streams advance together, one token per round,
 * inside the forward that also carries the watching streams' frame chunks; per round the host sees the head logits and ONE token id per talking stream -- no logits
 * tensor, no host arg-max, no embedding call.
 * mmd_sampler = greedy sampling state of one stream on the device: the token drawn last and the repetition-penalty list that persists across the turns of a video
 * (models/modeling_live.py:60-66).  mmd_sampler_begin starts a response: eos id, penalty (<= 0: none), the ids generated so far in this video (host), the most tokens
 * this response may add.  The sampler then grows the list itself: a drawn token joins it unless it is EOS (EOS is returned but neither fed back nor penalised).
 * mmd_round_multi = mmd_frame_step_multi with, per segment j, its input rows seg_embeds[j] [seg_rows[j], hidden] (device, ctx dtype) and flags:
 *   MMD_SEG_FEED    the segment is ONE row, the embedding of the token samplers[j] drew in an earlier round (gathered on the device; seg_embeds[j] is ignored);
 *   MMD_SEG_SAMPLE  after the step: lm_head over the segment's last row, repetition penalty over samplers[j]'s list, arg-max (first maximal index) -> tokens_out_host[j]
 *                   and samplers[j]'s token slot.
 * tokens_out_host [n_segs] receives -1 for the other segments; heads as in mmd_frame_step_multi.  ONE stream synchronisation per round (none when nothing is read).
 * At most 32 feed and 32 sampling segments per round.
 * A NaN among the logits of a sampling segment's row fails the round with MMD_EDOM, whichever way the segment's sampler takes its token (plain arg-max included: the
 * kernel answers -1 for such a row, never the arg-max of the rest).  The step itself has run: the streams are extended, tokens_out_host holds -1 for that segment, its sampler
 * has not advanced.  A following round without that sampler runs as usual. */
typedef struct mmd_sampler mmd_sampler;
#define MMD_SEG_FEED 1
#define MMD_SEG_SAMPLE 2
int mmd_sampler_create(mmd_ctx* ctx, mmd_sampler** out);
void mmd_sampler_destroy(mmd_sampler* sp);                /* before mmd_destroy of its context */
int mmd_sampler_begin(mmd_sampler* sp, int64_t eos_id, float rep_penalty, const int64_t* prev_ids_host, int n_prev, int max_new);
int mmd_sampler_prev_len(const mmd_sampler* sp);          /* entries of the penalty list that count */
/* Sampling instead of arg-max for this sampler (DESIGN.md "Sampling": scores pen(l) / T, top-k and top-p as thresholds that keep whole tie classes, an index-order inverse
 * CDF over fixed-point masses, the random word from Philox4x32-10 keyed by `seed` at counter (offset, lane)).  temperature <= 0 switches back to arg-max; top_k 0 (or >= vocab)
 * and top_p 1 are off.  Called after mmd_sampler_begin or at any response boundary; the offset -- tokens drawn since the seed was set -- restarts at 0 only when the seed changes.
 * The lane is the sampler's id within its context (mmd_sampler_lane), so a stream's tokens do not depend on which other streams share a round.  In mmd_round_multi the sampling
 * segments of such samplers go through the sampling chain, the others keep the arg-max; a round may mix both.  A NaN among a row's logits fails the round with MMD_EDOM. */
int mmd_sampler_set_sampling(mmd_sampler* sp, float temperature, int top_k, float top_p, uint64_t seed);
int mmd_sampler_lane(const mmd_sampler* sp);
int64_t mmd_sampler_offset(const mmd_sampler* sp);        /* tokens drawn since the seed was set */
int mmd_round_multi(mmd_ctx* ctx, mmd_stream* const* streams, const int32_t* seg_rows, int n_segs, const void* const* seg_embeds, mmd_sampler* const* samplers,
                    const int32_t* seg_flags, const int32_t* head_rows, int n_head_rows, float* heads_out_host, int64_t* tokens_out_host);

/* replaces fast_greedy_generate (models/modeling_live.py:51-77): feeds prompt_embeds [S,hidden], then up to max_new
 * greedy steps.  prev_ids_host / n_prev: the repetition-penalty list persisted across turns (grown in place, capacity
 * prev_cap); rep_penalty <= 0 disables the penalty (and the list is not updated, like the reference).  EOS is written
 * to out_ids but neither fed back nor added to the list.  out_ids_host int64[max_new]; n_out = tokens written.
 * The arg-max is the first maximal index of pen(l) over the fp32 logits l (-inf everywhere: index 0; +inf: the first +inf).  MMD_EDOM: a NaN among the logits of a step --
 * wherever it sits, on the penalty list or not; n_out tokens were returned before, the step's token is neither returned nor fed back, and the stream keeps the rows it was
 * extended by, exactly as mmd_sample_generate leaves it. */
int mmd_greedy_generate(mmd_ctx* ctx, mmd_stream* s, const void* prompt_embeds, int S, int64_t eos_id, float rep_penalty,
                        int64_t* prev_ids_host, int* n_prev, int prev_cap, int64_t* out_ids_host, int max_new, int* n_out);

/* mmd_greedy_generate's loop with the sampling chain in the arg-max's place (what HF `generate(do_sample=True)` does for the reference class,
 * models/live_llava/video_head_live_llava_qwen.py:207-242): one loop and one decode step serve both; each draw keeps its own captured step.  Draw i uses Philox offset *offset_inout + i and the lane set by
 * mmd_set_sample_lane (default 0); *offset_inout advances by the tokens drawn.  max_new == 0 enqueues nothing.  MMD_EDOM: a NaN among the logits (n_out tokens were drawn before). */
int mmd_sample_generate(mmd_ctx* ctx, mmd_stream* s, const void* prompt_embeds, int S, int64_t eos_id, float rep_penalty, int64_t* prev_ids_host, int* n_prev, int prev_cap,
                        float temperature, int top_k, float top_p, uint64_t seed, uint64_t* offset_inout, int64_t* out_ids_host, int max_new, int* n_out);
int mmd_set_sample_lane(mmd_ctx* ctx, int lane);

/* Log-probabilities of the tokens the two generate calls above return (what HF exposes as output_scores + compute_transition_scores; no reference counterpart: the
 * reference's loops keep the ids only).  For every returned token t (EOS included), with l the fp32 lm_head logits of its step:
 *   logprob          = l[t] - logsumexp(l): the model's log-probability, -nll of mmd_lm_nll for label t;
 *   sampling_logprob = z[t] - logsumexp over the kept set of z: under the distribution t was taken from (z = pen(l) / T and the kept set {z >= tau} of DESIGN.md "Sampling";
 *                      after an arg-max T = 1 and everything is kept, i.e. log_softmax(pen(l))[t]);
 *   top_n alternatives = the top_n largest raw logits by (value descending, index ascending), as ids and logprobs; id -1 and -inf where the vocabulary is shorter.
 * The maximum is subtracted and mass is summed as in the sampling chain (trunc(exp(x - max) 2^40) in 64-bit integers, one writer per partial): a token's numbers do not depend
 * on the grid.  A row with a NaN gives NaN (mmd_sample_generate still fails with MMD_EDOM).
 * mmd_set_generate_logprobs: top_n = -1 off (the default: the generate calls enqueue what they enqueue without this feature), 0..8 on with that many alternatives; holds for the
 * following generate calls of the context; anything else is MMD_ERANGE.  The captured decode step is keyed by the setting too.  The records stay on the device until
 * mmd_generate_logprobs_read copies those of the most recent generate call (ONE copy, then a stream synchronisation): logprob_host / sampling_logprob_host float[cap_tokens],
 * top_ids_host int64[cap_tokens, top_n], top_logprob_host float[cap_tokens, top_n] (host; each may be NULL); *n_out = that call's token count, 0 if it did not record;
 * MMD_ERANGE if cap_tokens is smaller.
 * mmd_round_multi records per sampler.  mmd_sampler_set_logprobs: -1 off (the default: a round enqueues and posts what it does without this feature), 0..8 on with that many
 * alternatives, anything else MMD_ERANGE; refused for vocabularies above 2^18 like the context-wide setting.  It is called at a response boundary -- before
 * mmd_sampler_begin, or after it and before the response's first sampled token -- and returns MMD_EINVAL once the running response has returned a token (a response is over
 * with its EOS or its max_new-th token; switching then discards its records).  The records live in a sampler-owned device array sized for the response's max_new, grown (the
 * stream drained first) at mmd_sampler_begin or here, whichever comes second.  In a round a recording sampler's row writes the record of its token into the slot of the
 * response's token count; samplers that record, with different top_n, and samplers that do not may share a round, and a row's numbers do not depend on the others.  Nothing
 * more crosses to the host per round and the round's one synchronisation stays one.  A round that fails with MMD_EDOM leaves the failing sampler's count where it was.
 * mmd_sampler_logprobs_read: the records of the response begun by the most recent mmd_sampler_begin, shapes and meaning as mmd_generate_logprobs_read (logprob and the
 * alternatives over the raw logits, sampling_logprob over z and its kept set, under constraints too); *n_out = the tokens that sampler's rounds have returned so far in the
 * response (EOS included), 0 when the sampler does not record; ONE copy, then a stream synchronisation; MMD_ERANGE if cap_tokens is smaller than *n_out. */
int mmd_set_generate_logprobs(mmd_ctx* ctx, int top_n);
int mmd_generate_logprobs_read(mmd_ctx* ctx, float* logprob_host, float* sampling_logprob_host, int64_t* top_ids_host, float* top_logprob_host, int cap_tokens, int* n_out);
int mmd_sampler_set_logprobs(mmd_sampler* sp, int top_n);
int mmd_sampler_logprobs_read(mmd_sampler* sp, float* logprob_host, float* sampling_logprob_host, int64_t* top_ids_host, float* top_logprob_host, int cap_tokens, int* n_out);

/* Constrained decoding (DESIGN.md "Constraints"; what HF generate gives the reference class through eos_token_id lists, min_new_tokens, suppress_tokens, single-token
 * bad_words_ids and sequence_bias, models/live_llava/video_head_live_llava_qwen.py:231).  For the fp32 lm_head logits l of a step the chain's score becomes
 *   z_i = mask_i(pen(l_i + b_i)) / T
 * b_i: the bias of id i in the table (0 when absent; -inf = suppressed); pen: the repetition penalty, once per id, on l_i + b_i; mask_i = -inf when i is suppressed or when i is
 * one of the EOS ids and fewer than min_new tokens have been returned so far in this response.  Everything behind z is the chain as it was (DESIGN.md "Sampling"); the arg-max
 * is the first maximal index of z at T = 1.  A token equal to ANY of the EOS ids ends the response: returned, not fed back, not appended to the penalty list.  With recording
 * on, logprob and the top_n alternatives stay over the raw logits; sampling_logprob is over z.
 * mmd_set_generate_constraints holds for the following mmd_greedy_generate / mmd_sample_generate calls (host arrays, copied before it returns): eos_ids [n_eos <= 8] -- with a
 * set given the calls' own eos_id is ignored, with none it stays the one EOS id --, min_new >= 0, the table ids [n <= 256] (unique, in [0, vocab)) with bias [n] (finite or
 * -inf).  n_eos = min_new = n = 0 is off, the default: the calls then enqueue what they enqueue without this feature.  MMD_EINVAL: a limit above is broken, a bias is NaN or
 * +inf, or the suppressed ids together with the EOS ids cover the vocabulary.  Switching on or off gives another captured decode step; new values of a set that stays on are
 * re-uploaded into the context's buffers and the captured step is replayed as it is.  Per token: a row whose every z is -inf (the raw logits may hold -inf themselves) fails the
 * call with MMD_EDOM like a NaN row, on the arg-max and on the draw route.
 * mmd_sampler_set_constraints: the same per sampler (the table lives in a sampler-owned device buffer, uploaded synchronously); a round of mmd_round_multi may mix constrained
 * and unconstrained samplers, arg-max and sampled. */
int mmd_set_generate_constraints(mmd_ctx* ctx, const int64_t* eos_ids_host, int n_eos, int min_new, const int32_t* ids_host, const float* bias_host, int n);
int mmd_sampler_set_constraints(mmd_sampler* sp, const int64_t* eos_ids_host, int n_eos, int min_new, const int32_t* ids_host, const float* bias_host, int n);

/* ---- multi-GPU: the one collective of the path ------------------------------------------------------------------ */
/* The reference shards videos over N manually launched processes (--start_idx/--end_idx, test/inference.py:337) and has no
 * collective; here one process per GPU gathers the per-frame head scores of its streams with ONE RCCL all-gather over xGMI.
 * Rank 0 draws an id (mmd_comm_unique_id, host bytes), the launcher's rendezvous store hands it to every rank, each rank calls
 * mmd_comm_create (collective).  mmd_gather_scores: local [T,2] fp32 (device; informative, relevance probability per frame)
 * -> all [world, t_max+1, 2] fp32 (device): row 0 of every rank's block = (T, 0), rows 1..T the scores, NaN beyond.  Enqueued
 * on the communicator's stream, no host synchronisation. */
#define MMD_COMM_ID_BYTES 128
typedef struct mmd_comm mmd_comm;
int mmd_comm_unique_id(uint8_t* id_out_host);
int mmd_comm_create(const uint8_t* id_host, int rank, int world, int device, void* hip_stream, mmd_comm** out);
void mmd_comm_destroy(mmd_comm* comm);
int mmd_comm_world(const mmd_comm* comm);
const char* mmd_comm_last_error(const mmd_comm* comm);    /* comm may be NULL: error of the last failed create / unique_id */
int mmd_gather_scores(mmd_comm* comm, const float* local, int T, int t_max, float* all);
int mmd_comm_probe(void);                                          /* MMD_OK if librccl can be bound (asked by every rank before the collective create) */
int mmd_comm_set_stream(mmd_comm* comm, void* hip_stream);         /* the stream the following gathers are issued on */
int mmd_gather_block(mmd_comm* comm, const float* block, int64_t n_floats, float* all);   /* raw: [n_floats] per rank -> [world, n_floats], one ncclAllGather */

/* ---- measurement ---------------------------------------------------------------------------------------------- */
/* HIP-event timing of kernel classes on the context's stream (bench.py `roofline`).  While enabled every launch of a
 * enabled class is bracketed by events; mmd_prof_read returns accumulated ms and launch counts. */
enum { MMD_K_GEMM_SKINNY = 0, MMD_K_GEMM_TILE = 1, MMD_K_ATTN_LLM = 2, MMD_K_ATTN_VIT = 3, MMD_K_NORM_ROPE = 4,
       MMD_K_OTHER = 5, MMD_K_COUNT = 6 };
int mmd_prof_enable(mmd_ctx* ctx, int class_mask);       /* bit k set = bracket launches of class MMD_K_k; 0 = off */
int mmd_prof_set_stride(mmd_ctx* ctx, int stride);       /* bracket only every stride-th launch of an enabled class (sampling) */
int mmd_prof_read(mmd_ctx* ctx, double* ms_out /*[MMD_K_COUNT]*/, int64_t* launches_out /*[MMD_K_COUNT]*/,
                  double* bytes_out /*[MMD_K_COUNT] algorithmic bytes*/, double* flops_out /*[MMD_K_COUNT]*/);
int mmd_prof_reset(mmd_ctx* ctx);

/* ---- raw operator entry points (parity tests call the kernels through these) ------------------------------------ */
/* Y[M,N] = epilogue(X[M,K] . W[N,K]^T + bias).  epi: 0 none, 1 gelu(tanh), 2 gelu(erf), 3 add residual R[M,N],
 * 4 SwiGLU (W rows interleaved gate/up in blocks of 16 -> Y[M,N/2]).  out_f32 != 0 writes fp32. variant: 0 auto,
 * 1 generic tile, 2 skinny/split-K, 3 large tile, 4 DMA 128-row tile, 5 skinny slabs, 6 256x256 ring, 8 streaming kernel (32 < M <= 256; SwiGLU only in this form). */
int mmd_op_gemm(mmd_ctx* ctx, const void* X, const void* W, const void* bias, const void* R, void* Y, int M, int N, int K,
                int epi, int out_f32, int variant);
/* raw form for parity tests: the same path over an explicit W [V,K] (device, ctx dtype, row-major) and X [M,K] */
int mmd_op_lm_nll(mmd_ctx* ctx, const void* X, const void* W, int M, int V, int K, const int64_t* labels, int64_t ignore_index, int chunk_cols,
                  float* nll_out, float* lse_out);
/* what the dispatcher chose for the most recent GEMM of this context: out4 = {kernel (0 tile64, 1 tile128, 2 skinny, 3 gemv16, 4 big64,
 * 5 big128, 6 ring256), output tiles, K splits, blocks launched} */
int mmd_op_gemm_last_plan(mmd_ctx* ctx, int* out4);
/* a producer GEMM and its ONLY consumer: T = epi1(X[M,K1] . W1[N1,K1]^T + b1), Y[M,N2] = T . W2[N2,T]^T (+ R).  piece_major != 0 lets the intermediate live in the ring
 * kernel's piece-major activation layout when both GEMMs take that kernel (what the tower's fc1 -> fc2 and a chunk's gate_up -> down do inside the model); *used_pm_out says
 * whether it did.  Same bits either way. */
int mmd_op_gemm_pair(mmd_ctx* ctx, const void* X, const void* W1, const void* b1, int epi1, const void* W2, const void* R, void* Y, int M, int N1, int K1, int N2,
                     int piece_major, int* used_pm_out);
/* the weight-streaming GEMMs in slab mode (what the fused LLM schedule launches for M <= 256): `*splits_out` fp32 partial slabs [splits][M][N] of X . W^T in slabs_out
 * (device, room for max_splits slabs); variant 2 = the dispatcher's choice by M (gemv16 / skinny / stream), 8 = gemm_stream_kernel */
int mmd_op_gemm_slabs(mmd_ctx* ctx, const void* X, const void* W, int M, int N, int K, int variant, float* slabs_out, int max_splits, int* splits_out);
/* fp8 weight path, raw form: mmd_op_quantize_fp8 replaces W [N,K] (bf16, row-major, device) by bf16(q), q = rne_e4m3(W / scale[n]),
 * scale[n] = amax_n / 448, and writes the fp8 bytes q8 [N,K] and scale [N] (fp32).  mmd_op_gemm_w8 = mmd_op_gemm on such a matrix:
 * Y = epilogue((X . q^T) * scale + bias); M <= 64 streams the fp8 copy, larger M the bf16(q) copy (bit-identical values). */
int mmd_op_quantize_fp8(mmd_ctx* ctx, void* W, int N, int K, uint8_t* q8_out, float* scale_out);
int mmd_op_gemm_w8(mmd_ctx* ctx, const void* X, const void* Wq, const uint8_t* q8, const float* scale, const void* bias, const void* R, void* Y,
                   int M, int N, int K, int epi, int out_f32, int variant);
/* micro-benchmark of one GEMM shape (HIP events on the context's stream); avg ms per call incl. any split-K reduce.  X [M,K] / W [N,K]
 * (device, ctx dtype) supply the operand VALUES (random data: operand bits set the chip's clock); NULL = a constant fill */
int mmd_op_gemm_bench(mmd_ctx* ctx, int M, int N, int K, int epi, int variant, int iters, float* avg_ms_out, const void* X, const void* W);
/* the sampling chain on n <= 4096 rows of fp32 logits [n, V] (V <= 2^18), one set of parameters, row i on lane i; prev_ids_dev [n_prev] int64 is the penalty list of every row
 * (rep_penalty <= 0: none).  r_host: NULL = Philox words from (seed, offset, lane), else uint64[n] explicit random words (host).  tokens_out int64[n] (-1: the row holds a NaN),
 * info_out float[n,4] = (tau, kept count, kept mass / total mass, NaN flag), scores_out [n,V] or NULL = the scores z = pen(l) / T.  Synchronises the stream. */
int mmd_op_sample(mmd_ctx* ctx, const float* logits, int n, int V, const int64_t* prev_ids_dev, int n_prev, float rep_penalty, float temperature, int top_k, float top_p,
                  uint64_t seed, uint64_t offset, const uint64_t* r_host, int64_t* tokens_out, float* info_out, float* scores_out);
/* mmd_op_sample with the rows' log-probability records.  greedy != 0: the arg-max with penalty (first maximal index) stands in the draw's place -- temperature, top_k, top_p and
 * the random words are ignored, the scores are pen(l), info_out is not written and may be NULL.  Outputs on the HOST: lp_out_host float[n, 2] = (logprob, sampling_logprob),
 * top_ids_out_host int64[n, top_n], top_lp_out_host float[n, top_n] (0 <= top_n <= 8, else MMD_ERANGE).  Synchronises the stream.  A row with a NaN: token -1 (greedy
 * too) and NaN records; the call still answers MMD_OK. */
int mmd_op_sample_logprobs(mmd_ctx* ctx, const float* logits, int n, int V, const int64_t* prev_ids_dev, int n_prev, float rep_penalty, float temperature, int top_k, float top_p,
                           uint64_t seed, uint64_t offset, const uint64_t* r_host, int greedy, int top_n, int64_t* tokens_out, float* info_out, float* scores_out,
                           float* lp_out_host, int64_t* top_ids_out_host, float* top_lp_out_host);
/* mmd_op_sample_logprobs with one constraint set per row (the limits of mmd_set_generate_constraints, checked per row): row i's table is entries [tab_off_host[i],
 * tab_off_host[i + 1]) of tab_ids_host / tab_bias_host, its EOS ids eos_host[i * 8 ..] (n_eos_host[i] of them), min_new_host[i], and step_host[i] = tokens returned so far.
 * greedy != 0: the constrained arg-max.  lp_out_host may be NULL (nothing recorded, top_n ignored).  MMD_EDOM when a row has a NaN or nothing above -inf (its token is -1). */
int mmd_op_sample_constrained(mmd_ctx* ctx, const float* logits, int n, int V, const int64_t* prev_ids_dev, int n_prev, float rep_penalty, float temperature, int top_k, float top_p,
                              uint64_t seed, uint64_t offset, const uint64_t* r_host, int greedy, int top_n,
                              const int32_t* tab_off_host, const int32_t* tab_ids_host, const float* tab_bias_host, const int64_t* eos_host, const int32_t* n_eos_host,
                              const int32_t* min_new_host, const int32_t* step_host,
                              int64_t* tokens_out, float* info_out, float* scores_out, float* lp_out_host, int64_t* top_ids_out_host, float* top_lp_out_host);
int mmd_op_rmsnorm(mmd_ctx* ctx, const void* x, const void* w, void* y, int M, int H, float eps);
int mmd_op_layernorm(mmd_ctx* ctx, const void* x, const void* w, const void* b, void* y, int M, int H, float eps);
/* the autocast tower's residual step (models/modeling_live.py:28: `hidden (fp32) + sublayer_out (fp16)` promotes, LayerNorm returns fp32, the next linear casts to
 * fp16): h32[M,H] = (pos16 ? float(pos16[m % period]) : h32) + float(y16); out16 = fp16(LayerNorm(h32) * w16 + b16) when w16 is given; outbf = bf16(h32) when outbf
 * is given (h32 itself is not rewritten then).  All 16-bit operands are IEEE half except outbf.  H % 8 == 0, H <= 2048. */
int mmd_op_resid32_layernorm(mmd_ctx* ctx, const void* y16, float* h32, const void* pos16, int period, const void* w16, const void* b16, void* out16, void* outbf,
                             int M, int H, float eps);
/* q [S, nh*d] (rotated in place), k/v [S, nkv*d] appended rotated/unrotated at pos0.. into Kc/Vc [nkv, cap, d] */
int mmd_op_rope_append(mmd_ctx* ctx, void* qkv, int S, int nh, int nkv, int d, float theta, int64_t pos0, void* q_out,
                       void* Kc, void* Vc, int64_t cap);
/* the code that writes the KV arena, one `writer` at a time, on caller-owned Kc / Vc [nkv, cap, d] (parity tests of the arena's contents):
 *   0 rope_append_kernel, row-major V (mmd_op_rope_append)      1 rope_append_kernel, V in transposed 64-token blocks (fp32 contexts, tile steps under 64 rows)
 *   2 rope_append_chunk_kernel over the step's (cos, sin) table (bf16, d = 128)      3 slab_rope_append_kernel (bf16)
 *   4 the decode attention's fused q / k / v preparation (bf16, d = 128, S * nh / nkv <= 16, n_slabs <= 4): attention variant 3 over n_ctx = pos0 context tokens already in
 *     Kc / Vc, result in attn_out [S, nh*d]; q_out is not written (q never leaves the kernel).
 * src: writers 0-2 the fused qkv rows [S, (nh + 2 nkv) d] in the context dtype; writers 3 / 4 the first row of this step inside fp32 split-K slabs [n_slabs][slab_rows][(nh + 2 nkv) d]
 * with bias [(nh + 2 nkv) d] (bf16).  inv_freq_host [d / 2]: the RoPE frequencies, used as given.  Transposed V needs cap % 64 == 0.  An unsupported combination is
 * MMD_EINVAL before anything is launched.  Synchronises the stream. */
int mmd_op_kv_write(mmd_ctx* ctx, int writer, const void* src, int n_slabs, int slab_rows, const void* bias, const float* inv_freq_host, int S, int nh, int nkv, int d,
                    int64_t pos0, void* q_out, void* Kc, void* Vc, int64_t cap, void* attn_out);
/* The code that writes the residual stream h between two GEMMs of a decoder layer, and its RMSNorm image, on caller-owned device buffers (tests/test_gpu_residual_stream.py).
 * Both entries are bf16 kernels, refuse with MMD_EINVAL before anything is launched, synchronise the stream, and leave what they launched to mmd_op_gemm_last_plan.
 *
 * mmd_op_slab_resid_rmsnorm: slab_resid_rmsnorm_kernel alone.  slabs fp32 [splits][M][H] are summed in slab order (x wscale [H] fp32, if given), rounded to bf16, added to
 * resid [M,H] and rounded: h_out [M,H] (may be resid itself); xn_out [M,H] = rnd(norm_w * rnd(h_out / rms)).  last_plan: {32, instantiation 4 / 8 / 16, splits, M}.
 * Refused: a context that is not bf16, a missing operand (wscale alone may be NULL), M < 1, H > 4096, H % 4 != 0, splits outside 1 .. 16.
 *
 * mmd_op_gemv_chain: one GEMV of the decode chain, W [N,K] bf16 row-major (packed as mmd_op_gemm does; with q8 [N,K] and scale [N] of mmd_op_quantize_fp8 the fp8 copy as in
 * mmd_op_gemm_w8, W then being bf16(q)).  ssq is [rows >= M][256] fp32: per row, the sums of squares of h per 16-column tile.
 *   role 2, producer: h [M,N] <- rnd(rnd((X [M,K] . W^T) * scale) + h) in place, ssq[m][t] for t < N / 16 written.  gamma, Y NULL, epi 0.
 *   role 1, consumer: x = rnd(gamma [K] * rnd(h [M,K] * rsqrt(sum(ssq[m][0 .. 255]) / K + eps))) is built inside the kernel; X is passed on as the step passes it and never read.
 *     epi 0: Y receives fp32 slabs [splits][M][N] (room for max_splits; the planner chooses a count that fits), *splits_out the count.   epi 4: Y = SwiGLU product bf16 [M,N/2]
 *     (gate / up rows of W interleaved in blocks of 16).
 * Refused: a context that is not bf16; a role other than 1 / 2, operands that do not belong to the role (above), q8 without scale or the reverse; M outside 1 .. 16, N % 16 != 0,
 * K % 32 != 0 (fp8: K % 64), epi 4 with N % 32 != 0; and whatever the planner refuses or plans in another chain form: a consumer with M > 4 or with more than 1024 k per wave
 * (K / (4 x splits), in whole k-tiles rounded up), a producer with N > 4096. */
int mmd_op_slab_resid_rmsnorm(mmd_ctx* ctx, const float* slabs, int splits, int M, int H, const void* resid, void* h_out, const void* norm_w, float eps, void* xn_out,
                              const float* wscale);
int mmd_op_gemv_chain(mmd_ctx* ctx, int role, const void* X, const void* W, const uint8_t* q8, const float* scale, void* h, const void* gamma, float* ssq, float eps,
                      void* Y, int M, int N, int K, int epi, int max_splits, int* splits_out);
/* The kernels of the plain greedy token loop (lm_head -> penalty + arg-max -> state advance -> embedding of the winner) on caller-owned device buffers
 * (tests/test_gpu_greedy.py).  The entries refuse with MMD_EINVAL before anything is launched, synchronise the stream, and go through the launchers and the context scratch
 * that mmd_greedy_generate and mmd_round_multi use.
 *
 * mmd_op_argmax: logits [n, V] fp32; row r's penalty list is entries [prev_off_host[r], prev_off_host[r + 1]) of prev_ids_dev (int64; ids outside [0, V) match no column),
 * its penalty penalty_host[r] (<= 0: none -- no list and the factor 1, as the generate calls pass it on).  tokens_out int64[n]: the first maximal index of pen(l), -1 for a row
 * with a NaN.
 *   form 0  argmax_penalty_kernel + argmax_final_kernel row by row, the list length in the kernel argument (the eager steps of mmd_greedy_generate);
 *   form 1  the same with the length in a device StepState and 0 in the kernel argument (the captured decode step; the kernel reads the StepState only when penalty != 1);
 *   form 2  argmax_penalty_multi_kernel + argmax_final_multi_kernel over all n <= 32 rows in ONE launch (mmd_round_multi): row r's token also goes to tok_slots_out[r] (the
 *           sampler's token slot) and, when its penalty is on, to append_out[r] (the slot behind the sampler's list); a row without penalty leaves append_out[r] alone.
 *           tok_slots_out / append_out int64[n], ignored (may be NULL) for forms 0 and 1.
 * Refused: a form outside 0 .. 2, a missing operand, n outside 1 .. 4096 (form 2: 1 .. 32), V < 1, offsets that do not start at 0 or decrease, lists without ids.
 *
 * mmd_op_advance_state: ONE launch of advance_state_kernel, no constraints: `token` joins prev_dev[*n_prev] when use_penalty != 0, token != eos_id and *n_prev < prev_cap;
 * n_ctx and step grow by one either way.  prev_dev int64[>= prev_cap] (device), the three counters in and out on the host.  Refused: *n_prev outside 0 .. prev_cap.
 *
 * mmd_op_embed_feed: launch_embed_feed over the context's embedding table: out[rows_host[i], :] = embed[clamp(tok_slots_dev[i], 0, vocab - 1), :] for i < n <= 32; out
 * [out_rows, hidden] in the context dtype, rows not listed are not written.  Refused: a row index outside [0, out_rows).  (mmd_embed_tokens is embed_kernel, same clamp.) */
int mmd_op_argmax(mmd_ctx* ctx, int form, const float* logits, int n, int V, const int64_t* prev_ids_dev, const int32_t* prev_off_host, const float* penalty_host,
                  int64_t* tokens_out, int64_t* tok_slots_out, int64_t* append_out);
int mmd_op_advance_state(mmd_ctx* ctx, int64_t token, int64_t eos_id, int use_penalty, int64_t* prev_dev, int prev_cap, int* n_prev_inout_host, int64_t* n_ctx_inout_host,
                         int* step_inout_host);
int mmd_op_embed_feed(mmd_ctx* ctx, const int64_t* tok_slots_dev, const int32_t* rows_host, int n, int out_rows, void* out);
/* the first n tokens (n % 64 == 0, n <= mmd_kv_capacity) of one layer of a stream's arena AS STORED: K_out [nkv, n, d] rotated rows, V_out [nkv, n / 64, d, 64] transposed
 * 64-token blocks (token t, dim e of a head at ((t >> 6) * d + e) * 64 + (t & 63)); device buffers in the context dtype.  Synchronises the stream. */
int mmd_kv_debug_read(mmd_stream* s, int layer, int64_t n, void* K_out, void* V_out);
/* causal GQA attention with query offset: q [S, nh*d], Kc/Vc [nkv, cap, d], n_ctx = tokens before this step;
 * out [S, nh*d].  causal = 0 -> full attention over n_ctx + S keys.  variant: 0 auto, 1 simple, 2 mfma, 3 the arena kernels (attn_gqa128_kernel), 4 row-major
 * K / V (the tower's), 5 attn_gqa128_w1_kernel, 6 attn_gqa128_chunk_kernel. */
int mmd_op_attention(mmd_ctx* ctx, const void* q, const void* Kc, const void* Vc, void* out, int S, int nh, int nkv, int d,
                     int64_t n_ctx, int64_t cap, int causal, int variant);
int mmd_op_attention_bench(mmd_ctx* ctx, int S, int nh, int nkv, int d, int64_t n_ctx, int variant, int iters, float* avg_ms_out);
/* which attention form the most recent LLM (or raw-operator) attention launch of THIS context took (what mmd_op_gemm_last_plan is for the GEMMs: parity tests assert that
 * the production kernel really ran; the tower's launches and other contexts do not disturb it): 1 one wave per row, 2 16-row MFMA tiles, 3 / 4 attn_gqa128_kernel with 16- /
 * 32-row waves (decode and two-slot forms / 256-row phase-split chunks), 5 attn_gqa128_w1_kernel (per-frame steps, short chunks), 6 register-staged row-major (ViT), 7
 * attn_d72_ring_kernel (SigLIP-so400m), 8 attn_gqa128_chunk_kernel (multi-frame chunks, contiguous decomposition), 9 the decode rows of several streams in one launch
 * (mmd_round_multi); out2 = {form, key splits or the most blocks sharing a unit} */
int mmd_op_attention_last_form(mmd_ctx* ctx, int* out2);
/* what the decode steps of the most recent mmd_greedy_generate / mmd_sample_generate of this context did: 0 none or launched one by one, 1 replayed an existing captured
 * step, 2 captured the step in that call, then replayed it (tests of the replay assert that it ran) */
int mmd_op_decode_last_route(mmd_ctx* ctx);
/* the schedule the most recent LLM step of this context took (step_plan() of mmduet_amd/csrc/step_plan.h; tests assert that a step, or an A/B switch, took the schedule they
 * mean): out9 = {schedule (0 tile, 1 fused slabs, 2 decode chain), rope_fused, chunk_rope, sparse_last, run0, run_n, run_all (the batched decode attention's run of segments),
 * down_slab_norm, mlp_pm} */
int mmd_op_step_last_plan(mmd_ctx* ctx, int* out9);
/* the schedule the most recent vision-tower run of this context took (tower_plan() of mmduet_amd/csrc/tower_plan.h): out12 = {element type (0 fp32, 1 bf16, 2 IEEE half),
 * residual form (0 epilogue add, 1 fp32 stream, 2 epilogue add in half), embed form (0 add rows, 1 class token, 2 fp32 stream), sparse_last, pout, U, compact_rows,
 * proj_compact, proj_gather, mlp_pm, mlp_pm_last, final_convert}.  mmd_vit_debug_tap refuses exactly when sparse_last is set. */
int mmd_op_tower_last_plan(mmd_ctx* ctx, int* out12);
/* the plan the most recent token selection of this context was launched from (select_plan() of mmduet_amd/csrc/select_plan.h; after a generate call whose steps replayed a
 * captured step: the plan that step was captured from): out22 = {kind (0 arg-max, 1 constrained arg-max, 2 draw), single, any_k, any_p, needs_row, needs_cons, record,
 * scores_after_argmax, record_greedy, advance}, then whose selection it was -- 0 a raw operator, 1 a generate call, 2 a round -- and that caller's own plan: a generate call's
 * {can_graph, upload_state, post_row_dynamic, post_row_each_eager_step, post_cons_dynamic, post_cons_each_eager_step, host_appends_penalty, pen_key_is_value, key_sel, key_lp,
 * key_cons_gen}, a round's {n_plain, n_greedy, n_sample, any_k, any_p, any_cons_sampled} (the rest of the 11 unspecified) */
int mmd_op_select_last_plan(mmd_ctx* ctx, int* out22);
/* what the most recent round of this context recorded: out4 = {recording rows in the plain arg-max block, in the constrained arg-max block, in the sampled block, the largest
 * top_n among them (-1: no row recorded)}; {0, 0, 0, -1} before the first round (tests assert that the record path ran, or did not) */
int mmd_op_round_last_record(mmd_ctx* ctx, int* out4);
int mmd_op_pool(mmd_ctx* ctx, const void* x, void* y, int B, int grid, int H, int mode, int stride);

#ifdef __cplusplus
}
#endif
#endif
