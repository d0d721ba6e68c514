"""HIP-backed LiveLlava model with the reference's Python surface.

Mirrors (names, argument meaning, error behaviour) the pieces of the reference the stream driver touches:
  VideoHeadLiveLlavaQwenForCausalLM   models/live_llava/video_head_live_llava_qwen.py:67-242
  VideoHeadCausalLMOutputWithPast     models/live_llava/video_head_live_llava_qwen.py:48-58
  LiveMixin.visual_embed / joint_embed   models/modeling_live.py:26-48
  fast_greedy_generate                models/modeling_live.py:51-77
  build_live / build_model_and_tokenizer   models/modeling_live.py:80-129, models/__init__.py:8-13
All arithmetic runs in libmmduet_hip.so (include/mmduet.h); torch only provides device buffers and the stream.
"""
from __future__ import annotations
import ctypes as C
import threading
import weakref
from typing import Optional
import torch

from . import _lib, constraints as _constraints
from ._lib import lib, check, MmdConfig, MMD_BF16, MMD_F32, POOL_MODES
from .configuration_live import VideoHeadLiveLlavaQwenConfig
from .tokenization_live import build_live_tokenizer_and_update_config

_TORCH2MMD = {torch.float32: MMD_F32, torch.bfloat16: MMD_BF16}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


# ----------------------------------------------------------------------------------------------------------------
# KV cache handles
# ----------------------------------------------------------------------------------------------------------------
class _KVArena:
    """Owns one native KV arena (mmd_stream): contiguous per-layer K/V with O(1) append / truncate.

    Arenas are recycled through a small per-model pool: creating one is two hipMalloc + memset of ~1 GB (30 ms, 3 % of a 300-frame
    stream), reusing one is an O(1) truncate to length 0 (every slot holds finite data, which is all the masked tail of a key
    tile needs).  Only arenas up to POOL_MAX_TOKENS are kept, at most POOL_SIZE of them; `model.release_pooled_arenas()` frees them."""
    POOL_SIZE = 8
    POOL_MAX_TOKENS = 1 << 16

    def __init__(self, model, initial_tokens):
        self.model = model
        self.handles = weakref.WeakSet()
        model._bind_stream()          # a new arena's zero-fill is stream-ordered: on the caller's stream, where the steps that write the arena follow (not on the tower's side stream, if that was bound last)
        pool = model.__dict__.setdefault('_arena_pool', [])
        for i, h in enumerate(pool):
            if lib().mmd_kv_capacity(h) >= int(initial_tokens):
                pool.pop(i)
                check(lib().mmd_stream_reset(h), model._ctx, 'mmd_stream_reset')          # length 0 and position 0 (a recycled arena may have had spans dropped)
                self.h = h
                return
        h = C.c_void_p()
        check(lib().mmd_stream_create(model._ctx, int(initial_tokens), C.byref(h)), model._ctx, 'mmd_stream_create')
        self.h = h

    def length(self):
        return int(lib().mmd_kv_len(self.h))

    def truncate(self, n):
        if n < self.length():
            for hd in list(self.handles):
                if hd.length > n:
                    hd.stale = True
            check(lib().mmd_kv_truncate(self.h, int(n)), self.model._ctx, 'mmd_kv_truncate')

    def __del__(self):
        try:
            if self.h and self.model._ctx:
                pool = self.model.__dict__.get('_arena_pool')
                if pool is not None and len(pool) < self.POOL_SIZE and lib().mmd_kv_capacity(self.h) <= self.POOL_MAX_TOKENS:
                    pool.append(self.h)
                else:
                    lib().mmd_stream_destroy(self.h)
        except Exception:
            pass
        self.h = None


class KVCacheHandle:
    """`past_key_values` as callers see it: an opaque (arena, length) pair.

    Semantics the reference driver relies on:
      * falsy when empty (`if not self.past_key_values`, test/inference.py:229);
      * functional: a handle held before `fast_greedy_generate` still denotes the pre-generation context
        afterwards (remove_assistant_turns, test/inference.py:265-269).  Continuing from an older handle truncates
        the arena back to its length in O(1); handles that pointed beyond that become stale and raise if used.
    """
    __slots__ = ('arena', 'length', 'stale', '__weakref__')

    def __init__(self, arena: _KVArena, length: int):
        self.arena, self.length, self.stale = arena, int(length), False
        arena.handles.add(self)

    def __len__(self):
        return self.length

    def __bool__(self):
        return self.length > 0

    def get_seq_length(self, layer_idx=0):
        return self.length


_MMD2TORCH = {MMD_F32: torch.float32, MMD_BF16: torch.bfloat16}
_SNAPSHOT_FORMAT = 1


def snapshot_chunks(n, token_bytes, staging_bytes):
    """Token ranges [(a, b), ...] that cover [0, n) exactly once, each small enough that its K and V (`token_bytes` per token together) fit in `staging_bytes`;
    a budget below one token's bytes gives one token per chunk."""
    n, per = int(n), max(1, int(staging_bytes) // max(1, int(token_bytes)))
    return [(a, min(a + per, n)) for a in range(0, n, per)]


class KVSnapshot:
    """A stream's KV context outside any arena (DESIGN.md section 5 "Snapshots"): host tensors K, V [layers, kv_heads, n, head_dim] in the canonical, token-major form,
    the rotary position the next token gets, the dtype, and a fingerprint of the model geometry the keys were rotated for (layers, kv heads, head_dim, rope inv_freq).
    Not in it: the repetition-penalty list, sampler state and driver fields -- they remain the caller's."""
    FIELDS = ('layers', 'kv_heads', 'head_dim')

    def __init__(self, K, V, position, dtype, layers, kv_heads, head_dim, inv_freq):
        self.K, self.V, self.position, self.dtype = K, V, int(position), dtype
        self.layers, self.kv_heads, self.head_dim = int(layers), int(kv_heads), int(head_dim)
        self.inv_freq = inv_freq.detach().to('cpu', torch.float32).contiguous()
        want = (self.layers, self.kv_heads, K.shape[2] if K.ndim == 4 else -1, self.head_dim)
        for name, t in (('K', K), ('V', V)):
            if tuple(t.shape) != want or t.dtype != dtype:
                raise ValueError(f'KVSnapshot.{name}: shape {tuple(t.shape)} / {t.dtype}, expected [layers, kv_heads, n, head_dim] = {want[:2]} x n x {want[3]} in {dtype}')
        if self.position < self.length:
            raise ValueError(f'KVSnapshot.position {self.position} below its {self.length} tokens')

    @property
    def length(self):
        return int(self.K.shape[2])

    def __len__(self):
        return self.length

    def state_dict(self):
        """plain tensors and ints: torch.save / torch.load round-trip it"""
        return {'format': _SNAPSHOT_FORMAT, 'K': self.K, 'V': self.V, 'position': self.position, 'dtype': _TORCH2MMD[self.dtype], 'layers': self.layers,
                'kv_heads': self.kv_heads, 'head_dim': self.head_dim, 'inv_freq': self.inv_freq}

    @classmethod
    def from_state_dict(cls, d):
        if d.get('format') != _SNAPSHOT_FORMAT:
            raise ValueError(f"KVSnapshot: format {d.get('format')!r}, this package reads format {_SNAPSHOT_FORMAT}")
        if d['dtype'] not in _MMD2TORCH:
            raise ValueError(f"KVSnapshot: unknown dtype code {d['dtype']!r}")
        return cls(d['K'], d['V'], d['position'], _MMD2TORCH[d['dtype']], d['layers'], d['kv_heads'], d['head_dim'], d['inv_freq'])

    def save(self, path):
        torch.save(self.state_dict(), path)

    @classmethod
    def load(cls, path):
        return cls.from_state_dict(torch.load(path, map_location='cpu'))

    def check_against(self, dtype, layers, kv_heads, head_dim, inv_freq):
        """ValueError naming the first field in which this snapshot differs from a model's geometry (kv_load)"""
        if self.dtype != dtype:
            raise ValueError(f'KVSnapshot mismatch in dtype: the snapshot holds {self.dtype}, the model runs {dtype}')
        for name, mine, theirs in zip(self.FIELDS, (self.layers, self.kv_heads, self.head_dim), (layers, kv_heads, head_dim)):
            if mine != int(theirs):
                raise ValueError(f'KVSnapshot mismatch in {name}: the snapshot has {mine}, the model {int(theirs)}')
        other = inv_freq.detach().to('cpu', torch.float32)
        if other.shape != self.inv_freq.shape or not torch.equal(other.view(torch.int32), self.inv_freq.view(torch.int32)):
            raise ValueError('KVSnapshot mismatch in inv_freq: the keys were rotated with another rope table')


_U64 = (1 << 64) - 1
# generate() arguments that ask for something this package does not build: the value that means "off" is accepted, anything else raises
_GENERATE_OFF = {'num_beams': 1, 'num_beam_groups': 1, 'num_return_sequences': 1, 'min_p': None, 'typical_p': 1.0, 'penalty_alpha': None, 'epsilon_cutoff': 0.0, 'eta_cutoff': 0.0,
                 'diversity_penalty': 0.0, 'length_penalty': 1.0, 'no_repeat_ngram_size': 0, 'encoder_repetition_penalty': 1.0, 'force_words_ids': None,
                 'constraints': None, 'logits_processor': None, 'stopping_criteria': None, 'prefix_allowed_tokens_fn': None, 'min_length': 0,
                 'guidance_scale': None, 'assistant_model': None, 'streamer': None, 'output_scores': False, 'output_logits': False,
                 'output_attentions': False, 'output_hidden_states': False, 'early_stopping': False, 'renormalize_logits': False}
# the constraint arguments (DESIGN.md "Constraints"): merged by constraints.merge, applied on the device
_GENERATE_CONSTRAINTS = ('min_new_tokens', 'suppress_tokens', 'bad_words_ids', 'sequence_bias')
_GENERATE_IGNORED = ('attention_mask', 'position_ids', 'use_cache', 'return_dict', 'pad_token_id', 'bos_token_id', 'synced_gpus')


class GenerateOutput:
    """What generate(return_dict_in_generate=True) returns.  The four log-probability fields are None unless output_logprobs was asked for: logprobs and
    sampling_logprobs [1, n] fp32, top_logprobs [1, n, top_n] fp32, top_logprob_ids [1, n, top_n] int64 (n = the new tokens)."""

    def __init__(self, sequences, past_key_values, logprobs=None, sampling_logprobs=None, top_logprobs=None, top_logprob_ids=None):
        self.sequences, self.past_key_values = sequences, past_key_values
        self.logprobs, self.sampling_logprobs, self.top_logprobs, self.top_logprob_ids = logprobs, sampling_logprobs, top_logprobs, top_logprob_ids


class SamplerHandle:
    """mmd_sampler: greedy sampling state of one stream on the device (models/modeling_live.py:51-77 run by mmd_round_multi)."""

    def __init__(self, model):
        self.model = model
        h = C.c_void_p()
        with model._lock:
            model._bind_stream()          # (the sampler's slot is zeroed on the bound stream: the caller's, not the tower's side stream if that was bound last)
            check(lib().mmd_sampler_create(model._ctx, C.byref(h)), model._ctx, 'mmd_sampler_create')
        self.h = h.value

    def begin(self, eos_token_id, repetition_penalty, generated_token_ids, max_new_tokens, sampling=None, constraints=None):
        """Start of a response: the penalty list is every id generated so far in this video (it persists across turns, models/modeling_live.py:60-66).
        sampling: None = arg-max, or dict(temperature, top_k, top_p, seed) handed to mmd_sampler_set_sampling (the Philox offset restarts only when the seed changes).
        constraints: None = off, or a constraints.Constraints handed to mmd_sampler_set_constraints (with an EOS set given, eos_token_id is ignored)."""
        pen = float(repetition_penalty) if repetition_penalty is not None else 0.0
        prev = list(generated_token_ids) if (generated_token_ids is not None and pen > 0) else []
        arr = (C.c_int64 * max(1, len(prev)))(*prev)
        with self.model._lock:
            self.model._bind_stream()
            check(lib().mmd_sampler_begin(self.h, int(eos_token_id if eos_token_id is not None else -1), pen, arr, len(prev), int(max_new_tokens)), self.model._ctx, 'mmd_sampler_begin')
            cons_on = constraints is not None and constraints.on
            if cons_on or getattr(self, '_constraints_on', False):          # (a sampler that never had constraints is not touched)
                check(lib().mmd_sampler_set_constraints(self.h, *_constraints.c_arrays(constraints if cons_on else None)), self.model._ctx, 'mmd_sampler_set_constraints')
                self._constraints_on = cons_on
            if sampling is None and not getattr(self, '_sampling_on', False):
                return          # arg-max, as the sampler was created: nothing to switch
            sm = sampling or {}
            self._sampling_on = sampling is not None
            if sm.get('restart'):          # a new video on this sampler: the offset restarts although the seed stays (the native call restarts it on a seed change only)
                check(lib().mmd_sampler_set_sampling(self.h, 1.0, 0, 1.0, (int(sm.get('seed', 0)) + 1) & _U64), self.model._ctx, 'mmd_sampler_set_sampling')
            check(lib().mmd_sampler_set_sampling(self.h, float(sm.get('temperature', 1.0)) if sampling else 0.0, int(sm.get('top_k', 0) or 0), float(sm.get('top_p', 1.0)),
                                                 int(sm.get('seed', 0)) & _U64), self.model._ctx, 'mmd_sampler_set_sampling')

    def set_logprobs(self, top_n=-1):
        """mmd_sampler_set_logprobs: the sampler's rows of the following rounds record per-token log-probabilities with `top_n` (0..8) alternatives; -1 or None switches
        the recording off (the default).  At a response boundary: before `begin`, or after it and before the response's first token."""
        top_n = -1 if top_n is None else int(top_n)
        with self.model._lock:
            self.model._bind_stream()
            check(lib().mmd_sampler_set_logprobs(self.h, top_n), self.model._ctx, 'mmd_sampler_set_logprobs')
            self._logprobs_top = top_n

    def read_logprobs(self):
        """mmd_sampler_logprobs_read: the records of the response begun by the most recent `begin`, one per token the rounds have returned so far (EOS included), as the
        dict `last_generate_logprobs()` returns -- logprobs [n], sampling_logprobs [n], top_logprobs [n, top_n], top_logprob_ids [n, top_n], CPU tensors -- or None when
        the sampler does not record."""
        top = getattr(self, '_logprobs_top', -1)
        if top < 0:
            return None
        with self.model._lock:
            self.model._bind_stream()
            n = C.c_int(0)
            rc = lib().mmd_sampler_logprobs_read(self.h, None, None, None, None, 0, C.byref(n))          # the count alone: nothing is copied when there is no room
            if n.value == 0:
                check(rc, self.model._ctx, 'mmd_sampler_logprobs_read')
            k = n.value
            lp, slp = torch.empty(k, dtype=torch.float32), torch.empty(k, dtype=torch.float32)
            top_lp, top_ids = torch.empty(k, top, dtype=torch.float32), torch.empty(k, top, dtype=torch.long)
            if k:
                check(lib().mmd_sampler_logprobs_read(self.h, _ptr(lp), _ptr(slp), _ptr(top_ids), _ptr(top_lp), k, C.byref(n)), self.model._ctx, 'mmd_sampler_logprobs_read')
        return dict(logprobs=lp, sampling_logprobs=slp, top_logprobs=top_lp, top_logprob_ids=top_ids)

    @property
    def lane(self):
        """The sampler's id within its context: the Philox lane of its draws."""
        return int(lib().mmd_sampler_lane(self.h))

    @property
    def offset(self):
        """Tokens drawn since the seed was set."""
        return int(lib().mmd_sampler_offset(self.h))

    def __del__(self):
        try:
            if getattr(self, 'h', None) and getattr(self.model, '_ctx', None):
                lib().mmd_sampler_destroy(self.h)
        except Exception:
            pass
        self.h = None


class VideoHeadCausalLMOutputWithPast:
    """Output of the model call.  `.logits` (lm_head) is computed lazily and, unless
    `config.all_position_logits` is set, only for the LAST position ([1,1,V]): the streaming loop reads nothing else
    (`outputs.logits[:, -1:]`), and the reference's all-position lm_head is 53 GFLOP + 30 MB per frame of waste."""

    def __init__(self, model, hidden, cache):
        self._model, self._hidden = model, hidden          # hidden: [S, H] post-final-norm
        self.past_key_values = cache
        self.loss = 0.0
        self.lm_loss = 0.0
        self.video_loss = 0.0
        self.attentions = None
        self._logits = None
        self._heads = None

    @property
    def hidden_states(self):
        return self._hidden[None]

    @property
    def logits(self):
        if self._logits is None:
            rows = self._hidden if self._model.config.all_position_logits else self._hidden[-1:]
            self._logits = self._model.lm_head(rows)[None]
        return self._logits

    def _video_heads(self):
        if self._heads is None:
            self._heads = self._model.video_heads(self._hidden)
        return self._heads

    @property
    def informative_logits(self):
        return self._video_heads()[None, :, 0:2]

    @property
    def relevance_logits(self):
        return self._video_heads()[None, :, 2:4]


# ----------------------------------------------------------------------------------------------------------------
class _Embedding:
    """`model.get_input_embeddings()`: callable on LongTensor [..., k] (k may be 0, test/inference.py:234)."""

    def __init__(self, model):
        self._m = model

    def __call__(self, ids, out=None):
        """`out` (optional): a contiguous [k, hidden] slice of a caller's buffer to gather into (the stream driver's step buffer: no concatenation kernel)."""
        m = self._m
        ids = ids.to(device=m.device, dtype=torch.long).contiguous()
        k = ids.numel()
        if out is None:
            out = torch.empty(*ids.shape, m.config.hidden_size, dtype=m.dtype, device=m.device)
        elif out.shape != (k, m.config.hidden_size) or out.dtype != m.dtype or not out.is_contiguous():
            raise ValueError('embedding `out` must be a contiguous [k, hidden] tensor of the model dtype')
        if k:
            with m._lock:
                m._bind_stream()
                check(lib().mmd_embed_tokens(m._ctx, _ptr(ids), k, _ptr(out)), m._ctx, 'mmd_embed_tokens')
        return out


class SigLipImageProcessor:
    """`model.get_vision_tower().image_processor` (LLaVA SigLipImageProcessor, used at test/inference.py:203).
    preprocess = bicubic resize to the tower resolution (bit-exact with Pillow), 1/255, (x-.5)/.5 -- executed by the
    HIP kernel behind mmd_preprocess_frames; the result stays on the device in the model dtype, so the driver's
    `.to('cuda').to(dtype)` are no-ops."""

    def __init__(self, model):
        self._m = model
        s = model.config.vit_image_size
        self.size = (s, s)
        self.image_mean = self.image_std = (0.5, 0.5, 0.5)
        self.rescale_factor = 1 / 255

    def preprocess(self, images, return_tensors='pt'):
        m = self._m
        if isinstance(images, (list, tuple)):
            images = torch.stack([torch.as_tensor(i) for i in images])
        images = torch.as_tensor(images)
        if images.dtype != torch.uint8 or images.ndim != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3]:
            raise ValueError(f'expected uint8 frames [T,3,R,R], got {tuple(images.shape)} {images.dtype}')
        fr = images.to(m.device).contiguous()
        T, _, R, _ = fr.shape
        out = torch.empty(T, 3, self.size[0], self.size[1], dtype=m.dtype, device=m.device)
        if T:
            with m._lock:
                m._bind_stream()
                check(lib().mmd_preprocess_frames(m._ctx, _ptr(fr), T, R, _ptr(out)), m._ctx, 'mmd_preprocess_frames')
        return {'pixel_values': out}


class _VisionTower:
    def __init__(self, model):
        self.image_processor = SigLipImageProcessor(model)
        self.num_patches_per_side = model.config.vit_grid
        self.hidden_size = model.config.vit_hidden_size

    def parameters(self):
        return iter(())


class VideoHeadLiveLlavaQwenForCausalLM:
    config_class = VideoHeadLiveLlavaQwenConfig

    def __init__(self, config: VideoHeadLiveLlavaQwenConfig, torch_dtype=torch.bfloat16, device=None,
                 max_vit_batch=35, max_step_tokens=1024, kv_initial_tokens=32768):
        if torch_dtype not in _TORCH2MMD:
            raise ValueError(f'torch_dtype must be bfloat16 or float32 on this implementation, got {torch_dtype}')
        if not torch.cuda.is_available():
            raise _lib.MmduetError('no HIP device visible: this implementation runs on MI355X only (no CPU fallback)')
        L = lib()
        self.config = config
        if not hasattr(config, 'all_position_logits'):
            config.all_position_logits = False
        self.dtype = torch_dtype
        self.device = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
        self.vocab_size = config.vocab_size
        self.kv_initial_tokens = kv_initial_tokens
        self.max_vit_batch, self.max_step_tokens = max_vit_batch, max_step_tokens
        c = MmdConfig()
        c.struct_size = C.sizeof(MmdConfig)
        c.dtype = _TORCH2MMD[torch_dtype]
        c.vocab_size, c.hidden_size, c.intermediate_size = config.vocab_size, config.hidden_size, config.intermediate_size
        c.num_layers, c.num_heads, c.num_kv_heads, c.head_dim = config.num_hidden_layers, config.num_attention_heads, config.num_key_value_heads, config.head_dim
        c.rope_theta, c.rms_norm_eps = float(config.rope_theta), float(config.rms_norm_eps)
        c.vit_hidden, c.vit_intermediate, c.vit_layers, c.vit_heads = config.vit_hidden_size, config.vit_intermediate_size, config.vit_layers_run, config.vit_num_attention_heads
        c.vit_image, c.vit_patch, c.vit_ln_eps = config.vit_image_size, config.vit_patch_size, float(config.vit_layer_norm_eps)
        c.vit_post_layernorm = int(bool(config.vit_post_layernorm))
        if config.mm_spatial_pool_mode not in POOL_MODES:
            raise ValueError(f'Unexpected mm_spatial_pool_mode: {config.mm_spatial_pool_mode}')
        c.pool_mode, c.pool_stride = POOL_MODES[config.mm_spatial_pool_mode], config.video_pooling_stride
        g = config.vit_grid
        if config.mm_spatial_pool_mode == 'adaptive_avg':       # secondary path (models/vision_live.py): pool to frame_token_pooled[0] per side
            out_side = config.video_pooling_stride
        else:
            out_side = -(-g // config.video_pooling_stride) if config.mm_spatial_pool_mode == 'bilinear' else g // config.video_pooling_stride
        self.tokens_per_frame = out_side * out_side
        c.frame_num_tokens = self.tokens_per_frame
        c.max_vit_batch, c.max_step_tokens = max_vit_batch, max_step_tokens
        wd = getattr(config, 'weight_dtype', None)
        if wd not in (None, 'bf16', 'model', 'fp8', 'fp8_e4m3'):
            raise ValueError(f'unknown weight_dtype {wd!r} (None | "fp8_e4m3")')
        c.weight_dtype = 1 if wd in ('fp8', 'fp8_e4m3') else 0
        # The reference runs the tower under torch.cuda.amp.autocast() (models/modeling_live.py:28): IEEE-half matmuls, fp32 LayerNorm / softmax, whatever the model
        # dtype.  tower_dtype: None / 'auto' = do the same wherever the half forms of the kernels exist for the tower's shape (bf16 model, the LLaVA SigLIP form,
        # hidden % 64 == 0, head_dim % 8 == 0, >= 65 tokens per frame -- every real tower; measured free: 340 frames/s either way), else the model dtype;
        # 'fp16' = require it; 'bf16' / 'model' = tower in the model dtype (the round-2 behaviour).
        # 'fp16' keeps the hidden state between the fp16 matmuls in fp32, as autocast's type promotion does; 'fp16_resid16' rounds it to fp16 after every sublayer
        # (the round-3 form, a little faster, 0.022 instead of 0.020 rms from the fp32 tower at true width).
        td = getattr(config, 'tower_dtype', None)
        if td not in (None, 'auto', 'model', 'bf16', 'fp16', 'float16', 'fp16_resid16'):
            raise ValueError(f'unknown tower_dtype {td!r} (None | "auto" | "fp16" | "fp16_resid16" | "bf16")')
        half_ok = (torch_dtype == torch.bfloat16 and config.vit_hidden_size % 64 == 0 and (config.vit_hidden_size // config.vit_num_attention_heads) % 8 == 0 and
                   config.vit_grid ** 2 >= 65)
        if td in ('fp16', 'float16', 'fp16_resid16') and not half_ok:
            raise ValueError('tower_dtype=fp16 needs torch_dtype=bfloat16 and a tower with hidden % 64 == 0, head_dim % 8 == 0 and at least 65 tokens per frame')
        resid32_ok = not getattr(config, 'vit_post_layernorm', False) and config.vit_hidden_size <= 2048
        if td in ('fp16', 'float16') and not resid32_ok:
            raise ValueError('tower_dtype=fp16 (fp32 residual stream) needs a tower without post_layernorm and hidden <= 2048; use fp16_resid16')
        c.tower_f16 = 2 if (td == 'fp16_resid16' or (td in (None, 'auto') and half_ok and not resid32_ok)) else 1 if (td in ('fp16', 'float16') or (td in (None, 'auto') and half_ok)) else 0
        self.tower_dtype = {0: 'bf16' if torch_dtype == torch.bfloat16 else 'fp32', 1: 'fp16', 2: 'fp16_resid16'}[c.tower_f16]
        if c.weight_dtype and torch_dtype != torch.bfloat16:
            raise ValueError('weight_dtype=fp8_e4m3 needs torch_dtype=bfloat16 (fp8 weights x bf16 activations, fp32 accumulate)')
        self._cfg_struct = c
        self._ctx = None
        h = C.c_void_p()
        check(L.mmd_create(C.byref(c), self.device.index or 0, C.byref(h)), None, 'mmd_create')
        self._ctx = h
        self._lock = threading.RLock()      # the Gradio demo calls the model from two threads (demo/app.py:84-85)
        self._logprobs_top, self._last_logprobs = -1, None          # set_generate_logprobs / last_generate_logprobs
        self._constraints = None          # set_generate_constraints
        self._embed = _Embedding(self)
        self._tower = _VisionTower(self)
        self._finalized = False
        self._loaded_shapes = {}          # name -> shape of what load_tensor handed over (merge_lora checks an adapter against it)
        self.lm_loss_weight = self.video_loss_weight = 1
        # RoPE table with the reference's own expression (transformers qwen2/modeling_qwen2.py:84-85)
        d = config.head_dim
        inv = (1.0 / (float(config.rope_theta) ** (torch.arange(0, d, 2, dtype=torch.float) / d))).contiguous()
        check(L.mmd_set_rope_inv_freq(self._ctx, C.c_void_p(inv.data_ptr()), d // 2), self._ctx, 'mmd_set_rope_inv_freq')
        self._rope_inv_freq = inv          # part of a KVSnapshot's fingerprint: stored keys carry this rotation

    # ---- lifecycle ----------------------------------------------------------------------------------------------
    def release_pooled_arenas(self):
        """Free the KV arenas kept for reuse (see _KVArena)."""
        pool = self.__dict__.get('_arena_pool') or []
        while pool:
            lib().mmd_stream_destroy(pool.pop())

    def __del__(self):
        try:
            if self._ctx:
                self.release_pooled_arenas()
                lib().mmd_destroy(self._ctx)
        except Exception:
            pass
        self._ctx = None

    def _bind_stream(self):
        lib().mmd_set_stream(self._ctx, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    def set_tower_share(self, max_blocks: int):
        """Scheduling knob (results unchanged): cap the tower's ring-GEMM grids at `max_blocks` workgroups, 0 = all CUs (mmd_set_tower_share)."""
        with self._lock:
            check(lib().mmd_set_tower_share(self._ctx, int(max_blocks)), self._ctx, 'mmd_set_tower_share')

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    def to(self, *a, **k):
        return self

    def parameters(self):
        return iter(())

    # ---- weights ------------------------------------------------------------------------------------------------
    def load_tensor(self, name: str, t: torch.Tensor):
        if t.dtype not in _TORCH2MMD:
            t = t.float()
        t = t.contiguous()
        shape = (C.c_int64 * t.ndim)(*t.shape)
        on_dev = 1 if t.is_cuda else 0
        with self._lock:
            self._bind_stream()
            check(lib().mmd_load_tensor(self._ctx, name.encode(), _ptr(t), _TORCH2MMD[t.dtype], shape, t.ndim, on_dev), self._ctx, f'load {name}')
            if on_dev:
                torch.cuda.current_stream(self.device).synchronize()
            self._loaded_shapes[name] = tuple(t.shape)

    def merge_lora(self, weight_name: str, A: torch.Tensor, B: torch.Tensor, scale: float):
        """W += scale * B @ A on a loaded matrix.  The ABI carries r alone (the library copies r*in and out*r floats from the host pointers), so the pair is checked
        here against the shape the tensor was loaded with, or the one the configuration gives it."""
        from .weights import check_lora_shapes, expected_tensors
        check_lora_shapes(weight_name, A, B, self._loaded_shapes.get(weight_name) or expected_tensors(self.config).get(weight_name))
        A = A.float().cpu().contiguous(); B = B.float().cpu().contiguous()
        with self._lock:
            self._bind_stream()
            check(lib().mmd_merge_lora(self._ctx, weight_name.encode(), _ptr(A), _ptr(B), A.shape[0], float(scale)), self._ctx, f'lora {weight_name}')

    def load_state_dict(self, named_tensors, strict=True):
        for name, t in (named_tensors.items() if hasattr(named_tensors, 'items') else named_tensors):
            self.load_tensor(name, t)
        self.finalize()
        return self

    def finalize(self):
        with self._lock:
            self._bind_stream()
            check(lib().mmd_finalize_weights(self._ctx), self._ctx, 'mmd_finalize_weights')
        self._finalized = True

    def weight_bytes(self):
        return int(lib().mmd_weight_bytes(self._ctx))

    # ---- reference surface ------------------------------------------------------------------------------------------
    def get_model(self):
        return self

    def get_vision_tower(self):
        return self._tower

    def get_input_embeddings(self):
        return self._embed

    def set_vision_inside(self):
        """models/modeling_live.py:14-20: the tower is always inside this model."""
        return None

    def visual_embed(self, frames: torch.Tensor, out: torch.Tensor = None):
        """models/modeling_live.py:26-33 -> [B*frame_num_tokens, hidden] in the model dtype (written into `out` when given)."""
        frames = frames.to(device=self.device, dtype=self.dtype).contiguous()
        B = frames.shape[0]
        if out is None:
            out = torch.empty(B * self.tokens_per_frame, self.config.hidden_size, dtype=self.dtype, device=self.device)
        elif out.shape != (B * self.tokens_per_frame, self.config.hidden_size) or out.dtype != self.dtype or not out.is_contiguous():
            raise ValueError('visual_embed: `out` must be a contiguous [B*frame_num_tokens, hidden] tensor of the model dtype')
        with self._lock:
            self._bind_stream()
            for b0 in range(0, B, self.max_vit_batch):
                b1 = min(B, b0 + self.max_vit_batch)
                check(lib().mmd_vit_encode(self._ctx, _ptr(frames[b0:b1]), b1 - b0, _ptr(out[b0 * self.tokens_per_frame:])), self._ctx, 'mmd_vit_encode')
        return out

    def visual_embed_frames(self, frames_u8: torch.Tensor, out: torch.Tensor = None):
        """image_processor.preprocess + visual_embed (test/inference.py:203,211) in one native pass per tower batch: uint8 [B,3,R,R] -> [B*frame_num_tokens, hidden].
        The resampled, normalised pixels are written straight into the patch-embed GEMM's operand (no pixel_values tensor); bit-identical to the two-call form."""
        fr = torch.as_tensor(frames_u8)
        if fr.dtype != torch.uint8 or fr.ndim != 4 or fr.shape[1] != 3 or fr.shape[2] != fr.shape[3]:
            raise ValueError(f'expected uint8 frames [T,3,R,R], got {tuple(fr.shape)} {fr.dtype}')
        fr = fr.to(self.device).contiguous()
        B, R = fr.shape[0], fr.shape[2]
        if out is None:
            out = torch.empty(B * self.tokens_per_frame, self.config.hidden_size, dtype=self.dtype, device=self.device)
        with self._lock:
            self._bind_stream()
            for b0 in range(0, B, self.max_vit_batch):
                b1 = min(B, b0 + self.max_vit_batch)
                check(lib().mmd_vit_encode_frames(self._ctx, _ptr(fr[b0:b1]), b1 - b0, R, _ptr(out[b0 * self.tokens_per_frame:])), self._ctx, 'mmd_vit_encode_frames')
        return out

    def connector_pool(self, tower_features: torch.Tensor, out: torch.Tensor = None):
        """visual_embed for pre-extracted tower features [B, vit_tokens, vit_hidden] (models/modeling_live.py:26-33 without `vision_encode`):
        mm_projector -> post_projector_pooling -> [B*frame_num_tokens, hidden]."""
        f = tower_features.to(device=self.device, dtype=self.dtype).contiguous()
        if f.ndim != 3 or f.shape[1] != self.config.vit_grid ** 2 or f.shape[2] != self.config.vit_hidden_size:
            raise ValueError(f'expected tower features [B, {self.config.vit_grid ** 2}, {self.config.vit_hidden_size}], got {tuple(f.shape)}')
        B = f.shape[0]
        if out is None:
            out = torch.empty(B * self.tokens_per_frame, self.config.hidden_size, dtype=self.dtype, device=self.device)
        with self._lock:
            self._bind_stream()
            for b0 in range(0, B, self.max_vit_batch):
                b1 = min(B, b0 + self.max_vit_batch)
                check(lib().mmd_connector_pool(self._ctx, _ptr(f[b0:b1]), b1 - b0, _ptr(out[b0 * self.tokens_per_frame:])), self._ctx, 'mmd_connector_pool')
        return out

    def tower_features(self, frames: torch.Tensor):
        """What the reference's `vision_encode(vision_encoder, frames)` returns for the LLaVA tower (models/live_llava/video_head_live_llava_qwen.py:96-98):
        [B, vit_tokens, vit_hidden] -- the tensor its offline feature extraction stores (data/utils.py:114)."""
        frames = frames.to(device=self.device, dtype=self.dtype).contiguous()
        B, T, C = frames.shape[0], self.config.vit_grid ** 2, self.config.vit_hidden_size
        out = torch.empty(B, T, C, dtype=self.dtype, device=self.device)
        scratch = torch.empty(min(B, self.max_vit_batch) * self.tokens_per_frame, self.config.hidden_size, dtype=self.dtype, device=self.device)
        with self._lock:
            self._bind_stream()
            was = int(lib().mmd_vit_get_full_tower(self._ctx))          # a caller's own set_full_tower(True) survives this call
            check(lib().mmd_vit_set_full_tower(self._ctx, 1), self._ctx, 'mmd_vit_set_full_tower')          # vision_encode's output is the tower over ALL tokens
            try:
                for b0 in range(0, B, self.max_vit_batch):
                    b1 = min(B, b0 + self.max_vit_batch)
                    check(lib().mmd_vit_encode(self._ctx, _ptr(frames[b0:b1]), b1 - b0, _ptr(scratch)), self._ctx, 'mmd_vit_encode')
                    check(lib().mmd_vit_debug_tap(self._ctx, 0, _ptr(out[b0:b1]), (b1 - b0) * T * C), self._ctx, 'mmd_vit_debug_tap')
            finally:
                check(lib().mmd_vit_set_full_tower(self._ctx, 1 if was > 0 else 0), self._ctx, 'mmd_vit_set_full_tower')
        return out

    def set_full_tower(self, on: bool):
        """Debug / feature extraction: have the tower compute its last layer (and the projector) for every token instead of the (2 out)^2 the bilinear pool reads;
        `vit_debug_tap` needs it switched on BEFORE the visual_embed call it inspects."""
        with self._lock:
            check(lib().mmd_vit_set_full_tower(self._ctx, 1 if on else 0), self._ctx, 'mmd_vit_set_full_tower')

    def vit_debug_tap(self, stage: int, B: int):
        n = B * self.config.vit_grid ** 2
        width = self.config.vit_hidden_size if stage == 0 else self.config.hidden_size
        out = torch.empty(n, width, dtype=self.dtype, device=self.device)
        with self._lock:
            self._bind_stream()
            check(lib().mmd_vit_debug_tap(self._ctx, stage, _ptr(out), out.numel()), self._ctx, 'mmd_vit_debug_tap')
        return out

    def joint_embed(self, input_ids: torch.Tensor = None, frames: torch.Tensor = None):
        """models/modeling_live.py:35-48."""
        if frames is None:
            return self._embed(input_ids)
        if input_ids is None:
            return self.visual_embed(frames)
        input_ids = input_ids.to(self.device)
        e = self._embed(input_ids.clamp(max=self.vocab_size - 1))
        mask = input_ids == self.config.v_placeholder_id
        if mask.any():
            e[mask] = self.visual_embed(frames).to(e.dtype)
        return e

    # ---- cache plumbing ---------------------------------------------------------------------------------------------
    def _resolve_cache(self, past_key_values):
        if past_key_values is None or (isinstance(past_key_values, KVCacheHandle) and past_key_values.arena is None):
            return _KVArena(self, self.kv_initial_tokens), 0
        if not isinstance(past_key_values, KVCacheHandle) or past_key_values.arena.model is not self:
            raise TypeError('past_key_values must be a KVCacheHandle produced by this model (or None)')
        if past_key_values.stale:
            raise RuntimeError('stale KV handle: the context it denoted was overwritten by a later forward from an older handle')
        arena = past_key_values.arena
        arena.truncate(past_key_values.length)
        return arena, past_key_values.length

    def cache_prefix(self, handle: KVCacheHandle, length: int):
        """Handle denoting the first `length` tokens of `handle`'s context (speculative multi-frame chunks)."""
        if length > handle.length:
            raise ValueError('prefix longer than the context')
        return KVCacheHandle(handle.arena, length)

    def kv_stash(self, handle: KVCacheHandle, start: int):
        """Set the KV of tokens [start, len(handle)) aside (device copy, stream-ordered); `kv_unstash` brings them back after something else used those slots."""
        if handle.stale:
            raise RuntimeError('stale KV handle')
        with self._lock:
            self._bind_stream()
            check(lib().mmd_kv_stash(handle.arena.h, int(start), int(handle.length)), self._ctx, 'mmd_kv_stash')
        return (handle.arena, int(start), int(handle.length))

    def kv_unstash(self, stash):
        """-> a handle denoting the context as it was when `kv_stash` was called (everything below `start` must be unchanged since)."""
        arena, start, end = stash
        with self._lock:
            arena.truncate(min(arena.length(), start))
            self._bind_stream()
            check(lib().mmd_kv_unstash(arena.h), self._ctx, 'mmd_kv_unstash')
        return KVCacheHandle(arena, end)

    def kv_drop(self, handle: KVCacheHandle, start: int, end: int, shift: bool = False):
        """Sliding context window: tokens [start, end) leave `handle`'s context; the tokens behind them move down (device move, stream-ordered) and keep the
        rotary positions they were written with, and whatever is appended next goes on counting from `kv_position`.  With `shift` (mmd_kv_drop_shift) the keys
        behind the span are turned back by end - start positions instead, so positions are counted inside the arena and `kv_position` shrinks with the length.
        -> the handle of the shortened context; every other handle that reached beyond `start` is stale."""
        if handle.stale:
            raise RuntimeError('stale KV handle')
        start, end = int(start), int(end)
        if not 0 <= start <= end <= handle.length:
            raise ValueError(f'kv_drop [{start}, {end}) outside the context ({handle.length} tokens)')
        arena = handle.arena
        if arena is None or start == end:
            return handle
        with self._lock:
            arena.truncate(handle.length)
            self._bind_stream()
            if shift:
                check(lib().mmd_kv_drop_shift(arena.h, start, end), self._ctx, 'mmd_kv_drop_shift')
            else:
                check(lib().mmd_kv_drop(arena.h, start, end), self._ctx, 'mmd_kv_drop')
            for hd in list(arena.handles):
                if hd.length > start:
                    hd.stale = True
        return KVCacheHandle(arena, handle.length - (end - start))

    def kv_drop_many(self, handle: KVCacheHandle, spans, shift: bool = False):
        """`kv_drop` for many spans at once (mmd_kv_drop_spans): `spans` is any iterable of (start, end), ascending and disjoint; what stays moves down once, and with
        `shift` every retained key is turned back once, by the tokens dropped in front of it.  `kv_position` behaves as for `kv_drop`.
        -> the handle of the shortened context; every other handle that reached beyond the first span is stale."""
        if handle.stale:
            raise RuntimeError('stale KV handle')
        spans = [(int(a), int(b)) for a, b in spans]
        for a, b in spans:
            if not 0 <= a <= b <= handle.length:
                raise ValueError(f'kv_drop_many [{a}, {b}) outside the context ({handle.length} tokens)')
        arena = handle.arena
        if arena is None or not spans:
            return handle
        flat = (C.c_int64 * (2 * len(spans)))(*[x for sp in spans for x in sp])
        with self._lock:
            arena.truncate(handle.length)
            self._bind_stream()
            check(lib().mmd_kv_drop_spans(arena.h, C.cast(flat, C.c_void_p), len(spans), 1 if shift else 0), self._ctx, 'mmd_kv_drop_spans')
            total = sum(b - a for a, b in spans)
            if total == 0:
                return handle
            first = min(a for a, b in spans if b > a)
            for hd in list(arena.handles):
                if hd.length > first:
                    hd.stale = True
        return KVCacheHandle(arena, handle.length - total)

    def kv_position(self, handle: KVCacheHandle):
        """The rotary position the next token appended to `handle` gets: its length plus everything `kv_drop` took out of its arena without `shift`."""
        if handle is None or handle.arena is None:
            return 0
        with self._lock:
            h = handle.arena.h
            return handle.length + int(lib().mmd_kv_position(h)) - int(lib().mmd_kv_len(h))

    # ---- snapshots (DESIGN.md section 5 "Snapshots") ----------------------------------------------------------------------
    def _kv_geometry(self):
        c = self.config
        return c.num_hidden_layers, c.num_key_value_heads, c.head_dim

    def _kv_source(self, cache, what):
        """-> (arena or None, length) of the context `cache` denotes; a stale or foreign handle raises"""
        if cache is None or (isinstance(cache, KVCacheHandle) and cache.arena is None):
            return None, 0
        if not isinstance(cache, KVCacheHandle) or cache.arena.model is not self:
            raise TypeError(f'{what}: the cache must be a KVCacheHandle produced by this model (or None)')
        if cache.stale:
            raise RuntimeError('stale KV handle')
        return cache.arena, cache.length

    def _snapshot_arena(self, n):
        """The arena kv_load / kv_fork write into (the lock is held).  The stream is bound BEFORE the arena is made: a newly created arena queues the zero-fill of its
        pages on the context's stream, and the copy that follows must be behind it on the same stream."""
        self._bind_stream()
        return _KVArena(self, max(n, self.kv_initial_tokens))

    def kv_save(self, cache: KVCacheHandle, pin: bool = True, staging_bytes: int = 256 << 20) -> KVSnapshot:
        """The whole context `cache` denotes, [0, len(cache)), as a KVSnapshot in host memory (pinned when `pin`).  The arena is exported in chunks of tokens whose
        device staging buffers stay within `staging_bytes`; the arena and every handle of it stay as they are."""
        arena, n = self._kv_source(cache, 'kv_save')
        layers, nkv, d = self._kv_geometry()
        K = torch.empty(layers, nkv, n, d, dtype=self.dtype, pin_memory=bool(pin) and n > 0)
        V = torch.empty_like(K, pin_memory=bool(pin) and n > 0)
        position = 0
        if arena is not None:
            token_bytes = 2 * layers * nkv * d * K.element_size()
            chunks = snapshot_chunks(n, token_bytes, staging_bytes)
            with self._lock:
                position = n + int(lib().mmd_kv_position(arena.h)) - int(lib().mmd_kv_len(arena.h))
                if n:
                    self._bind_stream()
                    m = max(b - a for a, b in chunks)
                    sk = torch.empty(layers * nkv * m * d, dtype=self.dtype, device=self.device)
                    sv = torch.empty_like(sk)
                    for a, b in chunks:
                        ck, cv = (s[:layers * nkv * (b - a) * d].view(layers, nkv, b - a, d) for s in (sk, sv))
                        check(lib().mmd_kv_export(arena.h, a, b, _ptr(ck), _ptr(cv)), self._ctx, 'mmd_kv_export')
                        K[:, :, a:b].copy_(ck)          # (blocking: the staging buffers are reused by the next chunk)
                        V[:, :, a:b].copy_(cv)
        return KVSnapshot(K, V, position, self.dtype, layers, nkv, d, self._rope_inv_freq)

    def kv_load(self, snapshot: KVSnapshot, staging_bytes: int = 256 << 20) -> KVCacheHandle:
        """A handle on a fresh arena holding the snapshot's context; `kv_position` of it is the snapshot's.  The snapshot may come from another model instance,
        process or device; a dtype or fingerprint mismatch raises ValueError naming the field."""
        layers, nkv, d = self._kv_geometry()
        snapshot.check_against(self.dtype, layers, nkv, d, self._rope_inv_freq)
        n = snapshot.length
        with self._lock:
            arena = self._snapshot_arena(n)
            if n:
                chunks = snapshot_chunks(n, 2 * layers * nkv * d * snapshot.K.element_size(), staging_bytes)
                m = max(b - a for a, b in chunks)
                sk = torch.empty(layers * nkv * m * d, dtype=self.dtype, device=self.device)
                sv = torch.empty_like(sk)
                for a, b in chunks:
                    ck, cv = (s[:layers * nkv * (b - a) * d].view(layers, nkv, b - a, d) for s in (sk, sv))
                    ck.copy_(snapshot.K[:, :, a:b]); cv.copy_(snapshot.V[:, :, a:b])
                    check(lib().mmd_kv_import(arena.h, _ptr(ck), _ptr(cv), b - a), self._ctx, 'mmd_kv_import')
            check(lib().mmd_kv_set_position(arena.h, snapshot.position), self._ctx, 'mmd_kv_set_position')
        return KVCacheHandle(arena, n)

    def kv_fork(self, cache: KVCacheHandle) -> KVCacheHandle:
        """A handle on a fresh arena holding `cache`'s context (device copy, stream-ordered).  `cache` and every other handle of its arena stay valid, and nothing done
        to either arena afterwards -- steps, truncate, drop, stash -- is visible in the other."""
        src, n = self._kv_source(cache, 'kv_fork')
        with self._lock:
            arena = self._snapshot_arena(n)
            if src is not None:
                check(lib().mmd_kv_fork(arena.h, src.h, n), self._ctx, 'mmd_kv_fork')
        return KVCacheHandle(arena, n)

    def new_cache(self, initial_tokens=None):
        return KVCacheHandle(_KVArena(self, initial_tokens or self.kv_initial_tokens), 0)

    # ---- forward ----------------------------------------------------------------------------------------------------
    def __call__(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                 labels=None, informative_labels=None, relevance_labels=None, use_cache=None, output_attentions=None,
                 output_hidden_states=None, frames=None, return_dict=None, **kwargs):
        """models/live_llava/video_head_live_llava_qwen.py:121-205.  With `labels` (and the two video label tensors) the output carries the reference's
        lm_loss / video_loss / loss, computed without gradients (teacher-forced scoring); without them the call is what it was."""
        if inputs_embeds is None:
            inputs_embeds = self.joint_embed(input_ids, frames)
        if inputs_embeds.ndim != 3 or inputs_embeds.shape[0] != 1:
            raise ValueError(f'inputs_embeds must be [1, S, hidden] (streaming is batch 1), got {tuple(inputs_embeds.shape)}')
        x = inputs_embeds[0].to(device=self.device, dtype=self.dtype).contiguous()
        S = x.shape[0]
        hidden = torch.empty(S, self.config.hidden_size, dtype=self.dtype, device=self.device)
        with self._lock:
            arena, n = self._resolve_cache(past_key_values)
            self._bind_stream()
            for s0 in range(0, S, self.max_step_tokens):
                s1 = min(S, s0 + self.max_step_tokens)
                check(lib().mmd_llm_step(self._ctx, arena.h, _ptr(x[s0:s1]), s1 - s0, _ptr(hidden[s0:s1])), self._ctx, 'mmd_llm_step')
            cache = KVCacheHandle(arena, n + S)
        out = VideoHeadCausalLMOutputWithPast(self, hidden, cache)
        if labels is not None or (informative_labels is not None and relevance_labels is not None):
            self._score(out, input_ids, labels, informative_labels, relevance_labels)
        if return_dict is False:
            return (out.loss, out.logits, cache)
        return out

    forward = __call__

    @torch.no_grad()
    def _score(self, out, input_ids, labels, informative_labels, relevance_labels):
        """models/live_llava/video_head_live_llava_qwen.py:163-189: labels arrive already shifted, [1, S], -100 ignored, mean over the counted rows
        (CrossEntropyLoss() defaults); a missing part of the loss is the float 0."""
        import torch.nn.functional as F
        lm_loss = video_loss = 0.
        if labels is not None:
            if not (labels != -100).any():
                if input_ids is None:
                    raise TypeError('labels without a counted position need input_ids: labels[:, 0] = input_ids[:, 1]')
                labels[:, 0] = input_ids[:, 1]          # in the caller's tensor, as the reference does (:168-169)
            lab = labels.to(device=self.device, dtype=torch.long).flatten()
            lm_loss = self.token_nll(out._hidden, lab).sum() / (lab != -100).sum()
        if informative_labels is not None and relevance_labels is not None:
            video_labels = torch.cat([informative_labels, relevance_labels], dim=0).to(device=self.device, dtype=torch.long)
            video_logits = torch.cat([out.informative_logits, out.relevance_logits], dim=0)
            if not (video_labels != -100).any():
                video_labels[:, 0] = 0
            video_loss = F.cross_entropy(video_logits.flatten(0, 1), video_labels.flatten())
        out.lm_loss, out.video_loss = lm_loss, video_loss
        out.loss = lm_loss * self.lm_loss_weight + video_loss * self.video_loss_weight

    def token_nll(self, hidden_rows: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100, return_lse: bool = False, chunk_cols: int = 0):
        """Per-row negative log-likelihood of `labels` [M] under lm_head(hidden_rows [M,H]) -> fp32 [M] on the device, 0 where the label is `ignore_index`
        (CrossEntropyLoss(reduction='none')); with return_lse also logsumexp of every row's logits.  The [M, vocab] logits are never held: the vocabulary streams
        through a workspace of at most 64 MiB (mmd_lm_nll); chunk_cols forces the columns per pass (0 = auto).  A label outside [0, vocab) raises, as torch's loss does."""
        M = hidden_rows.shape[0]
        hidden_rows = hidden_rows.to(device=self.device, dtype=self.dtype).contiguous()
        labels = labels.to(device=self.device, dtype=torch.long).contiguous()
        if hidden_rows.ndim != 2 or hidden_rows.shape[1] != self.config.hidden_size or labels.shape != (M,):
            raise ValueError(f'token_nll takes hidden rows [M, {self.config.hidden_size}] and labels [M], got {tuple(hidden_rows.shape)} and {tuple(labels.shape)}')
        bad = (labels != ignore_index) & ((labels < 0) | (labels >= self.config.vocab_size))
        if bad.any():
            raise IndexError(f'Target {int(labels[bad][0])} is out of bounds.')
        nll = torch.empty(M, dtype=torch.float32, device=self.device)
        lse = torch.empty(M, dtype=torch.float32, device=self.device) if return_lse else None
        if M:
            with self._lock:
                self._bind_stream()
                check(lib().mmd_lm_nll(self._ctx, _ptr(hidden_rows), M, _ptr(labels), int(ignore_index), int(chunk_cols), _ptr(nll), _ptr(lse)), self._ctx, 'mmd_lm_nll')
        return (nll, lse) if return_lse else nll

    def lm_head(self, hidden_rows: torch.Tensor):
        M = hidden_rows.shape[0]
        hidden_rows = hidden_rows.contiguous()
        out = torch.empty(M, self.config.vocab_size, dtype=torch.float32, device=self.device)
        if M:
            with self._lock:
                self._bind_stream()
                check(lib().mmd_lm_head(self._ctx, _ptr(hidden_rows), M, _ptr(out)), self._ctx, 'mmd_lm_head')
        return out

    def video_heads(self, hidden_rows: torch.Tensor):
        """-> [M,4] fp32 = informative(2) | relevance(2)."""
        M = hidden_rows.shape[0]
        hidden_rows = hidden_rows.contiguous()
        out = torch.empty(M, 4, dtype=torch.float32, device=self.device)
        if M:
            with self._lock:
                self._bind_stream()
                check(lib().mmd_video_heads(self._ctx, _ptr(hidden_rows), M, _ptr(out)), self._ctx, 'mmd_video_heads')
        return out

    # ---- fused fast paths used by mmduet_amd.inference (same results as __call__ + heads) -------------------------
    def frame_step(self, inputs_embeds: torch.Tensor, past_key_values, head_rows):
        """One LLM step over `inputs_embeds` [S,H] and the 4 video-head logits at `head_rows` (list of row indices).
        Returns (numpy-like list [[inf0, inf1, rel0, rel1], ...] as a float32 CPU tensor, new handle)."""
        x = inputs_embeds.reshape(-1, self.config.hidden_size).to(device=self.device, dtype=self.dtype).contiguous()
        S = x.shape[0]
        if S > self.max_step_tokens:
            raise ValueError(f'step of {S} tokens exceeds max_step_tokens={self.max_step_tokens}')
        rows = (C.c_int32 * len(head_rows))(*[int(r) for r in head_rows])
        res = (C.c_float * (4 * len(head_rows)))()
        with self._lock:
            arena, n = self._resolve_cache(past_key_values)
            self._bind_stream()
            check(lib().mmd_frame_step(self._ctx, arena.h, _ptr(x), S, rows, len(head_rows), res), self._ctx, 'mmd_frame_step')
            cache = KVCacheHandle(arena, n + S)
        return torch.tensor(list(res), dtype=torch.float32).view(-1, 4), cache

    def multi_step(self, segments, want_logits=True):
        """ONE causal forward over several video streams (mmd_frame_step_multi): the GEMMs run once over all rows, so a stream that
        is generating token by token rides on the other streams' frame chunks instead of streaming the weights for itself.

        segments: list of dicts with
            x          [S_i, H] / [1, S_i, H] input embeddings of this stream's rows
            cache      its KV handle (or None)
            head_rows  row indices (relative to the segment) whose 4 video-head logits are wanted
            hidden     'none' | 'last' | 'all': which final hidden rows to return (and, with want_logits, run lm_head on 'last')
        Returns, per segment, dict(heads=[n,4] fp32 CPU tensor | None, hidden=[r,H] device tensor | None,
        logits=[1,V] fp32 device tensor | None, cache=new handle)."""
        H = self.config.hidden_size
        xs, seg_rows, head_rows, hid_rows, hid_slices, arenas = [], [], [], [], [], []
        at = 0
        for sg in segments:
            x = sg['x'].reshape(-1, H).to(device=self.device, dtype=self.dtype)
            S = x.shape[0]
            if S == 0:
                raise ValueError('empty segment')
            xs.append(x); seg_rows.append(S)
            head_rows += [at + int(r) for r in sg.get('head_rows', ())]
            want = sg.get('hidden', 'none')
            rows = [at + S - 1] if want == 'last' else (list(range(at, at + S)) if want == 'all' else [])
            hid_slices.append((len(hid_rows), len(rows), want))
            hid_rows += rows
            at += S
        if at > self.max_step_tokens:
            raise ValueError(f'step of {at} tokens exceeds max_step_tokens={self.max_step_tokens}')
        x_all = torch.cat(xs, dim=0).contiguous() if len(xs) > 1 else xs[0].contiguous()
        n_seg = len(segments)
        hidden_out = torch.empty(max(1, len(hid_rows)), H, dtype=self.dtype, device=self.device)
        last_idx = [i for i, (o, n, w) in enumerate(hid_slices) if w == 'last']
        # lm_head runs over the 'last' rows only; when 'all' rows are mixed in, it is done per segment afterwards
        only_last = want_logits and last_idx and all(w in ('last', 'none') for (_, _, w) in hid_slices)
        logits = torch.empty(len(hid_rows), self.config.vocab_size, dtype=torch.float32, device=self.device) if only_last else None
        res = (C.c_float * (4 * max(1, len(head_rows))))()
        with self._lock:
            for sg in segments:
                arena, n = self._resolve_cache(sg.get('cache'))
                if any(a is arena for a, _ in arenas):
                    raise ValueError('a KV arena may appear once per multi_step')
                arenas.append((arena, n))
            self._bind_stream()
            streams = (C.c_void_p * n_seg)(*[a.h for a, _ in arenas])
            rows_c = (C.c_int32 * n_seg)(*seg_rows)
            hr = (C.c_int32 * max(1, len(head_rows)))(*head_rows)
            hd = (C.c_int32 * max(1, len(hid_rows)))(*hid_rows)
            check(lib().mmd_frame_step_multi(self._ctx, streams, rows_c, n_seg, _ptr(x_all), hr, len(head_rows), res, hd, len(hid_rows),
                                             _ptr(hidden_out), _ptr(logits) if logits is not None else None), self._ctx, 'mmd_frame_step_multi')
            caches = [KVCacheHandle(a, n + S) for (a, n), S in zip(arenas, seg_rows)]
        heads_all = torch.tensor(list(res)[:4 * len(head_rows)], dtype=torch.float32).view(-1, 4)
        out, hp = [], 0
        for i, sg in enumerate(segments):
            nh = len(sg.get('head_rows', ()))
            o, n, want = hid_slices[i]
            hid = hidden_out[o:o + n] if n else None
            lg = None
            if want == 'last' and want_logits:
                lg = logits[o:o + 1] if logits is not None else self.lm_head(hid)
            out.append(dict(heads=heads_all[hp:hp + nh] if nh else None, hidden=hid, logits=lg, cache=caches[i]))
            hp += nh
        return out

    def new_sampler(self):
        """Device-resident greedy sampling state of one stream (mmd_sampler): the token drawn last + the repetition-penalty list."""
        return SamplerHandle(self)

    def round_multi(self, segments):
        """ONE scheduler round over several video streams with the sampling on the device (mmd_round_multi): `multi_step` for the rows, plus -- for the streams that are
        talking -- lm_head, repetition penalty, arg-max and the next round's embedding gather without a host round trip.  One synchronisation per round.

        segments: list of dicts with
            x          [S_i, H] / [1, S_i, H] input rows, or None with feed=True
            cache      the stream's KV handle (or None)
            head_rows  row indices (relative to the segment) whose 4 video-head logits are wanted
            sampler    a SamplerHandle (needed for feed / sample)
            feed       the segment is the ONE row of the token `sampler` drew in an earlier round
            sample     draw the next token from the segment's last row
        Returns per segment dict(heads=[n,4] fp32 CPU tensor | None, token=int | None, cache=new handle)."""
        H = self.config.hidden_size
        n_seg = len(segments)
        seg_rows, head_rows, ptrs, flags, samplers, keep = [], [], [], [], [], []
        at = 0
        for sg in segments:
            feed, smp = bool(sg.get('feed')), sg.get('sampler')
            if feed:
                S = 1; ptrs.append(None)
            else:
                x = sg['x'].reshape(-1, H)
                if x.dtype != self.dtype or x.device != self.device or not x.is_contiguous():
                    x = x.to(device=self.device, dtype=self.dtype).contiguous()
                S = x.shape[0]
                if S == 0:
                    raise ValueError('empty segment')
                keep.append(x); ptrs.append(x.data_ptr())
            seg_rows.append(S)
            head_rows += [at + int(r) for r in sg.get('head_rows', ())]
            flags.append((1 if feed else 0) | (2 if sg.get('sample') else 0))
            samplers.append(smp.h if smp is not None else None)
            at += S
        if at > self.max_step_tokens:
            raise ValueError(f'round of {at} tokens exceeds max_step_tokens={self.max_step_tokens}')
        nh = len(head_rows)
        res = (C.c_float * (4 * max(1, nh)))()
        toks = (C.c_int64 * n_seg)()
        arenas = []
        with self._lock:
            for sg in segments:
                arena, n = self._resolve_cache(sg.get('cache'))
                if any(a is arena for a, _ in arenas):
                    raise ValueError('a KV arena may appear once per round')
                arenas.append((arena, n))
            self._bind_stream()
            check(lib().mmd_round_multi(self._ctx, (C.c_void_p * n_seg)(*[a.h for a, _ in arenas]), (C.c_int32 * n_seg)(*seg_rows), n_seg, (C.c_void_p * n_seg)(*ptrs),
                                        (C.c_void_p * n_seg)(*samplers), (C.c_int32 * n_seg)(*flags), (C.c_int32 * max(1, nh))(*head_rows), nh, res, toks),
                  self._ctx, 'mmd_round_multi')
            caches = [KVCacheHandle(a, n + S) for (a, n), S in zip(arenas, seg_rows)]
        heads_all = torch.tensor(res[:4 * nh], dtype=torch.float32).view(-1, 4) if nh else None
        out, hp = [], 0
        for i, sg in enumerate(segments):
            k = len(sg.get('head_rows', ()))
            out.append(dict(heads=heads_all[hp:hp + k] if k else None, token=int(toks[i]) if flags[i] & 2 else None, cache=caches[i]))
            hp += k
        return out

    def _native_generate(self, inputs_embeds, past_key_values, eos_token_id, max_new_tokens, repetition_penalty, generated_token_ids, sampling=None):
        """The marshalling of mmd_greedy_generate (sampling None) / mmd_sample_generate (sampling = (temperature, top_k, top_p, seed, offset, lane)):
        -> (ids, cache, offset behind the last draw).  `generated_token_ids` is read and written back only when the penalty is > 0."""
        x = inputs_embeds.reshape(-1, self.config.hidden_size).to(device=self.device, dtype=self.dtype).contiguous()
        S = x.shape[0]
        if S == 0:
            raise ValueError('empty prompt')
        pen = float(repetition_penalty) if repetition_penalty is not None else 0.0
        grow = generated_token_ids is not None and pen > 0
        prev = list(generated_token_ids) if grow else []
        cap = len(prev) + max_new_tokens + 1
        prev_arr = (C.c_int64 * cap)(*prev)
        n_prev = C.c_int(len(prev))
        out_ids = (C.c_int64 * max_new_tokens)()
        n_out = C.c_int(0)
        eos = int(eos_token_id if eos_token_id is not None else -1)
        off = C.c_uint64(0)
        with self._lock:
            arena, n = self._resolve_cache(past_key_values)
            self._bind_stream()
            if sampling is None:
                check(lib().mmd_greedy_generate(self._ctx, arena.h, _ptr(x), S, eos, pen, prev_arr, C.byref(n_prev), cap, out_ids, int(max_new_tokens), C.byref(n_out)),
                      self._ctx, 'mmd_greedy_generate')
            else:
                temperature, top_k, top_p, seed, offset, lane = sampling
                off.value = int(offset)
                check(lib().mmd_set_sample_lane(self._ctx, int(lane)), self._ctx, 'mmd_set_sample_lane')
                check(lib().mmd_sample_generate(self._ctx, arena.h, _ptr(x), S, eos, pen, prev_arr, C.byref(n_prev), cap, float(temperature), int(top_k or 0), float(top_p),
                                                int(seed) & _U64, C.byref(off), out_ids, max_new_tokens, C.byref(n_out)), self._ctx, 'mmd_sample_generate')
            cache = KVCacheHandle(arena, arena.length())
            self._last_logprobs = self._read_generate_logprobs(n_out.value) if self._logprobs_top >= 0 else None
        ids = [int(out_ids[i]) for i in range(n_out.value)]
        if grow:
            generated_token_ids[:] = [int(prev_arr[i]) for i in range(n_prev.value)]
        return ids, cache, int(off.value)

    def set_generate_logprobs(self, top_n=-1):
        """mmd_set_generate_logprobs: the following greedy_generate / sample_generate calls record per-token log-probabilities with `top_n` (0..8) alternatives
        (DESIGN.md "Log-probabilities"); -1 or None switches the recording off (the default)."""
        top_n = -1 if top_n is None else int(top_n)
        with self._lock:
            check(lib().mmd_set_generate_logprobs(self._ctx, top_n), self._ctx, 'mmd_set_generate_logprobs')
            self._logprobs_top = top_n

    def set_generate_constraints(self, constraints=None, *, eos_token_id=None, min_new_tokens=None, suppress_tokens=None, bad_words_ids=None, sequence_bias=None):
        """mmd_set_generate_constraints: the following greedy_generate / sample_generate calls decode under the constraints (DESIGN.md "Constraints") -- an EOS set of up to 8
        ids (the calls' own eos_token_id is then ignored), min_new_tokens, suppressed ids, single-token bad_words_ids and sequence_bias.  Either a constraints.Constraints or
        the HF-shaped keywords; nothing (or a set that constrains nothing) switches them off, the default.  Returns what was set before."""
        if constraints is None:
            constraints = _constraints.merge(self.config.vocab_size, eos_token_id, min_new_tokens, suppress_tokens, bad_words_ids, sequence_bias)
        if not constraints.on:
            constraints = None
        with self._lock:
            was = getattr(self, '_constraints', None)
            if constraints is not None or was is not None:
                check(lib().mmd_set_generate_constraints(self._ctx, *_constraints.c_arrays(constraints)), self._ctx, 'mmd_set_generate_constraints')
            self._constraints = constraints
        return was

    def _read_generate_logprobs(self, n_tokens):
        top = self._logprobs_top
        lp, slp = torch.empty(n_tokens, dtype=torch.float32), torch.empty(n_tokens, dtype=torch.float32)
        top_lp, top_ids = torch.empty(n_tokens, top, dtype=torch.float32), torch.empty(n_tokens, top, dtype=torch.long)
        n = C.c_int(0)
        check(lib().mmd_generate_logprobs_read(self._ctx, _ptr(lp), _ptr(slp), _ptr(top_ids), _ptr(top_lp), int(n_tokens), C.byref(n)), self._ctx, 'mmd_generate_logprobs_read')
        if n.value != n_tokens:
            raise RuntimeError(f'{n.value} log-probability records for {n_tokens} tokens')
        return dict(logprobs=lp, sampling_logprobs=slp, top_logprobs=top_lp, top_logprob_ids=top_ids)

    def last_generate_logprobs(self):
        """The records of the most recent native generate call of this model as CPU tensors -- logprobs [n], sampling_logprobs [n], top_logprobs [n, top_n],
        top_logprob_ids [n, top_n] -- or None if that call did not record (set_generate_logprobs)."""
        return self._last_logprobs

    def greedy_generate(self, inputs_embeds, past_key_values, eos_token_id, max_new_tokens, repetition_penalty=None,
                        generated_token_ids=None):
        """mmd_greedy_generate: -> (ids, cache).  NaN logits raise ValueError, as in `sample_generate`: no id is made up for such a step."""
        return self._native_generate(inputs_embeds, past_key_values, eos_token_id, max_new_tokens, repetition_penalty, generated_token_ids)[:2]

    def sample_generate(self, inputs_embeds, past_key_values, eos_token_id, max_new_tokens, repetition_penalty=None, generated_token_ids=None,
                        temperature=1.0, top_k=0, top_p=1.0, seed=0, offset=0, lane=0):
        """mmd_sample_generate, `greedy_generate` with a draw in the arg-max's place: -> (ids, cache, offset behind the last draw).  Draw i uses the Philox word of
        (seed, offset + i, lane).  Zero new tokens posts nothing; the penalty list is extended only when the penalty is > 0.  NaN logits raise ValueError."""
        max_new_tokens = int(max_new_tokens)
        if max_new_tokens <= 0:
            return [], past_key_values, int(offset)
        return self._native_generate(inputs_embeds, past_key_values, eos_token_id, max_new_tokens, repetition_penalty, generated_token_ids,
                                     (temperature, top_k, top_p, seed, offset, lane))

    def decode_last_route(self):
        """What the decode steps of the most recent greedy_generate / sample_generate did (mmd_op_decode_last_route): 0 none or launched one by one,
        1 replayed an existing captured step, 2 captured the step in that call, then replayed it."""
        return int(lib().mmd_op_decode_last_route(self._ctx))

    STEP_PLAN_FIELDS = ('schedule', 'rope_fused', 'chunk_rope', 'sparse_last', 'run0', 'run_n', 'run_all', 'down_slab_norm', 'mlp_pm')

    def step_last_plan(self):
        """The schedule the most recent LLM step took (mmd_op_step_last_plan): a dict over STEP_PLAN_FIELDS; schedule 0 tile, 1 fused slabs, 2 decode chain."""
        out = (C.c_int * len(self.STEP_PLAN_FIELDS))()
        check(lib().mmd_op_step_last_plan(self._ctx, out), self._ctx, 'step_last_plan')
        return dict(zip(self.STEP_PLAN_FIELDS, out))

    TOWER_PLAN_FIELDS = ('dt', 'resid', 'embed', 'sparse_last', 'pout', 'U', 'compact_rows', 'proj_compact', 'proj_gather', 'mlp_pm', 'mlp_pm_last', 'final_convert')

    def tower_last_plan(self):
        """The schedule the most recent vision-tower run took (mmd_op_tower_last_plan): a dict over TOWER_PLAN_FIELDS; dt 0 fp32, 1 bf16, 2 IEEE half; resid 0 the GEMM
        epilogue adds, 1 fp32 residual stream, 2 epilogue add in half; embed 0 add rows, 1 class token, 2 fp32 stream.  vit_debug_tap refuses exactly when sparse_last is set."""
        out = (C.c_int * len(self.TOWER_PLAN_FIELDS))()
        check(lib().mmd_op_tower_last_plan(self._ctx, out), self._ctx, 'tower_last_plan')
        return dict(zip(self.TOWER_PLAN_FIELDS, out))

    SELECT_PLAN_FIELDS = ('kind', 'single', 'any_k', 'any_p', 'needs_row', 'needs_cons', 'record', 'scores_after_argmax', 'record_greedy', 'advance')
    GENERATE_PLAN_FIELDS = ('can_graph', 'upload_state', 'post_row_dynamic', 'post_row_each_eager_step', 'post_cons_dynamic', 'post_cons_each_eager_step', 'host_appends_penalty',
                            'pen_key_is_value', 'key_sel', 'key_lp', 'key_cons_gen')
    ROUND_BLOCKS_FIELDS = ('n_plain', 'n_greedy', 'n_sample', 'any_k', 'any_p', 'any_cons_sampled')

    def select_last_plan(self):
        """The plan the most recent token selection was launched from (mmd_op_select_last_plan): dict(select=..., generate=... | None, round=... | None) over the three field
        lists above; kind 0 arg-max, 1 constrained arg-max, 2 draw.  generate / round: the plan of the generate call / round the selection belonged to."""
        ns, ng = len(self.SELECT_PLAN_FIELDS), len(self.GENERATE_PLAN_FIELDS)
        out = (C.c_int * (ns + 1 + ng))()
        check(lib().mmd_op_select_last_plan(self._ctx, out), self._ctx, 'select_last_plan')
        tail = out[ns + 1:]
        return dict(select=dict(zip(self.SELECT_PLAN_FIELDS, out[:ns])), generate=dict(zip(self.GENERATE_PLAN_FIELDS, tail)) if out[ns] == 1 else None,
                    round=dict(zip(self.ROUND_BLOCKS_FIELDS, tail)) if out[ns] == 2 else None)

    ROUND_RECORD_FIELDS = ('plain', 'constrained', 'sampled', 'top_n')

    def round_last_record(self):
        """What the most recent round recorded (mmd_op_round_last_record): the recording rows of its plain arg-max, constrained arg-max and sampled blocks, and the
        largest top_n among them (-1: no row recorded)."""
        out = (C.c_int * len(self.ROUND_RECORD_FIELDS))()
        check(lib().mmd_op_round_last_record(self._ctx, out), self._ctx, 'round_last_record')
        return dict(zip(self.ROUND_RECORD_FIELDS, out))

    @torch.no_grad()
    def generate(self, input_ids=None, inputs_embeds=None, frames=None, past_key_values=None, max_new_tokens=20, do_sample=False, temperature=1.0, top_k=50, top_p=1.0,
                 repetition_penalty=None, eos_token_id=None, seed=None, return_dict_in_generate=False, output_logprobs=False, top_logprobs=0, **kwargs):
        """models/live_llava/video_head_live_llava_qwen.py:210-242 (HF `generate` for batch 1).  do_sample=False is the greedy path; do_sample=True draws with temperature,
        top-k and top-p on the device (DESIGN.md "Sampling"), seeded by `seed` (None: one draw from torch.initial_seed() per call).  Returns a LongTensor [1, n]: with
        `input_ids` the prompt followed by the new tokens, with `inputs_embeds` only the new tokens; with return_dict_in_generate an object with .sequences and
        .past_key_values.  output_logprobs=True (dict form only) adds the per-token log-probabilities recorded by the native loop, with `top_logprobs` (0..8) alternatives per
        token (GenerateOutput).  Arguments that ask for what is not built (beam search, min_p, typical_p, ...) raise NotImplementedError."""
        top_logprobs = int(top_logprobs or 0)
        if output_logprobs and not return_dict_in_generate:
            raise ValueError('generate: output_logprobs needs return_dict_in_generate=True (a plain id tensor has no place for them)')
        if top_logprobs and not output_logprobs:
            raise ValueError('generate: top_logprobs needs output_logprobs=True')
        if not 0 <= top_logprobs <= 8:
            raise ValueError('generate: top_logprobs is 0..8')
        if 'max_length' in kwargs and kwargs['max_length'] is not None:
            raise NotImplementedError('generate: max_length is not supported, pass max_new_tokens')
        kwargs.pop('max_length', None)
        cons_kw = {k: kwargs.pop(k) for k in _GENERATE_CONSTRAINTS if k in kwargs}
        for k, v in kwargs.items():
            if k in _GENERATE_IGNORED:
                continue
            if k not in _GENERATE_OFF:
                raise NotImplementedError(f'generate: argument {k!r} is not supported')
            if v is not None and v != _GENERATE_OFF[k]:
                raise NotImplementedError(f'generate: {k}={v!r} is not supported')
        if eos_token_id is None:
            eos_token_id = getattr(self.config, 'eos_token_id', None)
        if isinstance(eos_token_id, (list, tuple)):
            eos_token_id = list(dict.fromkeys(int(t) for t in eos_token_id))
            if len(eos_token_id) <= 1:
                eos_token_id = eos_token_id[0] if eos_token_id else None
        # one EOS id and nothing else asked for: the unconstrained loop, as before.  Otherwise the merged set holds for this call (a set switched on for the bare loops is put back)
        cons = _constraints.merge(self.config.vocab_size, eos_token_id if isinstance(eos_token_id, list) else None, **cons_kw)
        if isinstance(eos_token_id, list):
            eos_token_id = eos_token_id[0]          # (ignored by the native call: the set is given)
        prompt = input_ids
        if inputs_embeds is None:
            if input_ids is None:
                raise ValueError('generate needs input_ids or inputs_embeds')
            if input_ids.ndim == 1:
                input_ids = input_ids[None]
            inputs_embeds = self.joint_embed(input_ids, frames)
        if inputs_embeds.ndim == 2:
            inputs_embeds = inputs_embeds[None]
        if inputs_embeds.shape[0] != 1:
            raise NotImplementedError('generate: batch size 1 only (streaming is batch 1)')
        pen = float(repetition_penalty) if repetition_penalty not in (None, 1.0) else None
        max_new_tokens = int(max_new_tokens)
        cons_was = self.set_generate_constraints(cons) if (cons.on or self._constraints is not None) else None
        was = self._logprobs_top
        if output_logprobs or was >= 0:          # (this call's own setting; a recording switched on for the bare loops is put back afterwards)
            self.set_generate_logprobs(top_logprobs if output_logprobs else -1)
        try:
            if max_new_tokens <= 0:
                ids, cache = [], past_key_values
                rec = dict(logprobs=torch.empty(0), sampling_logprobs=torch.empty(0), top_logprobs=torch.empty(0, top_logprobs), top_logprob_ids=torch.empty(0, top_logprobs, dtype=torch.long))
            elif not do_sample:
                ids, cache = self.greedy_generate(inputs_embeds, past_key_values, eos_token_id, max_new_tokens, pen, [] if pen else None)
                rec = self._last_logprobs
            else:
                if seed is None:
                    seed = torch.initial_seed()
                ids, cache, _ = self.sample_generate(inputs_embeds, past_key_values, eos_token_id, max_new_tokens, pen, [] if pen else None,
                                                     temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
                rec = self._last_logprobs
        finally:
            if self._logprobs_top != was:
                self.set_generate_logprobs(was)
            if cons.on or cons_was is not None:
                self.set_generate_constraints(cons_was or _constraints.OFF)
        new = torch.tensor([ids], dtype=torch.long, device=self.device).view(1, -1)
        seq = new if prompt is None else torch.cat([prompt.reshape(1, -1).to(device=self.device, dtype=torch.long), new], dim=1)
        if not return_dict_in_generate:
            return seq
        if not output_logprobs:
            return GenerateOutput(seq, cache)
        return GenerateOutput(seq, cache, **{k: v[None] for k, v in rec.items()})

    def generate_after_embed(self, input_ids, frames, **kwargs):
        """models/live_llava/video_head_live_llava_qwen.py:207-208: generate over joint_embed(input_ids, frames); like HF with inputs_embeds only, the new tokens are returned."""
        return self.generate(inputs_embeds=self.joint_embed(input_ids, frames), **kwargs)

    def sample_op(self, logits, temperature=1.0, top_k=0, top_p=1.0, seed=0, offset=0, r=None, prev_ids=None, repetition_penalty=None, return_scores=False):
        """The sampling chain on rows of fp32 logits [n, V] (mmd_op_sample; row i draws on lane i).  r: None = Philox words, else n explicit 64-bit random words.
        -> (tokens int64 [n], info fp32 [n, 4] = (tau, kept count, kept mass / total mass, NaN flag), scores [n, V] or None), on the device."""
        lg = logits.to(device=self.device, dtype=torch.float32).contiguous()
        if lg.ndim == 1:
            lg = lg[None]
        n, V = lg.shape
        toks = torch.empty(n, dtype=torch.long, device=self.device)
        info = torch.empty(n, 4, dtype=torch.float32, device=self.device)
        scores = torch.empty(n, V, dtype=torch.float32, device=self.device) if return_scores else None
        prev = torch.as_tensor(prev_ids, dtype=torch.long).to(self.device).contiguous() if prev_ids is not None and len(prev_ids) else None
        r_arr = None
        if r is not None:
            if len(r) != n:
                raise ValueError('one random word per row')
            r_arr = (C.c_uint64 * n)(*[int(v) & _U64 for v in r])
        with self._lock:
            self._bind_stream()
            check(lib().mmd_op_sample(self._ctx, _ptr(lg), n, V, _ptr(prev), 0 if prev is None else prev.numel(), float(repetition_penalty or 0.0), float(temperature),
                                      int(top_k or 0), float(top_p), int(seed) & _U64, int(offset) & _U64, r_arr, _ptr(toks), _ptr(info), _ptr(scores)), self._ctx, 'mmd_op_sample')
        return toks, info, scores

    def sample_logprob_op(self, logits, temperature=1.0, top_k=0, top_p=1.0, seed=0, offset=0, r=None, prev_ids=None, repetition_penalty=None, greedy=False, top_n=0,
                          return_scores=False):
        """`sample_op` with the rows' log-probability records (mmd_op_sample_logprobs).  greedy: the arg-max with penalty stands in the draw's place (info is None then).
        -> (tokens [n], info [n, 4] or None, scores [n, V] or None) on the device and, as CPU tensors, lp fp32 [n, 2] = (logprob, sampling_logprob), top ids int64 [n, top_n],
        top logprobs fp32 [n, top_n]."""
        lg = logits.to(device=self.device, dtype=torch.float32).contiguous()
        if lg.ndim == 1:
            lg = lg[None]
        n, V = lg.shape
        top_n = int(top_n)
        toks = torch.empty(n, dtype=torch.long, device=self.device)
        info = None if greedy else torch.empty(n, 4, dtype=torch.float32, device=self.device)
        scores = torch.empty(n, V, dtype=torch.float32, device=self.device) if return_scores else None
        prev = torch.as_tensor(prev_ids, dtype=torch.long).to(self.device).contiguous() if prev_ids is not None and len(prev_ids) else None
        lp, top_ids, top_lp = torch.empty(n, 2, dtype=torch.float32), torch.empty(n, max(top_n, 0), dtype=torch.long), torch.empty(n, max(top_n, 0), dtype=torch.float32)
        r_arr = None
        if r is not None:
            if len(r) != n:
                raise ValueError('one random word per row')
            r_arr = (C.c_uint64 * n)(*[int(v) & _U64 for v in r])
        with self._lock:
            self._bind_stream()
            check(lib().mmd_op_sample_logprobs(self._ctx, _ptr(lg), n, V, _ptr(prev), 0 if prev is None else prev.numel(), float(repetition_penalty or 0.0), float(temperature),
                                               int(top_k or 0), float(top_p), int(seed) & _U64, int(offset) & _U64, r_arr, int(bool(greedy)), top_n, _ptr(toks), _ptr(info),
                                               _ptr(scores), _ptr(lp), _ptr(top_ids), _ptr(top_lp)), self._ctx, 'mmd_op_sample_logprobs')
        return toks, info, scores, lp, top_ids, top_lp

    def sample_constrained_op(self, logits, constraints, steps=0, temperature=1.0, top_k=0, top_p=1.0, seed=0, offset=0, r=None, prev_ids=None, repetition_penalty=None,
                              greedy=False, top_n=None, return_scores=False):
        """`sample_logprob_op` under constraints (mmd_op_sample_constrained).  constraints: one constraints.Constraints for every row or a list of one per row; steps: the
        tokens returned so far, an int or one per row.  top_n None: no records (lp / top ids / top logprobs are None), else 0..8.  ValueError when a row has nothing to draw
        from.  -> (tokens [n], info [n, 4] or None, scores [n, V] or None, lp [n, 2], top ids, top logprobs)."""
        lg = logits.to(device=self.device, dtype=torch.float32).contiguous()
        if lg.ndim == 1:
            lg = lg[None]
        n, V = lg.shape
        cons = [constraints] * n if isinstance(constraints, _constraints.Constraints) else list(constraints)
        steps = [int(steps)] * n if isinstance(steps, int) else [int(v) for v in steps]
        if len(cons) != n or len(steps) != n:
            raise ValueError('one constraint set and one step per row')
        off = [0]
        for cs in cons:
            off.append(off[-1] + len(cs.ids))
        eos = [([int(t) for t in cs.eos] + [-1] * 8)[:max(8, len(cs.eos))] for cs in cons]
        if any(len(e) > 8 for e in eos):
            raise ValueError('at most 8 EOS ids per row')
        flat_ids = [t for cs in cons for t in cs.ids]
        flat_bias = [b for cs in cons for b in cs.bias]
        toks = torch.empty(n, dtype=torch.long, device=self.device)
        info = None if greedy else torch.empty(n, 4, dtype=torch.float32, device=self.device)
        scores = torch.empty(n, V, dtype=torch.float32, device=self.device) if return_scores else None
        prev = torch.as_tensor(prev_ids, dtype=torch.long).to(self.device).contiguous() if prev_ids is not None and len(prev_ids) else None
        rec = top_n is not None
        tn = int(top_n or 0)
        lp = torch.empty(n, 2, dtype=torch.float32) if rec else None
        top_ids = torch.empty(n, tn, dtype=torch.long) if rec else None
        top_lp = torch.empty(n, tn, dtype=torch.float32) if rec else None
        r_arr = None
        if r is not None:
            if len(r) != n:
                raise ValueError('one random word per row')
            r_arr = (C.c_uint64 * n)(*[int(v) & _U64 for v in r])
        with self._lock:
            self._bind_stream()
            check(lib().mmd_op_sample_constrained(self._ctx, _ptr(lg), n, V, _ptr(prev), 0 if prev is None else prev.numel(), float(repetition_penalty or 0.0), float(temperature),
                                                  int(top_k or 0), float(top_p), int(seed) & _U64, int(offset) & _U64, r_arr, int(bool(greedy)), tn,
                                                  (C.c_int32 * (n + 1))(*off), (C.c_int32 * max(1, len(flat_ids)))(*flat_ids), (C.c_float * max(1, len(flat_bias)))(*flat_bias),
                                                  (C.c_int64 * (8 * n))(*[t for e in eos for t in e]), (C.c_int32 * n)(*[len(cs.eos) for cs in cons]),
                                                  (C.c_int32 * n)(*[int(cs.min_new) for cs in cons]), (C.c_int32 * n)(*steps),
                                                  _ptr(toks), _ptr(info), _ptr(scores), _ptr(lp), _ptr(top_ids), _ptr(top_lp)), self._ctx, 'mmd_op_sample_constrained')
        return toks, info, scores, lp, top_ids, top_lp

    # ---- measurement --------------------------------------------------------------------------------------------------
    def prof_enable(self, classes=True):
        """classes: True = all kernel classes, False = off, or an iterable of class names from _lib.K_NAMES."""
        if classes is True:
            mask = (1 << len(_lib.K_NAMES)) - 1
        elif not classes:
            mask = 0
        else:
            mask = sum(1 << _lib.K_NAMES.index(k) for k in classes)
        check(lib().mmd_prof_enable(self._ctx, mask), self._ctx)

    def prof_set_stride(self, stride):
        check(lib().mmd_prof_set_stride(self._ctx, int(stride)), self._ctx)

    def prof_reset(self):
        check(lib().mmd_prof_reset(self._ctx), self._ctx)

    def prof_read(self):
        n = len(_lib.K_NAMES)
        ms, cnt, by, fl = (C.c_double * n)(), (C.c_int64 * n)(), (C.c_double * n)(), (C.c_double * n)()
        check(lib().mmd_prof_read(self._ctx, ms, cnt, by, fl), self._ctx)
        return {k: dict(ms=ms[i], launches=cnt[i], bytes=by[i], flops=fl[i]) for i, k in enumerate(_lib.K_NAMES)}


# ----------------------------------------------------------------------------------------------------------------
def fast_greedy_generate(*, model, inputs_embeds: torch.Tensor, past_key_values, eos_token_id: int, inplace_output_ids: torch.Tensor,
                         repetition_penalty=None, generated_token_ids=None):
    """models/modeling_live.py:51-77, same signature and return triple.  The token loop runs natively
    (mmd_greedy_generate): argmax (+ HF repetition penalty over `generated_token_ids`) on the device, EOS written but
    neither fed back nor penalised."""
    if repetition_penalty is not None:
        assert isinstance(repetition_penalty, float)
    if generated_token_ids is None:
        generated_token_ids = list()
    max_new = inplace_output_ids.size(1)
    if not hasattr(model, 'greedy_generate') or getattr(model, 'python_generate_loop', False):
        return _greedy_generate_by_calls(model, inputs_embeds, past_key_values, eos_token_id, inplace_output_ids,
                                         repetition_penalty, generated_token_ids)
    ids, cache = model.greedy_generate(inputs_embeds, past_key_values, eos_token_id, max_new, repetition_penalty, generated_token_ids)
    return _write_ids(inplace_output_ids, ids), cache, generated_token_ids


def fast_sample_generate(*, model, inputs_embeds: torch.Tensor, past_key_values, eos_token_id: int, inplace_output_ids: torch.Tensor, repetition_penalty=None,
                         generated_token_ids=None, temperature=1.0, top_k=0, top_p=1.0, seed=0, offset=0):
    """`fast_greedy_generate` with a draw per token (mmd_sample_generate, or the scheduler rounds behind a multi-stream proxy): -> (ids, cache, generated_token_ids,
    the Philox offset behind the last draw).  There is no host fallback: a model without `sample_generate` is an error."""
    if generated_token_ids is None:
        generated_token_ids = list()
    ids, cache, offset = model.sample_generate(inputs_embeds, past_key_values, eos_token_id, inplace_output_ids.size(1), repetition_penalty, generated_token_ids,
                                               temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, offset=offset)
    return _write_ids(inplace_output_ids, ids), cache, generated_token_ids, offset


def _write_ids(inplace_output_ids, ids):
    n = len(ids)
    inplace_output_ids[:, :n] = torch.tensor(ids, dtype=inplace_output_ids.dtype, device=inplace_output_ids.device)
    return inplace_output_ids[:, :n]


def _greedy_generate_by_calls(model, x, cache, eos_token_id, out_ids, penalty, seen):
    """Token loop through the public model call (any duck-typed model; also the cross-check of the native loop)."""
    n = 0
    for n in range(out_ids.size(1)):
        res = model(inputs_embeds=x, past_key_values=cache, use_cache=True, return_dict=True)
        cache = res.past_key_values
        scores = res.logits[0, -1].float().clone()
        if penalty is not None and seen:
            idx = torch.as_tensor(seen, dtype=torch.long, device=scores.device)
            picked = scores[idx]
            scores[idx] = torch.where(picked < 0, picked * penalty, picked / penalty)
        tok = int(scores.argmax(-1))
        if penalty is not None and tok != eos_token_id:
            seen.append(tok)
        out_ids[:, n] = tok
        if tok == eos_token_id:
            break
        x = model.get_input_embeddings()(torch.tensor([[tok]], device=out_ids.device))
    return out_ids[:, :n + 1], cache, seen


def build_live(*, is_training: bool, config_class=VideoHeadLiveLlavaQwenConfig, model_class=VideoHeadLiveLlavaQwenForCausalLM,
               llm_pretrained: str = None, lora_pretrained: str = None, finetune_modules=None, lora_modules: str = None,
               lora_r: int = None, lora_alpha: int = None, set_vision_inside: bool = False,
               attn_implementation: str = 'flash_attention_2', torch_dtype='auto', **kwargs):
    """models/modeling_live.py:80-129 for inference.  `llm_pretrained` is a local checkpoint directory / hub id of a
    LLaVA-OneVision-Qwen2 checkpoint, or 'synthetic:<seed>' for seeded random weights at the configured shape."""
    from .weights import load_pretrained_into, load_lora_into, synthetic_weights
    if is_training:
        raise NotImplementedError('training is out of scope of the MI355X inference implementation')
    if torch_dtype == 'auto' or torch_dtype is None:
        torch_dtype = torch.bfloat16
    runtime = {k: kwargs.pop(k) for k in ('max_vit_batch', 'max_step_tokens', 'kv_initial_tokens') if k in kwargs}
    # workspace sizing from the driver flags: rows of one LLM forward (frames_per_forward chunks) and the KV arena
    fpf = int(kwargs.get('frames_per_forward', 1) or 1)
    nt = int(kwargs.get('frame_num_tokens', 49) or 49)
    runtime.setdefault('max_step_tokens', max(1024, fpf * nt + 256))
    if kwargs.get('kv_capacity_tokens'):
        runtime.setdefault('kv_initial_tokens', int(kwargs['kv_capacity_tokens']))
    elif kwargs.get('max_num_frames'):
        runtime.setdefault('kv_initial_tokens', max(32768, int(kwargs['max_num_frames']) * nt + 4096))
    if llm_pretrained.startswith('synthetic'):
        config = config_class(**kwargs)
    else:
        config = config_class.from_pretrained(llm_pretrained, **kwargs)
    model = model_class(config, torch_dtype=torch_dtype, **runtime)
    tokenizer = build_live_tokenizer_and_update_config(llm_pretrained, model.config)
    if llm_pretrained.startswith('synthetic'):
        seed = int(llm_pretrained.split(':')[1]) if ':' in llm_pretrained and llm_pretrained.split(':')[1].isdigit() else 0
        for name, t in synthetic_weights(config, seed=seed, device=model.device, dtype=torch_dtype):
            model.load_tensor(name, t)
    else:
        load_pretrained_into(model, llm_pretrained)
    if lora_pretrained:
        load_lora_into(model, lora_pretrained)
    else:
        import warnings
        warnings.warn(f'!!! Fail to load lora from checkpoint: {lora_pretrained}. Return a new initialized model.')
    model.finalize()
    return model, tokenizer


def build_model_and_tokenizer(is_training, **kwargs):
    """models/__init__.py:8-13."""
    llm_pretrained = kwargs.get('llm_pretrained', None)
    if llm_pretrained is not None and ('llava' in llm_pretrained or llm_pretrained.startswith('synthetic')):
        return build_live(is_training=is_training, **kwargs)
    raise NotImplementedError(f'Not support {llm_pretrained}')
