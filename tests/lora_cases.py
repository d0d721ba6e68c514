"""The LoRA / weight-intake path stated on the host, for tests/test_lora_host.py (CPU) and tests/test_gpu_lora.py.

  * merge_ref64 / merge_bound: what mmd_merge_lora must write into one matrix, in float64, and how far an fp32 (or fp32-then-bf16) evaluation may be from it;
  * pair / adapter: seeded adapters whose update has a stated size against the matrix it lands on (rel = rms(s B A) / rms(W));
  * KERNEL_CASES: merges that are read back bit for bit (embedding table through mmd_embed_tokens, both head matrices through mmd_video_heads on an identity);
  * CONVERT_VALUES: the bit patterns mmd_load_tensor's conversions are checked on;
  * MODEL_CASES / MODES: adapters over the seven decoder targets, checked through the finalized model against the oracle on float64-merged weights.

Nothing here needs a GPU."""
import functools
import json
import math
import os
import torch
from oracle import duet_oracle as O

TARGETS = ('q_proj', 'k_proj', 'v_proj', 'o_proj', 'gate_proj', 'up_proj', 'down_proj')
R, ALPHA = 16, 32                      # the reference's adapter defaults (models/arguments_live.py:13-15): scale = alpha / r = 2
EMBED, INF, REL = 'model.embed_tokens.weight', 'informative_head.weight', 'relevance_head.weight'
PROJECTOR = ('model.mm_projector.0.weight', 'model.mm_projector.0.bias', 'model.mm_projector.2.weight', 'model.mm_projector.2.bias')


def weight_name(layer, target):
    return f"model.layers.{layer}.{'mlp' if target in ('gate_proj', 'up_proj', 'down_proj') else 'self_attn'}.{target}.weight"


def rms(t):
    return t.double().pow(2).mean().sqrt().item()


# ---- one matrix -----------------------------------------------------------------------------------------------------------------------------
def merge_ref64(W, A, B, scale):
    return W.double() + scale * (B.double() @ A.double())


def bf16_half_ulp(x):
    """Half the bf16 spacing at x (float64): 2^(floor(log2|x|) - 8), the subnormal spacing below 2^-126 (and at 0)."""
    _, e = torch.frexp(x.abs())                                   # |x| = m 2^e with m in [0.5, 1): floor(log2|x|) = e - 1
    fl = torch.where(x == 0, torch.full_like(e, -126), e - 1).clamp(min=-126)
    return torch.ldexp(torch.ones_like(x), fl - 8)


def merge_bound(W, A, B, scale, r, dtype):
    """Elementwise bound on |stored - merge_ref64|.  fp32: r multiply-adds, one multiply by the scale and one add, each rounded to fp32 (or fused): first order
    (r + 2) u (|W| + |s| sum_k |B_ok| |A_kc|) with u = 2^-24; r + 3 covers the higher orders.  bf16: that, plus the one rounding of the result to bf16."""
    assert A.shape[0] == r and B.shape[1] == r
    mag = W.double().abs() + abs(scale) * (B.double().abs() @ A.double().abs())
    bound = (r + 3) * 2.0 ** -24 * mag
    if dtype == torch.bfloat16:
        bound = bound + bf16_half_ulp(merge_ref64(W, A, B, scale))
    else:
        assert dtype == torch.float32
    return bound


def pair(W, r, seed, rel, scale):
    """fp32 A [r, in], B [out, r] with rms(scale B A) = rel rms(W)."""
    out_f, in_f = W.shape
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(r, in_f, generator=g) / math.sqrt(in_f)
    B = torch.randn(out_f, r, generator=g)
    B = B * (rel * rms(W) / rms(scale * (B.double() @ A.double())))
    return A.contiguous(), B.float().contiguous()


def adapter(cfg, targets, layers, r, seed, rel, weights, scale=ALPHA / R):
    """{weight name: (A, B)} for `targets` on `layers` of the decoder whose (stored) matrices are `weights`; rel a number or {target: number}."""
    out = {}
    for i in layers:
        assert 0 <= i < cfg['num_hidden_layers']
        for t in targets:
            name = weight_name(i, t)
            out[name] = pair(weights[name], r, seed * 1000 + i * 16 + TARGETS.index(t), rel[t] if isinstance(rel, dict) else rel, scale)
    return out


# ---- merges read back bit for bit -----------------------------------------------------------------------------------------------------------
# per tensor a list of (r, scale, seed): merged in that order.  rel = 1 throughout: a wrong index, a missing scale or a transposed A moves every element by
# many ulps.  Golden A: V = 512, H = 64 (32768 = 128 blocks; the heads' 2 x 64 = half a block).  Golden B: V = 320, H = 128 (a multiple of 256, in_f != 64).
KERNEL_CASES = [
    dict(id='A-r1', tag='A', merges={EMBED: [(1, 2.0, 11)]}),
    dict(id='A-r4', tag='A', merges={EMBED: [(4, 0.5, 12)]}),
    dict(id='A-r16-heads', tag='A', merges={EMBED: [(16, -1.0, 13)], INF: [(16, 2.0, 14)], REL: [(16, 0.5, 15)]}),
    dict(id='A-r64', tag='A', merges={EMBED: [(64, 2.0, 16)]}),
    dict(id='B-r16-heads', tag='B', merges={EMBED: [(16, 0.5, 17)], INF: [(16, -1.0, 18)], REL: [(16, 2.0, 19)]}),
    dict(id='A-sum', tag='A', merges={EMBED: [(16, 2.0, 20), (4, -1.0, 21)], INF: [(16, 0.5, 22), (1, 2.0, 23)]}),
]
KERNEL_REL = 1.0


def golden(tag):
    from conftest import load_golden_weights
    return load_golden_weights(tag)


@functools.lru_cache(maxsize=None)
def kernel_reference(case_id, dtype):
    """{name: (stored base, [(A, B, scale, r)], float64 result, bound)} of one KERNEL_CASES entry on a context of `dtype`.  A second merge lands on what the first
    one stored: the fp32 bounds add (the second evaluated on the exact intermediate, the difference is second order) and a bf16 context rounds once per merge."""
    case = next(c for c in KERNEL_CASES if c['id'] == case_id)
    _, w = golden(case['tag'])
    out = {}
    for name, merges in case['merges'].items():
        base = w[name].to(dtype)
        cur, bound, pairs = base.double(), torch.zeros(base.shape, dtype=torch.float64), []
        for n, (r, scale, seed) in enumerate(merges):
            A, B = pair(base, r, seed, KERNEL_REL, scale)
            bound = bound + merge_bound(cur, A, B, scale, r, torch.float32)
            cur = merge_ref64(cur, A, B, scale)
            if dtype == torch.bfloat16:
                # the first merge: merge_bound's half ulp of the exact result.  A later merge rounds a value that is already `bound` away from the exact one and may sit in
                # the next binade: half an ulp of the largest magnitude it can have
                bound = bound + bf16_half_ulp(cur if n == 0 else cur.abs() + bound)
            pairs.append((A, B, scale, r))
        out[name] = (base, pairs, cur, bound)
    return out


# ---- conversions ----------------------------------------------------------------------------------------------------------------------------
def _bits32(patterns):
    return torch.tensor([p - (1 << 32) if p >= (1 << 31) else p for p in patterns], dtype=torch.int32).view(torch.float32)


def _bits16(patterns):
    return torch.tensor([p - (1 << 16) if p >= (1 << 15) else p for p in patterns], dtype=torch.int16).view(torch.bfloat16)


def convert_values_f32(n, seed=5):
    """n fp32 values: the named edges first, seeded random bit patterns (every exponent, NaNs included) and ordinary normals behind them."""
    edge = [0x00000000, 0x80000000,                                   # +-0
            0x3F800000, 0xBF800000, 0x3F808000, 0x3F818000,           # 1, -1; ties: 1 + 2^-8 -> down to even (0x3F80), 1 + 3 2^-8 -> up to even (0x3F82)
            0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001,           # the same ties negative; just below / above a tie
            0x3F80FFFF, 0x3FFFFFFF,                                   # round up, with a carry into the exponent
            0x00010000, 0x80010000, 0x00008000, 0x00018000,           # bf16-subnormal results: 2^-133 exactly; the tie below it (-> 0); 1.5 x 2^-133 (tie -> 2^-132)
            0x00008001, 0x00007FFF, 0x00000001, 0x007FFFFF,           # just above / below half the smallest subnormal; smallest and largest fp32 subnormal
            0x007F8000, 0x00800000, 0x807F8000,                       # the tie that rounds into the smallest normal; the smallest normal
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,           # largest finite fp32 -> bf16 inf; the tie -> inf; just below it -> largest finite bf16
            0x7F800000, 0xFF800000,                                   # +-inf
            0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0x7F80FFFF, 0xFF800100]      # NaNs: quiet, and signalling ones whose payload sits below bf16's mantissa
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randint(-2 ** 31, 2 ** 31, (n // 2,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    nor = torch.randn(n - n // 2 - len(edge), generator=g) * 0.5
    return torch.cat([_bits32(edge), rnd, nor])


def convert_values_bf16(n, seed=6):
    edge = [0x0000, 0x8000, 0x3F80, 0xBF80, 0x0001, 0x8001, 0x007F, 0x0080, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0x7FBF, 0xFFA5]
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randint(-2 ** 15, 2 ** 15, (n - len(edge),), generator=g, dtype=torch.int64).to(torch.int16).view(torch.bfloat16)
    return torch.cat([_bits16(edge), rnd])


def convert_values_f16(n, seed=7):
    """fp16 patterns: subnormals (bf16 keeps their exponent but not their mantissa), the largest finite value, +-inf, NaN, random patterns"""
    edge = [0x0000, 0x8000, 0x3C00, 0x0001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x7C01, 0x3C08, 0x3C18, 0x3C07, 0x3C09]
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randint(-2 ** 15, 2 ** 15, (n - len(edge),), generator=g, dtype=torch.int64).to(torch.int16)
    return torch.cat([torch.tensor([p - (1 << 16) if p >= (1 << 15) else p for p in edge], dtype=torch.int16), rnd]).view(torch.float16)


def convert_values_f64(n, seed=8):
    """float64 values whose rounding to fp32 matters before the model dtype's: beyond fp32's range, below its subnormals, double-rounding ties, and the fp32 set widened"""
    edge = torch.tensor([0.0, -0.0, 1e39, -1e39, 3.4028235677973366e38, 1e-46, -1e-46, 1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8 - 2.0 ** -40,
                         1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, float('inf'), float('-inf'), float('nan')], dtype=torch.float64)
    g = torch.Generator().manual_seed(seed)
    nor = torch.randn(n - len(edge) - n // 2, generator=g, dtype=torch.float64) * 0.5
    return torch.cat([edge, convert_values_f32(n // 2, seed).double(), nor])


CONVERT_SOURCES = {torch.float32: convert_values_f32, torch.bfloat16: convert_values_bf16, torch.float16: convert_values_f16, torch.float64: convert_values_f64}


def same_bits_or_both_nan(got, want):
    """Integer bit patterns equal, NaNs compared as 'is NaN' -> the number of elements that differ"""
    assert got.dtype == want.dtype and got.shape == want.shape
    iv = torch.int32 if got.dtype == torch.float32 else torch.int16
    nan = torch.isnan(want)
    bad = torch.where(nan, ~torch.isnan(got), got.view(iv) != want.view(iv))
    return int(bad.sum())


# ---- every target through the finalized model -----------------------------------------------------------------------------------------------
def _tols():
    from test_gpu_model import F32_TOL, BF16_TOL
    return F32_TOL, BF16_TOL


def fp8_cfg():
    from test_gpu_fp8 import CFG
    return dict(CFG)


def mode_spec(mode):
    """context dtype, the oracle's dtype, and the bound of the same comparison without an adapter: (head logits, lm logits, visual_embed relative to max(1, |ref|)).
    f32 / bf16: tests/test_gpu_model.py (test_llm_step_sequence_fp32, test_bf16_model_tracks_bf16_oracle: heads BF16_TOL, lm logits 2 BF16_TOL);
    fp8: tests/test_gpu_fp8.py::test_fp8_model_matches_oracle_on_dequantised_weights (6e-2 on all three; its tower is the bf16 build's)."""
    F32_TOL, BF16_TOL = _tols()
    return {'f32': dict(cfg='A', dtype=torch.float32, oracle=torch.float32, head_tol=F32_TOL, lm_tol=F32_TOL, ve_tol=F32_TOL),
            'bf16': dict(cfg='A', dtype=torch.bfloat16, oracle=torch.bfloat16, head_tol=BF16_TOL, lm_tol=2 * BF16_TOL, ve_tol=BF16_TOL),
            'fp8': dict(cfg='fp8', dtype=torch.bfloat16, oracle=torch.float32, head_tol=6e-2, lm_tol=6e-2, ve_tol=BF16_TOL)}[mode]


MODES = ('f32', 'bf16', 'fp8')

# rel per target: chosen on the CPU so that the oracle on merged weights and the oracle on the base weights differ by at least 10 x the tolerance in one compared
# output, for every mode the case runs in (tests/test_lora_host.py asserts it).  The adapter of a real run is far smaller; these are sized to be seen.
ONE_TARGET_REL = {'q_proj': 8.0, 'k_proj': 8.0, 'v_proj': 2.0, 'o_proj': 2.0, 'gate_proj': 4.0, 'up_proj': 2.0, 'down_proj': 2.0}
LAST_LAYER_REL = {'k_proj': 16.0, 'gate_proj': 4.0}
FULL_REL = 0.5

# excess: where a case needs more than its mode's bound, the measured excess of the reference against itself (oracle in the mode's dtype against the oracle in float64 on
# the same merged weights), which the test allows twice over; None = the plain bound holds.
# Measured on the CPU: q_proj / k_proj at rel = 8 make the attention logits large, and bf16 execution of the H = 128 model then differs from float64 execution on the same
# (merged, dequantised) weights by more than the 6e-2 the fp32 oracle is compared with -- max |oracle in bf16 - oracle in float64| over the three steps.
ONE_TARGET_EXCESS = {'q_proj': {'fp8': {'lm': 0.064, 'inf': 0.081, 'rel': 0.047}},
                     'k_proj': {'fp8': {'lm': 0.0569, 'inf': 0.039, 'rel': 0.0305}}}
MODEL_CASES = (
    [dict(id='full', targets=TARGETS, layers='all', rel=FULL_REL, saved=False, modes=MODES, seed=1, excess={})] +
    [dict(id=t, targets=(t,), layers='all', rel=ONE_TARGET_REL[t], saved=False, modes=MODES, seed=2 + i, excess=ONE_TARGET_EXCESS.get(t, {})) for i, t in enumerate(TARGETS)] +
    [dict(id=f'{t}-last', targets=(t,), layers='last', rel=LAST_LAYER_REL[t], saved=False, modes=('bf16',), seed=20 + i, excess={}) for i, t in enumerate(LAST_LAYER_REL)] +
    [dict(id='saved+q_proj', targets=('q_proj',), layers='all', rel=ONE_TARGET_REL['q_proj'], saved=True, modes=MODES, seed=30, excess={})])
ONE_TARGET_IDS = [c['id'] for c in MODEL_CASES if len(c['targets']) == 1 and not c['saved']]


def model_case(case_id):
    return next(c for c in MODEL_CASES if c['id'] == case_id)


@functools.lru_cache(maxsize=None)
def base_weights(mode):
    """(config dict, weights as the context stores them) of a mode"""
    spec = mode_spec(mode)
    if spec['cfg'] == 'fp8':
        cfgd = fp8_cfg()
        return cfgd, O.random_weights(O.OracleConfig(**cfgd), seed=5, dtype=torch.bfloat16, scale='unit')
    cfgd, w = golden(spec['cfg'])
    return cfgd, {k: v.to(spec['dtype']) for k, v in w.items()}


STEP_SCALE = 0.125          # small against what the layers add to the residual stream, as a real embedding is: a change in one layer's matrix then shows at the outputs


def steps(cfgd, dtype, seed=1):
    """a 23-row chunk, a 4-row chunk and a 1-row decode: the skinny, stream and GEMV weight layouts"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(1, n, cfgd['hidden_size'], generator=g) * STEP_SCALE).to(dtype) for n in (23, 4, 1)]


def pixels(cfgd):
    """the golden pixel_values of config A (both tiny towers take 56 x 56 frames)"""
    from conftest import load_npz
    px = torch.from_numpy(load_npz('cfgA_ops.npz')['pixel_values'])
    assert px.shape[-1] == cfgd['vit_image_size']
    return px


def case_adapter(mode, case_id):
    """-> ({weight name: (A, B)}, {saved name: tensor})"""
    case = model_case(case_id)
    cfgd, w = base_weights(mode)
    L = cfgd['num_hidden_layers']
    ad = adapter(cfgd, case['targets'], range(L) if case['layers'] == 'all' else [L - 1], R, case['seed'], case['rel'], w)
    saved = {}
    if case['saved']:
        g = torch.Generator().manual_seed(case['seed'] + 500)
        for name in PROJECTOR + (INF, REL):
            saved[name] = (torch.randn(w[name].shape, generator=g) * max(rms(w[name]), 0.05)).to(w[name].dtype)
    return ad, saved


def merged_weights(mode, case_id):
    """the base weights with the adapter merged in float64 and cast the way the context stores them, saved modules replaced"""
    _, w = base_weights(mode)
    ad, saved = case_adapter(mode, case_id)
    out = dict(w)
    for name, (A, B) in ad.items():
        out[name] = merge_ref64(w[name], A, B, ALPHA / R).to(w[name].dtype)
    out.update(saved)
    return out


def oracle_on(mode, weights, dtype=None):
    """the mode's reference model on `weights` (as stored): fp8 dequantises what the quantiser makes of every decoder matrix"""
    spec = mode_spec(mode)
    cfgd, _ = base_weights(mode)
    dtype = dtype or spec['oracle']
    w = dict(weights)
    if mode == 'fp8':
        from rawops import quantize_ref
        for k, v in weights.items():
            if k.startswith('model.layers.') and k.endswith('.weight') and any(f'.{t}.' in k for t in TARGETS):
                q, s = quantize_ref(v)
                w[k] = q.float() * s[:, None]
    return O.OracleModel(O.OracleConfig(**cfgd), {k: v.to(dtype) for k, v in w.items()})


def run_steps(model, xs, device=None):
    """[{'lm': logits[0, -1], 'inf': informative_logits[0], 'rel': relevance_logits[0]}] per step, fp32 on the CPU"""
    cache, out = None, []
    for x in xs:
        o = model(inputs_embeds=x.to(device) if device is not None else x, past_key_values=cache)
        cache = o.past_key_values
        out.append({'lm': o.logits[0, -1].float().cpu(), 'inf': o.informative_logits[0].float().cpu(), 'rel': o.relevance_logits[0].float().cpu()})
    return out


@functools.lru_cache(maxsize=None)
def reference_outputs(mode, case_id):
    """the oracle's step outputs on the merged weights (case_id None: on the base weights), computed once"""
    cfgd, w = base_weights(mode)
    spec = mode_spec(mode)
    om = oracle_on(mode, merged_weights(mode, case_id) if case_id else w)
    return run_steps(om, [x.to(spec['oracle']) for x in steps(cfgd, spec['dtype'])])


def worst(got, want):
    """{'lm' | 'inf' | 'rel': max |got - want| over the steps}"""
    return {k: max((g[k] - r[k]).abs().max().item() for g, r in zip(got, want)) for k in ('lm', 'inf', 'rel')}


def tol_of(mode, key):
    spec = mode_spec(mode)
    return spec['lm_tol'] if key == 'lm' else spec['head_tol']


def write_adapter(path, ad, saved=None, originals=None, r=R, alpha=ALPHA):
    """A PEFT adapter directory: lora_A / lora_B under `base_model.model.<module>.lora_X.default.weight`, saved modules under
    `<module>.modules_to_save.default.<rest>` beside the `<module>.original_module.<rest>` copy PEFT keeps of the tensor they replace."""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    t = {}
    for name, (A, B) in ad.items():
        mod = name[:-len('.weight')]
        t[f'base_model.model.{mod}.lora_A.default.weight'] = A.contiguous()
        t[f'base_model.model.{mod}.lora_B.default.weight'] = B.contiguous()
    for name, v in (saved or {}).items():
        mod, rest = ('model.mm_projector', name[len('model.mm_projector.'):]) if name.startswith('model.mm_projector.') else name.rsplit('.', 1)
        t[f'base_model.model.{mod}.modules_to_save.default.{rest}'] = v.contiguous()
        if originals is not None:
            t[f'base_model.model.{mod}.original_module.{rest}'] = originals[name].contiguous()
    save_file(t, os.path.join(path, 'adapter_model.safetensors'))
    with open(os.path.join(path, 'adapter_config.json'), 'w') as f:
        json.dump({'r': r, 'lora_alpha': alpha, 'peft_type': 'LORA', 'target_modules': sorted({n.split('.')[-2] for n in ad})}, f)
    return path
