"""The case table of tests/test_model_plan_host.py: configurations as mmd_create receives them (the fields of mmd_config, include/mmduet.h), the bad configurations with the
message each is refused with, and the names finalize documents as dropped.  No GPU, no torch: the golden configurations are read from the npz files with numpy."""
import json
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
F32, BF16 = 0, 1
W_DTYPE, W_FP8 = 0, 1
POOL_BILINEAR, POOL_ADAPTIVE_AVG = 0, 3
MMD_OK, MMD_EINVAL, MMD_ENOENT = 0, -22, -2
STEP_STATE_BYTES = 48          # sizeof(StepState), csrc/common.h: 2 x int64, 2 pointers, 2 x int32, int64

FIELDS = ('dtype', 'vocab_size', 'hidden_size', 'intermediate_size', 'num_layers', 'num_heads', 'num_kv_heads', 'head_dim', 'rope_theta', 'rms_norm_eps', 'vit_hidden',
          'vit_intermediate', 'vit_layers', 'vit_heads', 'vit_image', 'vit_patch', 'vit_ln_eps', 'vit_post_layernorm', 'pool_mode', 'pool_stride', 'frame_num_tokens',
          'max_vit_batch', 'max_step_tokens', 'weight_dtype', 'vision_only', 'vit_class_token', 'vit_pre_layernorm', 'vit_act', 'vit_pool_head', 'tower_f16')


def decoder(dtype=BF16, vocab=152064, H=3584, I=18944, layers=28, heads=28, kv=4, C=1152, CI=4304, vit_layers=26, vit_heads=16, image=384, patch=14, stride=4,
            max_vit_batch=35, max_step_tokens=1024, **over):
    """a LLaVA model as modeling_live.py fills mmd_config (defaults: the true-shape 7B with the so400m tower)"""
    side = -(-(image // patch) // stride)
    c = dict(dtype=dtype, vocab_size=vocab, hidden_size=H, intermediate_size=I, num_layers=layers, num_heads=heads, num_kv_heads=kv, head_dim=H // heads, rope_theta=1e6,
             rms_norm_eps=1e-6, vit_hidden=C, vit_intermediate=CI, vit_layers=vit_layers, vit_heads=vit_heads, vit_image=image, vit_patch=patch, vit_ln_eps=1e-6,
             vit_post_layernorm=0, pool_mode=POOL_BILINEAR, pool_stride=stride, frame_num_tokens=side * side, max_vit_batch=max_vit_batch, max_step_tokens=max_step_tokens,
             weight_dtype=W_DTYPE, vision_only=0, vit_class_token=0, vit_pre_layernorm=0, vit_act=0, vit_pool_head=0, tower_f16=0)
    assert set(over) <= set(c), set(over) - set(c)
    c.update(over)
    return c


def encoder(kind, dtype=BF16, C=1024, CI=4096, layers=24, heads=16, image=384, patch=16, pooled=7, cls=False, max_batch=32):
    """a vision-only context as vision_live.py fills mmd_config: 'siglip' (post_layernorm, the pooling head when cls) | 'clip' (class token, pre_layrnorm, quick_gelu)"""
    return decoder(dtype=dtype, vocab=0, H=C, I=0, layers=0, heads=1, kv=1, C=C, CI=CI, vit_layers=layers, vit_heads=heads, image=image, patch=patch, stride=pooled,
                   max_vit_batch=max_batch, max_step_tokens=1, head_dim=2, rope_theta=1e4, vision_only=1, pool_mode=POOL_ADAPTIVE_AVG, frame_num_tokens=1,
                   vit_post_layernorm=int(kind == 'siglip'), vit_class_token=int(kind == 'clip'), vit_pre_layernorm=int(kind == 'clip'), vit_act=int(kind == 'clip'),
                   vit_pool_head=int(kind == 'siglip' and cls))


def golden(tag):
    """(configuration dict, {checkpoint name: elements}) of tests/golden/cfg{tag}_weights.npz"""
    with np.load(os.path.join(GOLDEN, f'cfg{tag}_weights.npz')) as z:
        cfg = json.loads(bytes(z['__config__']).decode())
        return cfg, {k: int(z[k].size) for k in z.files if k != '__config__'}


def golden_config(tag, dtype=BF16, **over):
    """tests/helpers.py hip_model(tag): max_vit_batch = 8, max_step_tokens = 512"""
    g = golden(tag)[0]
    return decoder(dtype=dtype, vocab=g['vocab_size'], H=g['hidden_size'], I=g['intermediate_size'], layers=g['num_hidden_layers'], heads=g['num_attention_heads'],
                   kv=g['num_key_value_heads'], C=g['vit_hidden_size'], CI=g['vit_intermediate_size'], vit_layers=g['vit_layers'], vit_heads=g['vit_heads'], image=g['vit_image_size'],
                   patch=g['vit_patch_size'], stride=g['video_pooling_stride'], max_vit_batch=8, max_step_tokens=512, rope_theta=g['rope_theta'], rms_norm_eps=g['rms_norm_eps'], **over)


# the 2 + 2 layer model of tests/model_plan_record.py (SYNTH)
def small(image, **over):
    return decoder(vocab=320, H=128, I=192, layers=2, heads=4, kv=1, C=64, CI=96, vit_layers=2, vit_heads=4, image=image, stride=2, max_vit_batch=8, max_step_tokens=512, **over)


CASES = {
    'cfgA': golden_config('A'),
    'cfgB': golden_config('B'),
    'cfgA_f32': golden_config('A', dtype=F32),
    'cfgB_f32': golden_config('B', dtype=F32),
    'cfgB_fp8': golden_config('B', weight_dtype=W_FP8),
    'true_7b': decoder(tower_f16=1),          # what the product builds: bf16, the autocast tower
    'true_7b_tower_f16_0': decoder(tower_f16=0),
    'true_7b_tower_f16_2': decoder(tower_f16=2),
    'true_7b_fp8': decoder(tower_f16=1, weight_dtype=W_FP8),
    'true_7b_f32': decoder(dtype=F32),
    'true_7b_post_ln': decoder(vit_post_layernorm=1, tower_f16=2),
    'true_7b_multi_stream': decoder(tower_f16=1, max_step_tokens=4096),
    'clip': encoder('clip', image=336, patch=14, cls=True),
    'clip_f32': encoder('clip', dtype=F32, image=224, patch=14),
    'pool_head': encoder('siglip', cls=True),
    'vision_only': encoder('siglip'),
    'small_tower_f16_0': small(126),
    'small_tower_f16_1': small(126, tower_f16=1),
    'small_tower_f16_2': small(126, tower_f16=2),
    'small_tower_384': small(384, tower_f16=1),
}

# ---- configurations mmd_create refuses: (name, base case, overrides, message) in the order of the checks; ACCEPTED: the valid neighbours ----------------------------------
TOWER_FORM = 'tower_f16 needs a bf16 context and the LLaVA SigLIP tower form (no class token / pre-LN / pooling head, hidden % 64 == 0, head_dim % 8 == 0)'
TOWER_RANGE = 'tower_f16: 0 | 1 (autocast: fp32 residual stream; no post_layernorm, hidden <= 2048) | 2 (fp16 residual stream)'
REFUSED = [
    ('struct_size', 'true_7b', dict(struct_size=-4), 'mmd_config size mismatch (ABI)'),          # struct_size: added to the true size
    ('dtype_2', 'true_7b', dict(dtype=2), 'unsupported dtype'),
    ('dtype_negative', 'cfgA', dict(dtype=-1), 'unsupported dtype'),
    ('fp8_in_f32', 'true_7b_f32', dict(weight_dtype=W_FP8), 'weight_dtype fp8_e4m3 needs a bf16 context'),
    ('weight_dtype_2', 'true_7b', dict(weight_dtype=2), 'weight_dtype fp8_e4m3 needs a bf16 context'),
    ('heads_not_grouped', 'true_7b', dict(num_kv_heads=5), 'unsupported head configuration'),
    ('head_dim_odd', 'true_7b', dict(head_dim=127), 'unsupported head configuration'),
    ('head_dim_130', 'true_7b', dict(head_dim=130), 'unsupported head configuration'),
    ('vit_heads_7', 'true_7b', dict(vit_heads=7), 'unsupported ViT head configuration'),
    ('vit_head_dim_144', 'true_7b', dict(vit_heads=8), 'unsupported ViT head configuration'),
    ('tower_f16_in_f32', 'true_7b_f32', dict(tower_f16=1), TOWER_FORM),
    ('tower_f16_vision_only', 'vision_only', dict(tower_f16=2, vit_post_layernorm=0), TOWER_FORM),
    ('tower_f16_class_token', 'true_7b', dict(vit_class_token=1), TOWER_FORM),
    ('tower_f16_pre_ln', 'true_7b', dict(vit_pre_layernorm=1), TOWER_FORM),
    ('tower_f16_quick_gelu', 'true_7b', dict(vit_act=1), TOWER_FORM),
    ('tower_f16_pool_head', 'true_7b', dict(vit_pool_head=1), TOWER_FORM),
    ('tower_f16_hidden_1120', 'true_7b', dict(vit_hidden=1120, vit_heads=14), TOWER_FORM),
    ('tower_f16_head_dim_36', 'true_7b', dict(vit_heads=32), TOWER_FORM),
    ('tower_f16_negative', 'true_7b', dict(tower_f16=-1), TOWER_RANGE),
    ('tower_f16_3', 'true_7b', dict(tower_f16=3), TOWER_RANGE),
    ('tower_f16_1_post_ln', 'true_7b', dict(vit_post_layernorm=1), TOWER_RANGE),
    ('tower_f16_1_hidden_2112', 'true_7b', dict(vit_hidden=2112, vit_heads=22), TOWER_RANGE),
    # the first failing check wins
    ('dtype_before_heads', 'true_7b', dict(dtype=2, num_kv_heads=5), 'unsupported dtype'),
    ('heads_before_vit_heads', 'true_7b', dict(head_dim=127, vit_heads=7), 'unsupported head configuration'),
    ('form_before_range', 'true_7b', dict(tower_f16=3, vit_act=1), TOWER_FORM),
]
ACCEPTED = [
    ('fp8_in_bf16', 'true_7b', dict(weight_dtype=W_FP8)),
    ('head_dim_128', 'true_7b', dict(head_dim=128)),
    ('head_dim_126', 'true_7b', dict(head_dim=126)),
    ('bad_heads_without_a_decoder', 'vision_only', dict(num_heads=3, num_kv_heads=2, head_dim=131)),
    ('vit_head_dim_128', 'true_7b', dict(vit_heads=9)),
    ('tower_f16_0_in_f32', 'true_7b_f32', dict(tower_f16=0)),
    ('class_token_without_tower_f16', 'true_7b_tower_f16_0', dict(vit_class_token=1, vit_pre_layernorm=1, vit_act=1, vit_pool_head=1)),
    ('hidden_1120_without_tower_f16', 'true_7b_tower_f16_0', dict(vit_hidden=1120, vit_heads=14)),
    ('head_dim_36_without_tower_f16', 'true_7b_tower_f16_0', dict(vit_heads=32)),
    ('tower_f16_2_post_ln', 'true_7b', dict(tower_f16=2, vit_post_layernorm=1)),
    ('tower_f16_2_hidden_2112', 'true_7b', dict(tower_f16=2, vit_hidden=2112, vit_heads=22)),
    ('tower_f16_1_hidden_2048', 'true_7b', dict(vit_hidden=2048)),
]

# ---- what finalize drops (model_plan.h, above weight_plan): loaded names the plan of a LLaVA context does not consume ---------------------------------------------------
DROPPED = (r'vit\.post_layernorm\.(weight|bias)$',          # without vit_post_layernorm
           r'vit\.head\.',                                   # without vit_pool_head
           r'vit\.encoder\.layers\.(\d+)\.',                 # layers beyond vit_layers (LLaVA removes the last): checked against the layer number below
           r'vision_encoder\.')                              # another module of the checkpoint


def dropped(name, cfg):
    for pat in DROPPED:
        m = re.match(pat, name)
        if m:
            return int(m.group(1)) >= cfg['vit_layers'] if pat.startswith(r'vit\.encoder') else True
    return False
