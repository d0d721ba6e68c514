"""What a context computes from its weights, as SHA-256 of raw output bytes: the recorder behind tests/golden/model_plan_parent.json and tests/test_gpu_model_plan.py.

The fixture was recorded before csrc/model_plan.h existed; mmd_finalize_weights only moves bytes, so a context built through the plan must reproduce every hash.
    python tests/model_plan_record.py OUT.json        records every case of GPU_CASES
Weights are the golden ones (cfgA / cfgB, tests/golden/vision_live.npz) or synthetic_weights(seed=3, scale='unit') generated on the host, as helpers._build seeds them;
inputs come from a host torch.Generator seeded per case."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

FRAMES, CHUNK_ROWS, PROMPT_ROWS, NEW_TOKENS, SEED = 3, 40, 7, 8, 3
DECODER_ENTRIES = ('tower_features', 'visual_embed', 'hidden', 'lm_head', 'video_heads', 'generate', 'weight_bytes')
VISION_ENTRIES = ('encode', 'weight_bytes')

# the 2 + 2 layer model the golden ones cannot express: a tower the half kernels accept (hidden % 64 == 0, head_dim % 8 == 0, >= 65 tokens per frame)
SYNTH = dict(vocab_size=320, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=1, vit_hidden_size=64,
             vit_intermediate_size=96, vit_num_hidden_layers=3, vit_layers_removed=1, vit_num_attention_heads=4, vit_patch_size=14, video_pooling_stride=2)

# name -> how the context is built.  golden: tag of tests/golden/cfg{tag}_weights.npz; synth: vit_image_size of SYNTH; vision: kind of tests/golden/vision_live.npz
GPU_CASES = {
    'cfgA_bf16': dict(golden='A', dtype='bf16'),
    'cfgB_bf16': dict(golden='B', dtype='bf16'),
    'cfgA_f32': dict(golden='A', dtype='f32'),
    'cfgB_fp8': dict(golden='B', dtype='bf16', weight_dtype='fp8_e4m3'),
    'tower_f16_0': dict(synth=126, dtype='bf16', tower_dtype='bf16'),
    'tower_f16_1': dict(synth=126, dtype='bf16', tower_dtype='fp16'),
    'tower_f16_2': dict(synth=126, dtype='bf16', tower_dtype='fp16_resid16'),
    'tower_384': dict(synth=384, dtype='bf16'),
    'clip': dict(vision='clip', dtype='bf16', cls=True),
    'pool_head': dict(vision='siglip', dtype='bf16', cls=True),
    'vision_only': dict(vision='siglip', dtype='f32', cls=False),
}
DTYPES = {'bf16': torch.bfloat16, 'f32': torch.float32}


def sha(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous()
        t = t.view(torch.int16).numpy() if t.dtype == torch.bfloat16 else t.numpy()
    return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()


def _vision_fixture(kind):
    from conftest import load_npz
    z = load_npz('vision_live.npz')
    cfg = json.loads(bytes(z['__config__']).decode())[kind]
    w = {k[len(kind) + 3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith(kind + '.w.')}
    return cfg, w, torch.from_numpy(z[kind + '.frames'])


def weights_of(case):
    """(product config or vision config, ordered [(name, tensor)]) of a case, on the host"""
    spec = GPU_CASES[case]
    if 'vision' in spec:
        cfg, w, _ = _vision_fixture(spec['vision'])
        return cfg, list(w.items())
    if 'golden' in spec:
        from conftest import load_golden_weights
        from helpers import product_config
        cfgd, w = load_golden_weights(spec['golden'])
        pcfg = product_config(cfgd)
        named = list(w.items())
    else:
        from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
        from mmduet_amd.weights import synthetic_weights
        side = -(-(spec['synth'] // SYNTH['vit_patch_size']) // SYNTH['video_pooling_stride'])
        pcfg = VideoHeadLiveLlavaQwenConfig(**SYNTH, vit_image_size=spec['synth'], frame_resolution=spec['synth'], frame_num_tokens=side * side, v_placeholder='<image>')
        named = list(synthetic_weights(pcfg, seed=SEED, device='cpu', dtype=DTYPES[spec['dtype']], scale='unit'))
    for k in ('tower_dtype', 'weight_dtype'):
        if k in spec:
            setattr(pcfg, k, spec[k])
    return pcfg, named


def create(case):
    """the context of a case with no tensor loaded: (model or encoder, [(name, tensor)] to load)"""
    spec = GPU_CASES[case]
    cfg, named = weights_of(case)
    if 'vision' in spec:
        from mmduet_amd.vision_live import LiveVisionEncoder
        return LiveVisionEncoder(spec['vision'], cfg, torch_dtype=DTYPES[spec['dtype']], frame_token_cls=spec['cls'], frame_token_pooled=(2, 2), max_batch=8), named
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    return VideoHeadLiveLlavaQwenForCausalLM(cfg, torch_dtype=DTYPES[spec['dtype']], max_vit_batch=8, max_step_tokens=512, kv_initial_tokens=512), named


def build(case):
    m, named = create(case)
    if 'vision' in GPU_CASES[case]:
        return m.load_state_dict(dict(named))
    for name, t in named:
        m.load_tensor(name, t)
    m.finalize()
    return m


def weight_bytes(m):
    from mmduet_amd._lib import lib
    return int(lib().mmd_weight_bytes(m._ctx))


def record(case, m):
    """entry -> SHA-256 of what the finalized context `m` of `case` computes"""
    spec = GPU_CASES[case]
    g = torch.Generator().manual_seed(SEED * 1000003 + sorted(GPU_CASES).index(case))
    if 'vision' in spec:
        out = {'encode': sha(m(_vision_fixture(spec['vision'])[2][:FRAMES])), 'weight_bytes': weight_bytes(m)}
        assert tuple(out) == VISION_ENTRIES
        return out
    R, H = m.config.vit_image_size, m.config.hidden_size
    frames = torch.randn(FRAMES, 3, R, R, generator=g).to(m.dtype)
    x = torch.randn(1, CHUNK_ROWS, H, generator=g).to(m.dtype)
    out = {'tower_features': sha(m.tower_features(frames)), 'visual_embed': sha(m.visual_embed(frames))}
    rows = m(inputs_embeds=x).hidden_states[0]
    out['hidden'] = sha(rows)
    out['lm_head'] = sha(m.lm_head(rows))
    out['video_heads'] = sha(m.video_heads(rows))
    ids, _ = m.greedy_generate(x[:, :PROMPT_ROWS], None, None, NEW_TOKENS)
    assert len(ids) == NEW_TOKENS
    out['generate'] = sha(np.asarray(ids, dtype=np.int64))
    out['weight_bytes'] = weight_bytes(m)
    assert tuple(out) == DECODER_ENTRIES
    return out


def record_all():
    out = {}
    for case in GPU_CASES:
        m = build(case)
        out[case] = record(case, m)
        del m
    return out


if __name__ == '__main__':
    res = record_all()
    with open(sys.argv[1], 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res, indent=1, sort_keys=True))
