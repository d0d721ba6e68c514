"""Digests of everything the vision tower feeds, for fixed seeds: a change to the tower's host code that keeps the launches and their arguments must leave every line
unchanged.  Run it on two builds of the library and compare the outputs (profiles/r14_tower_plan.md holds the columns of the tower-plan refactor).

Per tower mode (fp32 / bf16 / fp16 / fp16_resid16) at true width (C = 1152, 729 tokens, 2 tower layers) and B = 1 and 3: visual_embed with the sparse and with the full last
layer, visual_embed_frames, tower_features, both debug taps behind a full-tower encode, connector_pool of the tower features; then the launches, bytes and FLOPs the
profiler counts per kernel class for one 3-frame encode.  The 64-wide tower at grids 12 and 16 (stride 4; the fp16 tower's sparse / full gate) at B = 1, 2, 3 in the bf16
and fp16 towers.  The secondary encoders of mmduet_amd/vision_live.py on the golden tiny towers (class-token and pooling-head forms).

    python tools/tower_bits.py [out.json]
"""
import hashlib
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch
from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
from mmduet_amd.vision_live import LiveVisionEncoder
from mmduet_amd.weights import synthetic_weights

MODES = {'fp32': (torch.float32, None), 'bf16': (torch.bfloat16, 'bf16'), 'fp16': (torch.bfloat16, 'fp16'), 'fp16_resid16': (torch.bfloat16, 'fp16_resid16')}
out = {}


def digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def build(pcfg, dtype, tower, max_vit_batch, seed):
    if tower:
        pcfg.tower_dtype = tower
    m = VideoHeadLiveLlavaQwenForCausalLM(pcfg, torch_dtype=dtype, max_vit_batch=max_vit_batch, max_step_tokens=64, kv_initial_tokens=256)
    for name, t in synthetic_weights(pcfg, seed=seed, device=m.device, dtype=dtype, scale='unit'):
        m.load_tensor(name, t)
    m.finalize()
    return m


def encode_digests(m, key, px, frames=None):
    B = px.shape[0]
    out[f'{key}/visual_embed'] = digest(m.visual_embed(px))
    if frames is not None:
        out[f'{key}/visual_embed_frames'] = digest(m.visual_embed_frames(frames))
    m.set_full_tower(True)
    out[f'{key}/visual_embed_full_tower'] = digest(m.visual_embed(px))
    out[f'{key}/tap0'] = digest(m.vit_debug_tap(0, B))
    out[f'{key}/tap1'] = digest(m.vit_debug_tap(1, B))
    m.set_full_tower(False)
    feats = m.tower_features(px)
    out[f'{key}/tower_features'] = digest(feats)
    out[f'{key}/connector_pool'] = digest(m.connector_pool(feats))


for mode, (dtype, tower) in MODES.items():
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=1, vit_num_hidden_layers=3, vit_layers_removed=1, frame_num_tokens=49, frame_resolution=384,
                                        v_placeholder='<image>')
    m = build(pcfg, dtype, tower, 4, seed=3)
    assert m.tower_dtype == mode
    g = torch.Generator().manual_seed(11)
    for B in (1, 3):
        px = torch.randn(B, 3, 384, 384, generator=g).to(dtype).cuda()
        frames = torch.randint(0, 256, (B, 3, 336, 336), generator=g, dtype=torch.uint8)
        encode_digests(m, f'true/{mode}/B{B}', px, frames)
    m.prof_reset(); m.prof_set_stride(1); m.prof_enable(True)
    m.visual_embed(px); torch.cuda.synchronize()
    m.prof_enable(False)
    out[f'true/{mode}/prof_B3'] = {k: [v['launches'], v['bytes'], v['flops']] for k, v in m.prof_read().items() if v['launches']}
    del m
    torch.cuda.empty_cache()

for grid in (12, 16):
    for mode in ('bf16', 'fp16'):
        img, po = grid * 14, -(-grid // 4)
        pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                                            vit_hidden_size=64, vit_intermediate_size=128, vit_num_hidden_layers=3, vit_layers_removed=1, vit_num_attention_heads=4,
                                            vit_image_size=img, vit_patch_size=14, video_pooling_stride=4, frame_num_tokens=po * po, frame_resolution=img, v_placeholder='<image>')
        m = build(pcfg, torch.bfloat16, MODES[mode][1], 8, seed=7)
        assert m.tower_dtype == mode
        for B in (1, 2, 3):
            px = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(grid + B)).to(torch.bfloat16).cuda()
            encode_digests(m, f'grid{grid}/{mode}/B{B}', px)
        del m
        torch.cuda.empty_cache()

# the secondary encoders on the golden tiny towers: SigLIP (post-LayerNorm, pooling head) and CLIP (class token, pre-LayerNorm, quick-GELU)
with np.load(os.path.join(R, 'tests', 'golden', 'vision_live.npz')) as z:
    z = {k: z[k] for k in z.files}
vcfg = json.loads(bytes(z['__config__']).decode())
for tag, cls, pooled in (('siglip', False, (2, 2)), ('siglip', True, None), ('siglip', True, (2, 2)), ('clip', False, (2, 2)), ('clip', True, None)):
    w = {k[len(tag) + 3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith(tag + '.w.')}
    for dtype in (torch.float32, torch.bfloat16):
        enc = LiveVisionEncoder.from_state_dict(tag, vcfg[tag], w, torch_dtype=dtype, frame_token_cls=cls, frame_token_pooled=pooled)
        out[f'vision_live/{tag}/cls{int(cls)}_pooled{pooled}/{str(dtype)[6:]}'] = digest(enc(torch.from_numpy(z[tag + '.frames']).cuda()))
        del enc

text = json.dumps(out, indent=1, sort_keys=True)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        f.write(text + '\n')
