"""mmd_kv_drop_shift once at the 7B arena geometry (28 layers x 4 kv heads = 112 rows, head_dim 128, bf16), with the length and span of
tests/test_gpu_kv_drop_trueshape.py: 3 000 tokens, 1 000 dropped behind a 20-token sink.  Random canonical K / V go into two fresh streams; V of the shifted drop equals
V of the plain drop in every row, and a sample of rows is held against the host statement (tests/kv_shift_oracle.py) as tests/test_gpu_kv_shift.py holds the small arenas.
The model is the weightless 28-layer one of tools/kv_drop_bench.py: only its arena is used."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import kv_shift_oracle as S
from test_gpu_kv_drop import snapshot, up64
from test_gpu_kv_drop_trueshape import PREFIX, SINK, DROP
from mmduet_amd._lib import lib

BF = torch.bfloat16
SAMPLE = [(0, 0), (0, 3), (13, 1), (27, 0), (27, 3)]          # (layer, kv head): the first and last row and some between


def test_shifted_drop_at_the_7b_arena():
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM, KVSnapshot
    cfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=28, intermediate_size=256, vit_num_hidden_layers=2, vit_layers_removed=1,
                                       frame_num_tokens=49, frame_resolution=384, v_placeholder='<image>')
    m = VideoHeadLiveLlavaQwenForCausalLM(cfg, torch_dtype=BF, max_vit_batch=1, max_step_tokens=256, kv_initial_tokens=4096)
    c = m.config
    layers, nkv, d = c.num_hidden_layers, c.num_key_value_heads, c.head_dim
    assert (layers, nkv, d) == (28, 4, 128)
    g = torch.Generator().manual_seed(5)
    K0 = torch.randn(layers, nkv, PREFIX, d, generator=g).to(BF)
    V0 = (torch.randn(layers, nkv, PREFIX, d, generator=g) * 0.5).to(BF)

    def load():
        return m.kv_load(KVSnapshot(K0, V0, PREFIX, BF, layers, nkv, d, m._rope_inv_freq))
    a, b = m.kv_drop(load(), SINK, SINK + DROP), m.kv_drop(load(), SINK, SINK + DROP, shift=True)
    n1 = PREFIX - DROP
    assert len(a) == len(b) == n1 and m.kv_position(a) == PREFIX and m.kv_position(b) == n1 == int(lib().mmd_kv_position(b.arena.h))
    sa, sb = m.kv_save(a, pin=False), m.kv_save(b, pin=False)
    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(sa.V), bits(sb.V))          # V: the plain drop's bytes, every row
    assert torch.equal(bits(sb.V), bits(torch.cat([V0[:, :, :SINK], V0[:, :, SINK + DROP:]], 2)))
    assert torch.equal(bits(sb.K[:, :, :SINK]), bits(K0[:, :, :SINK]))          # the sink's keys: not written
    assert torch.equal(bits(sa.K), bits(torch.cat([K0[:, :, :SINK], K0[:, :, SINK + DROP:]], 2)))
    Ks, Vs = snapshot(m, b, up64(n1))          # every arena slot up to the end of the last V block is finite
    assert bool(torch.isfinite(Ks.float()).all()) and bool(torch.isfinite(Vs.float()).all())
    inv = m._rope_inv_freq.detach().cpu().float().numpy()
    worst = 0.0
    for layer, head in SAMPLE:
        k0 = K0[layer, head].float().numpy().astype(np.float64)
        exact, _ = S.drop_shift(k0, k0, SINK, SINK + DROP, inv)
        got = sb.K[layer, head].float().numpy().astype(np.float64)
        err = np.abs(got - exact)[SINK:]
        bnd = S.bound(exact[SINK:], S.pair_norm(k0[SINK + DROP:]), 'bf16')
        worst = max(worst, float((err / bnd).max()))
        assert (err <= bnd).all(), (layer, head, int((err > bnd).sum()))
    print(f'worst |got - exact| / bound over {len(SAMPLE)} rows: {worst:.3g}')
