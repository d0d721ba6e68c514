"""The sliding context window at the 7B head geometry (28 query heads, 4 kv heads, head_dim 128; bf16; two layers): a 3 000-token prefix, 1 000 tokens dropped
behind a 20-token sink, then a 49-row frame step and a decode row -- against the bf16 oracle composed over the sliced KV handle at the stream's true positions
(tests/kv_drop_cases.py), under the bounds tests/test_gpu_trueshape.py holds for true-width steps."""
import pytest
import torch

pytestmark = pytest.mark.gpu
import kv_drop_cases as D
from oracle import duet_oracle as O

TOL = 6e-2          # tests/test_gpu_trueshape.py: head logits under TOL, lm_head logits under 2 TOL
BF = torch.bfloat16
PREFIX, SINK, DROP = 3000, 20, 1000


def maxerr(a, b):
    return (a.float().cpu() - b.float().cpu()).abs().max().item()


def test_drop_behind_a_sink_then_frame_step_and_decode_row():
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    ocfg = O.OracleConfig(vocab_size=2048, num_hidden_layers=2, vit_layers=1)          # every other dimension is the 7B default
    assert (ocfg.num_attention_heads, ocfg.num_key_value_heads, ocfg.head_dim) == (28, 4, 128)
    w = O.random_weights(ocfg, seed=3, dtype=BF, scale='unit')
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=2, vit_num_hidden_layers=2, vit_layers_removed=1,
                                        frame_num_tokens=49, frame_resolution=384, v_placeholder='<image>')
    m = VideoHeadLiveLlavaQwenForCausalLM(pcfg, torch_dtype=BF, max_vit_batch=1, max_step_tokens=1024, kv_initial_tokens=4096)
    m.load_state_dict(w)
    g = torch.Generator().manual_seed(4)
    x0, x1, x2 = ((torch.randn(1, n, 3584, generator=g) * 0.5).to(BF) for n in (PREFIX, 49, 1))
    cache = m.kv_drop(m(inputs_embeds=x0.cuda()).past_key_values, SINK, SINK + DROP)
    assert len(cache) == PREFIX - DROP and m.kv_position(cache) == PREFIX
    _, kv = O.llm_forward(w, ocfg, x0[0], None)
    kv = D.drop_handle(kv, SINK, SINK + DROP)
    pos = PREFIX
    for x in (x1, x2):
        out = m(inputs_embeds=x.cuda(), past_key_values=cache); cache = out.past_key_values
        h, kv = D.oracle_step_at(w, ocfg, x[0], kv, pos)
        pos += x.shape[1]
        errs = (maxerr(out.informative_logits[0, -1], O.linear(h[-1:], w['informative_head.weight']).float()[0]),
                maxerr(out.relevance_logits[0, -1], O.linear(h[-1:], w['relevance_head.weight']).float()[0]),
                maxerr(out.logits[0, -1], O.linear(h[-1:], w['lm_head.weight']).float()[0]))
        print(f'S {x.shape[1]} at position {pos - x.shape[1]}: informative {errs[0]:.4g}, relevance {errs[1]:.4g}, logits {errs[2]:.4g}')
        assert errs[0] < TOL and errs[1] < TOL and errs[2] < 2 * TOL
        assert len(cache) == pos - DROP and m.kv_position(cache) == pos
