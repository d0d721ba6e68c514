"""Log-probabilities on the captured decode step (true layer widths, two layers, vocabulary 2048, bf16: the model tests/test_gpu_trueshape.py builds for its
test_sampled_replay_* tests): the replayed step records at the index it reads from device state, recording changes no id, and the step is keyed by the setting.

Values against single-row replay calls are held to the bf16 rule of tests/test_gpu_logprobs.py: twice the largest |log_softmax| difference, at the generated ids of
THIS file's two cases, between single-row replay calls and one teacher-forced chunk call, measured on the parent commit (profiles/r08_logprobs.md).  At true width the two
routes take different GEMM and attention forms: TRUE_MEASURED = 0.015653 (greedy 0.015520, sampled 0.015652), so TOL_TRUE = 0.031306.  (The tiny model's figure is 0.0 and
could not be met by any step whose logits went through another kernel form; the rule is applied to the cases of the test at hand.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu
from oracle import duet_oracle as O
from test_gpu_logprobs import SAMPLING, check_records

TRUE_MEASURED = 0.015653
TOL_TRUE = 2 * TRUE_MEASURED


@pytest.fixture(scope='module')
def graph_model():
    """The true-width model with the captured decode step switched on (MMDUET_GRAPH is read when the native context is created)."""
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    ocfg = O.OracleConfig(vocab_size=2048, num_hidden_layers=2, vit_layers=1)
    w = O.random_weights(ocfg, seed=3, dtype=torch.bfloat16, scale='unit')
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=2, vit_num_hidden_layers=2, vit_layers_removed=1,
                                        frame_num_tokens=49, frame_resolution=384, v_placeholder='<image>')
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('MMDUET_GRAPH', '1')
        m = VideoHeadLiveLlavaQwenForCausalLM(pcfg, torch_dtype=torch.bfloat16, max_vit_batch=1, max_step_tokens=1024, kv_initial_tokens=1024)
    m.load_state_dict(w)
    return m


def _rand(g, rows):
    return (torch.randn(1, rows, 3584, generator=g) * 0.5).to(torch.bfloat16).cuda()


def replay_rows(m, ctx, prompt, ids):
    out = m(inputs_embeds=prompt, past_key_values=m(inputs_embeds=ctx).past_key_values)
    rows = []
    for tok in ids:
        rows.append(out.logits[0, -1].float().cpu())
        out = m(inputs_embeds=m.get_input_embeddings()(torch.tensor([[tok]], device=m.device)).view(1, 1, -1), past_key_values=out.past_key_values)
    return torch.stack(rows)


@pytest.mark.parametrize('do_sample', [False, True], ids=['greedy', 'sampled'])
def test_replayed_step_records_and_is_keyed_by_the_setting(do_sample, graph_model):
    m = graph_model
    g = torch.Generator().manual_seed(31 + do_sample)
    ctx, prompt = _rand(g, 30), _rand(g, 13)
    pen = 1.3

    def run(top, **over):
        """top None: recording off -> (ids, route); else -> (ids, route, output)."""
        kw = dict(inputs_embeds=prompt, past_key_values=m(inputs_embeds=ctx).past_key_values, max_new_tokens=12, eos_token_id=-1, repetition_penalty=pen, do_sample=do_sample, seed=5,
                  return_dict_in_generate=True, **(SAMPLING if do_sample else {}))
        kw.update(over)
        out = m.generate(**kw) if top is None else m.generate(output_logprobs=True, top_logprobs=top, **kw)
        return out.sequences[0].tolist(), m.decode_last_route(), out

    ids_off, route, _ = run(None)
    assert route in (1, 2) and len(ids_off) == 12
    ids, route, out = run(3)
    assert route == 2 and ids == ids_off          # the setting is part of the step's key; recording changes no id
    assert tuple(out.logprobs.shape) == (1, 12) and tuple(out.top_logprob_ids.shape) == (1, 12, 3)
    check_records(out, replay_rows(m, ctx, prompt, ids), ids, do_sample, pen, TOL_TRUE)
    assert (out.sampling_logprobs != out.logprobs).any()
    again = run(3)
    assert again[1] == 1 and again[0] == ids_off          # the same key: a plain replay, the same records bit for bit
    for f in ('logprobs', 'sampling_logprobs', 'top_logprobs', 'top_logprob_ids'):
        assert torch.equal(getattr(again[2], f), getattr(out, f))
    other = run(1)
    assert other[1] == 2 and other[0] == ids_off          # another top_n: captured again ...
    assert torch.equal(other[2].logprobs, out.logprobs) and torch.equal(other[2].top_logprob_ids, out.top_logprob_ids[:, :, :1])
    assert run(1)[1] == 1                                 # ... then replayed
    off = run(None)
    assert off[1] == 2 and off[0] == ids_off              # off: captured again ...
    off = run(None)
    assert off[1] == 1 and off[0] == ids_off              # ... then replayed, with the first off run's ids
    assert m.last_generate_logprobs() is None
    # an EOS-terminated replay has as many records as ids
    eos = ids_off[4]
    j = ids_off.index(eos)
    ids_e, _, out_e = run(3, eos_token_id=eos)
    assert ids_e == ids_off[:j + 1] and out_e.logprobs.shape[1] == j + 1 and torch.equal(out_e.logprobs, out.logprobs[:, :j + 1])
