"""A context built through the model plan (mmduet_amd/csrc/model_plan.h) computes what it computed before the plan existed, bit for bit: tests/golden/model_plan_parent.json
holds SHA-256 of the raw output bytes, recorded with tests/model_plan_record.py at the commit before the plan (twice: every entry repeated).  Finalize moves bytes and launches
nothing new, so there is no tolerance.  Then: a finalize refused for a missing tensor leaves the context loadable, and creating and destroying contexts returns all memory,
the lazily reserved pinned buffers included."""
import gc
import json
import os
import pytest
import torch

import model_plan_record as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURE = json.load(open(os.path.join(GOLDEN, 'model_plan_parent.json')))


def test_the_fixture_holds_every_case_and_entry():
    assert set(FIXTURE) == set(R.GPU_CASES)
    for case, spec in R.GPU_CASES.items():
        assert tuple(sorted(FIXTURE[case])) == tuple(sorted(R.VISION_ENTRIES if 'vision' in spec else R.DECODER_ENTRIES)), case


@pytest.mark.parametrize('case', list(R.GPU_CASES))
def test_outputs_equal_the_parent_commit(case):
    m = R.build(case)
    got = R.record(case, m)
    assert got == FIXTURE[case], {k: (got[k], FIXTURE[case][k]) for k in got if got[k] != FIXTURE[case][k]}


# the last tensor the plan takes in each context: before the plan, everything in front of it had been consumed, fused and freed by the time it was missed
@pytest.mark.parametrize('case,missing', [('cfgA_bf16', 'model.mm_projector.2.bias'), ('cfgB_fp8', 'model.layers.1.mlp.down_proj.weight'),
                                          ('tower_f16_1', 'model.vision_tower.vision_tower.vision_model.encoder.layers.1.mlp.fc2.bias')])
def test_a_refused_finalize_leaves_the_context_loadable(case, missing):
    from mmduet_amd._lib import MmduetError
    m, named = R.create(case)
    held = dict(named)[missing]
    for name, t in named:
        if name != missing:
            m.load_tensor(name, t)
    for _ in range(2):          # ... and a second refusal changes nothing either
        with pytest.raises(MmduetError, match='missing weight tensor'):
            m.finalize()
    m.load_tensor(missing, held)
    m.finalize()
    assert R.record(case, m) == FIXTURE[case]


def test_contexts_return_their_memory_pinned_buffers_included():
    """twenty contexts, each with a round (mmd_round_multi's buffers), a sampled generate with log-probabilities and constraints (the samplers', the records', the constraint
    rows' buffers) and an lm_nll call: every lazily reserved pinned buffer exists when the context is destroyed"""
    case = 'cfgA_bf16'
    free = []
    for i in range(20):
        m = R.build(case)
        H = m.config.hidden_size
        x = torch.randn(1, 12, H, generator=torch.Generator().manual_seed(i)).to(m.dtype)
        s = m.new_sampler()
        s.set_logprobs(2)
        s.begin(None, 1.1, [], 4, sampling=dict(temperature=0.8, top_k=5, top_p=0.9, seed=i))
        out = m.round_multi([dict(x=x[0], cache=None, head_rows=[11], sampler=s, sample=True)])
        assert out[0]['token'] is not None and out[0]['heads'].shape == (1, 4)
        m.set_generate_logprobs(2)
        m.set_generate_constraints(min_new_tokens=2, suppress_tokens=[3, 4], eos_token_id=[1])
        ids, cache, _ = m.sample_generate(x[:, :5], None, None, 4, temperature=0.7, top_k=8, top_p=0.95, seed=i)
        assert 2 <= len(ids) <= 4 and m.last_generate_logprobs()['top_logprobs'].shape == (len(ids), 2)          # (EOS may end it once min_new_tokens are out)
        rows = m(inputs_embeds=x).hidden_states[0]
        nll = m.token_nll(rows, torch.arange(12) % m.config.vocab_size)
        assert bool(torch.isfinite(nll).all())
        del s, out, cache, rows, nll, m
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[-1] == free[0], free
