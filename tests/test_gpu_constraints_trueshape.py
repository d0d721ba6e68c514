"""Constrained decoding on the captured decode step (the true-width two-layer bf16 model of tests/test_gpu_logprobs_trueshape.py, the one configuration of the suite that
reaches the replay): the step is keyed by constraints on / off, reads the response step for min_new_tokens from device state inside the graph, tests the EOS set in its last
node, and new table values are re-uploaded without another capture.

The ids are held against the constrained operator on logits replayed through single-row calls.  Those take other GEMM and attention forms than the captured step, so a step
counts when the operator's token scores within TOL_TRUE of the returned one under the oracle -- the bf16 figure tests/test_gpu_logprobs_trueshape.py measured for exactly
this pair of routes (0.031306)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import constraint_oracle as CO
from mmduet_amd import constraints as CS
from test_gpu_logprobs import SAMPLING
from test_gpu_logprobs_trueshape import graph_model, _rand, replay_rows, TOL_TRUE          # noqa: F401 (graph_model is the fixture)


@pytest.mark.parametrize('do_sample', [False, True], ids=['greedy', 'sampled'])
def test_captured_step_under_constraints(do_sample, graph_model):
    m = graph_model
    V = m.config.vocab_size
    g = torch.Generator().manual_seed(41 + do_sample)
    ctx, prompt = _rand(g, 30), _rand(g, 13)
    pen = 1.3

    def run(**over):
        kw = dict(inputs_embeds=prompt, past_key_values=m(inputs_embeds=ctx).past_key_values, max_new_tokens=12, eos_token_id=-1, repetition_penalty=pen, do_sample=do_sample, seed=5,
                  **(SAMPLING if do_sample else {}))
        kw.update(over)
        return m.generate(**kw)[0].tolist(), m.decode_last_route()

    ids0, route = run()
    assert route in (1, 2) and len(ids0) == 12
    eos = [ids0[4], ids0[8]]
    j = next(i for i, t in enumerate(ids0) if t in eos)
    blocked = next(t for t in ids0 if t not in eos)
    kb = ids0.index(blocked)
    # constraints on: another captured step (2), then a replay (1)
    a, route = run(eos_token_id=eos, suppress_tokens=[(blocked + 1) % V])
    assert route == 2 and a == ids0[:j + 1]          # the EOS set is tested on the device: the run stops at its first member; an id nobody emits is suppressed for nothing
    a2, route = run(eos_token_id=eos, suppress_tokens=[(blocked + 1) % V])
    assert route == 1 and a2 == a
    # min_new_tokens is read from the step state inside the graph; only values change against the call before: still a replay
    cons = CS.merge(V, eos, 7, [blocked], sequence_bias={(ids0[1],): -0.5})
    b, route = run(eos_token_id=eos, min_new_tokens=7, suppress_tokens=[blocked], sequence_bias={(ids0[1],): -0.5})
    assert route == 1
    assert len(b) >= 7 and not set(b[:7]) & set(eos) and blocked not in b and b[:min(j, kb)] == ids0[:min(j, kb)]
    assert all(t not in eos for t in b[:-1])
    # against the constrained operator on replayed logits
    logits = replay_rows(m, ctx, prompt, b)
    T = SAMPLING['temperature'] if do_sample else 1.0
    for step, tok in enumerate(b):
        z = CO.scores(logits[step].numpy(), cons, step, b[:step], pen, T)
        assert z[tok] > -np.inf
        if not do_sample:
            t1 = int(m.sample_constrained_op(logits[step], cons, step, prev_ids=b[:step], repetition_penalty=pen, greedy=True)[0])
            assert t1 == tok or abs(z[t1] - z[tok]) <= TOL_TRUE, (step, tok, t1)
    # off again: the unconstrained step is captured again (its key is another), with the first run's ids
    off, route = run()
    assert route == 2 and off == ids0
    assert run()[1] == 1
