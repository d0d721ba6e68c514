"""The state of a response in progress lives in one struct with one set of helpers (mmduet_amd/csrc/response_plan.h, model.hip's `Response`), used by the generate calls and
by the samplers' rounds.  That was a move of host bookkeeping: tests/golden/response_parent.json holds token ids and log-probability records as raw bit patterns, recorded
with tests/response_record.py at the commit before the move (twice: an entry that differed between the two recordings would be listed as left out), and every entry must
come back bit for bit.  Then the buffers that grow -- each crossed by a few entries past its first size, not by a long decode -- and the memory a sampler and a context hand
back."""
import gc
import json
import os
import pytest
import torch

import response_record as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURE = json.load(open(os.path.join(GOLDEN, 'response_parent.json')))
GENERATE_CASES = [c for c in R.CASES if c != 'rounds' and c not in FIXTURE['left_out']]          # (what the parent itself did not repeat is listed, not compared)


@pytest.fixture(scope='module')
def models():
    """the three contexts of the recording, built when first asked for"""
    built = {}

    def get(kind):
        if kind not in built:
            built[kind] = R.build(kind)
        return built[kind]
    return get


@pytest.fixture(scope='module')
def recorded(models):
    """the generate cases of one context, recorded once: kind -> entries"""
    done = {}

    def get(kind):
        if kind not in done:
            done[kind] = R.record_generate(models(kind), kind + '_', R.CROSS if kind == 'f32' else R.CORNERS)
        return done[kind]
    return get


def test_the_fixture_holds_every_case_within_the_caps():
    assert sorted(list(FIXTURE['entries']) + FIXTURE['left_out']) == sorted(R.CASES)
    assert R.left_out_within_the_caps(FIXTURE['left_out']), FIXTURE['left_out']          # none of the fp32 cases, at most one in eight of the bf16 ones


@pytest.mark.parametrize('case', GENERATE_CASES)
def test_generate_calls_equal_the_parent_commit(recorded, case):
    got = recorded(case.split('_')[0])[case]
    assert got == FIXTURE['entries'][case], case
    a = case.split('_')[1:]
    assert (got['rec'] is not None) == ('lp' in a) and (got['prev'] is not None) == ('pen' in a) and 1 <= len(got['ids']) <= R.NEW_TOKENS


def test_rounds_equal_the_parent_commit(models):
    got = R.record_rounds(models('f32'))
    assert got == FIXTURE['entries']['rounds']
    assert list(got) == ['runs_into_max_new', 'ends_on_eos', 'second_turn'] and len(got['runs_into_max_new']['tokens']) == 5 and len(got['second_turn']['tokens']) == 4
    for r in got.values():          # the sampled sampler's records: one per token the rounds returned to it, EOS included
        assert len(r['rec']['logprobs']) == sum(t[2] is not None for t in r['tokens'])


# ---- growth -------------------------------------------------------------------------------------------------------------------------------------------------
def sampler_rounds(m, s, eos, pen, prev, max_new, rounds=4):
    H = m.config.hidden_size
    x = torch.randn(3, H, generator=torch.Generator().manual_seed(8)).cuda() * 0.5
    s.begin(eos, pen, prev, max_new)
    out = m.round_multi([dict(x=x, cache=None, sampler=s, sample=True)])
    toks = [out[0]['token']]
    for _ in range(rounds - 1):
        out = m.round_multi([dict(x=None, cache=out[0]['cache'], sampler=s, feed=True, sample=True)])
        toks.append(out[0]['token'])
    return toks, R.records(s.read_logprobs())


def test_a_samplers_penalty_list_grows_past_its_first_size(models):
    """1020 ids + 8 new tokens + the slot behind the list = 1029 > 1024: the list doubles in begin().  The same response on a sampler whose list had room already."""
    m, V = models('f32'), models('f32').config.vocab_size
    prev = [(7 * i + 3) % V for i in range(1020)]
    grown, roomy = m.new_sampler(), m.new_sampler()
    sampler_rounds(m, roomy, -1, 1.3, prev + prev + prev, 8, rounds=1)          # 3069 -> a list of 4096
    a, b = sampler_rounds(m, grown, -1, 1.3, prev, 8), sampler_rounds(m, roomy, -1, 1.3, prev, 8)
    assert a == b and len(a[0]) == 4 and all(0 <= t < V for t in a[0])


def test_a_samplers_records_grow_past_their_first_size(models):
    """max_new = 260 > 256: begin() reserves 512 records; four tokens are decoded.  The same response on a sampler whose records had room already."""
    m = models('f32')
    grown, roomy = m.new_sampler(), m.new_sampler()
    for s in (grown, roomy):
        s.set_logprobs(R.TOP_N)
    sampler_rounds(m, roomy, -1, None, None, 600, rounds=1)          # -> 1024 records
    a, b = sampler_rounds(m, grown, -1, None, None, 260), sampler_rounds(m, roomy, -1, None, None, 260)
    assert a == b and len(a[1]['logprobs']) == 4 and len(a[1]['top_logprob_ids']) == 4 * R.TOP_N


@pytest.mark.parametrize('kind', ('f32', 'graph'))
def test_a_contexts_buffers_grow_past_their_first_sizes(kind):
    """A context of its own (no earlier test has grown it).  The penalty list: 16380 ids + 8 new tokens > 16384.  The records: max_new = 1030 > 1024, the response ended at
    its fourth token by a set with min_new = 3 and a large bias on its EOS id.  Each call is made twice: the second has room to spare and must return the same ids and
    records.  On the context with captured decode steps the call that moved a buffer captures its step anew (route 2: the old step held the old pointer), the next
    identical call replays it (route 1)."""
    m = R.build(kind)
    V, x = m.config.vocab_size, R.prompt(m)
    from mmduet_amd import constraints as CS
    routes = []

    def call(**kw):
        out = R.generate(m, x, 0, **kw)
        routes.append(m.decode_last_route())
        return out

    small = dict(pen=1, cons=None, rec=1, max_new=8)
    first = [call(**small), call(**small)]
    assert first[0] == first[1]
    big = [(7 * i + 3) % V for i in range(16380)]
    lists = [call(prev=big, **small), call(prev=big, **small)]
    assert lists[0] == lists[1] and len(lists[0]['ids']) == 8 and lists[0]['prev'] == big + lists[0]['ids']
    eos = first[0]['ids'][3]
    cons = CS.merge(V, eos_token_id=[eos], min_new_tokens=3, sequence_bias={(eos,): 1e4})
    ended = [call(pen=0, cons=cons, rec=1, max_new=12), call(pen=0, cons=cons, rec=1, max_new=12)]
    recs = [call(pen=0, cons=cons, rec=1, max_new=1030), call(pen=0, cons=cons, rec=1, max_new=1030)]
    assert ended[0] == ended[1] == recs[0] == recs[1]
    assert len(recs[0]['ids']) == 4 and recs[0]['ids'][3] == eos and eos not in recs[0]['ids'][:3] and len(recs[0]['rec']['logprobs']) == 4
    assert routes == ([2, 1, 2, 1, 2, 1, 2, 1] if kind == 'graph' else [0] * 8), routes


# ---- memory -------------------------------------------------------------------------------------------------------------------------------------------------
def free_bytes():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def test_samplers_and_the_context_return_their_memory():
    """twenty samplers, each with a constraint table, records and a penalty list past its first size, leave free device memory where it was; destroying the context then
    returns what its own response state and the rounds had reserved"""
    from mmduet_amd import constraints as CS

    def context():
        m = R.build('f32')
        V = m.config.vocab_size
        cons = CS.merge(V, eos_token_id=[5], min_new_tokens=2, suppress_tokens=[7], sequence_bias={(9,): 1.5})
        x, free = R.prompt(m), []
        R.generate(m, x, 1, 1, cons, 1, max_new=4)          # the context's own list, table and records
        for i in range(21):
            s = m.new_sampler()
            s.set_logprobs(R.TOP_N)
            s.begin(-1, 1.3, [(3 * k + i) % V for k in range(1500)], 300, constraints=cons)
            if i == 0:
                m.round_multi([dict(x=x[0], cache=None, sampler=s, sample=True)])          # the rounds' lazily reserved buffers, once
            del s
            free.append(free_bytes())
        assert free[1:] == [free[0]] * 20, free
        del m

    context()          # (the first context of a process also loads code objects: the second is measured)
    before = free_bytes()
    context()
    assert free_bytes() == before
