"""The token-selection table (tests/select_regimes.py) on the device: generate calls on the eager and on the captured route, a mixed scheduler round and the raw operator
run under the rows' switches, and `select_last_plan()` -- the plans the launches came from -- must equal the table's.  (tests/test_select_plan_host.py checks every row
against the planner on the host.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import constraint_oracle as CO
import select_regimes as T
from helpers import hip_model
from mmduet_amd import constraints as CS
from test_gpu_sampling import DELTA, words, check_row

PEN, PREV = 1.2, [3, 4]
SAMPLING = dict(temperature=0.9, top_k=0, top_p=1.0, seed=7)          # the generate rows of the table draw with no filter
S = T.by_name(T.SELECT_ROWS)


@pytest.fixture(scope='module')
def small():
    """the small fp32 model of tests/test_gpu_constraints.py: every generate call takes the eager route"""
    return hip_model('A', torch.float32)[0]


@pytest.fixture(scope='module')
def graph_model():
    """the 2-layer true-width bf16 model of tests/test_gpu_step_regimes.py, created with the captured decode step switched on"""
    from oracle import duet_oracle as O
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    ocfg = O.OracleConfig(vocab_size=T.V, num_hidden_layers=2, vit_layers=1)
    w = O.random_weights(ocfg, seed=3, dtype=torch.bfloat16, scale='unit')
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=T.V, num_hidden_layers=2, vit_num_hidden_layers=2, vit_layers_removed=1,
                                        frame_num_tokens=49, frame_resolution=384, v_placeholder='<image>')
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('MMDUET_GRAPH', '1')
        m = VideoHeadLiveLlavaQwenForCausalLM(pcfg, torch_dtype=torch.bfloat16, max_vit_batch=1, max_step_tokens=64, kv_initial_tokens=1024)
    m.load_state_dict(w)
    return m


def run_generate(m, row, x, eos, max_new):
    """one generate call under the row's switches: -> (ids, records or None).  The context's settings are put back."""
    a = row.inputs
    V = m.config.vocab_size
    m.set_generate_logprobs(T.LP_TOP if a['record'] else -1)
    m.set_generate_constraints(CS.merge(V, suppress_tokens=[0, 5], sequence_bias={(7,): 1.5}) if a['constrained'] else None)
    try:
        pen, prev = (PEN, list(PREV)) if a['pen'] else (None, None)
        if a['sampled']:
            ids = m.sample_generate(x, None, eos, max_new, pen, prev, **SAMPLING)[0]
        else:
            ids = m.greedy_generate(x, None, eos, max_new, pen, prev)[0]
        return ids, m.last_generate_logprobs()
    finally:
        m.set_generate_logprobs(-1)
        m.set_generate_constraints(None)


def plans_of(m):
    p = m.select_last_plan()
    return tuple(p['select'].values()), tuple(p['generate'].values()) if p['generate'] else None


def check_ids(ids, rec, row, V):
    assert all(0 <= t < V for t in ids), ids
    if row.inputs['record']:
        assert rec is not None and rec['logprobs'].shape[0] == len(ids) and rec['top_logprob_ids'].shape == (len(ids), T.LP_TOP)
    else:
        assert rec is None


@pytest.mark.parametrize('row', T.generate_gpu_rows('fp32'), ids=[r.name for r in T.generate_gpu_rows('fp32')])
def test_eager_generate_takes_the_plans_of_the_table(small, row):
    m, V = small, small.config.vocab_size
    x = torch.randn(3, m.config.hidden_size, generator=torch.Generator().manual_seed(5)) * 0.5
    eos = -1
    if row.inputs['first_is_eos']:          # the token the call draws first, as its EOS id
        eos = run_generate(m, row, x, -1, 1)[0][0]
    ids, rec = run_generate(m, row, x, eos, row.inputs['max_new'])
    assert len(ids) == (1 if row.inputs['first_is_eos'] else row.inputs['max_new'])
    assert plans_of(m) == (S[row.select].plan, row.plan), (row.name, m.select_last_plan())
    assert m.decode_last_route() == 0
    check_ids(ids, rec, row, V)


@pytest.mark.parametrize('row', [r for r in T.generate_gpu_rows('graph') if not r.inputs['pen']], ids=lambda r: r.name)
def test_captured_generate_takes_the_plans_of_the_table(graph_model, row):
    m = graph_model
    x = (torch.randn(3, m.config.hidden_size, generator=torch.Generator().manual_seed(6)) * 0.5).to(torch.bfloat16)
    runs = []
    for route in (2, 1):          # captured in the first call, replayed as it is in the second
        ids, rec = run_generate(m, row, x, -1, row.inputs['max_new'])
        assert plans_of(m) == (S[row.select].plan, row.plan), (row.name, route, m.select_last_plan())
        assert row.plan[0] == 1 and m.decode_last_route() == route, (row.name, route, m.decode_last_route())
        assert len(ids) == row.inputs['max_new']
        check_ids(ids, rec, row, T.V)
        runs.append(ids)
    assert runs[0] == runs[1]          # same seed, same offset


def test_mixed_round_takes_the_blocks_of_the_table(small):
    m, V, H = small, small.config.vocab_size, small.config.hidden_size
    row = T.by_name(T.ROUND_ROWS)['mixed']
    g = torch.Generator().manual_seed(33)
    xs = [torch.randn(1, H, generator=g).cuda() * 0.5 for _ in row.segs]
    x2 = torch.randn(1, H, generator=g).cuda() * 0.5          # the second row of the segment that does not sample
    cons = CS.merge(V, suppress_tokens=[1, 2], sequence_bias={(9,): 2.0})
    smps = [m.new_sampler() for _ in row.segs]

    def begin(i, restart=False):
        feed, sample, sampling, constrained = row.segs[i][:4]
        smps[i].begin(-1, PEN, PREV, 2, sampling=dict(temperature=0.9, top_k=0, top_p=1.0, seed=11, restart=restart) if sampling else None, constraints=cons if constrained else None)

    def two_rounds(which):
        sample = [bool(row.segs[i][1]) for i in which]
        out = m.round_multi([dict(x=xs[i], cache=None, sampler=smps[i], sample=s) for i, s in zip(which, sample)])
        first, plan = [o['token'] for o in out], m.select_last_plan()['round']
        out = m.round_multi([dict(x=None if s else x2, cache=o['cache'], sampler=smps[i], feed=s, sample=s) for i, s, o in zip(which, sample, out)])
        return [(a, o['token']) for a, o in zip(first, out)], plan, m.select_last_plan()['round']

    for i in range(len(smps)):
        begin(i)
    toks, plan1, plan2 = two_rounds(range(len(smps)))
    assert tuple(plan1.values()) == row.plan and tuple(plan2.values()) == row.plan          # the feed round has the same blocks
    assert tuple(m.select_last_plan()['select'].values()) == S['block_draw'].plan          # the sampled block is launched last
    assert [t == (None, None) for t in toks] == [not s[1] for s in row.segs]
    for i, seg in enumerate(row.segs):          # batch independence: the same sampler alone, in rounds of one
        if not seg[1]:
            continue
        begin(i, restart=True)
        alone, plan, _ = two_rounds([i])
        assert alone[0] == toks[i], (i, alone, toks[i])
        assert 0 <= toks[i][0] < V and 0 <= toks[i][1] < V
        assert (plan['n_plain'], plan['n_greedy'], plan['n_sample']) == {(0, 0): (1, 1, 1), (0, 1): (0, 1, 1), (1, 0): (0, 0, 1)}[seg[2:4]]


@pytest.mark.parametrize('constrained', (False, True), ids=('free', 'cons'))
@pytest.mark.parametrize('params', ('greedy', (0.8, 20, 0.9)), ids=('greedy', 'draw'))
def test_raw_op_across_a_chunk_and_a_slice_boundary(small, params, constrained):
    """n = 33 rows (a chunk of 32 and one more), V = 515 (two slices of 256 and three columns): row 32 equals the same row run alone -- the entries take no lane, so the draw
    gets its random word handed in -- and is the token the oracles call over the device's own scores (tolerances of tests/test_gpu_sampling.py / test_gpu_constraints.py)."""
    m, n, V = small, 33, 515
    greedy = params == 'greedy'
    Tm, top_k, top_p = (1.0, 0, 1.0) if greedy else params
    lg = torch.randn(n, V, generator=torch.Generator().manual_seed(515)) * 4
    made = [CO.table_for(V, i, lg[i].numpy()) for i in range(n)]
    cons, steps = [CS.merge(V, **a) for a, _ in made], [s for _, s in made]
    r, prev = words(n, seed=33), [0, V - 1, 3, 3, 0]
    kw = dict(temperature=Tm, top_k=top_k, top_p=top_p, prev_ids=prev, repetition_penalty=1.3, greedy=greedy, top_n=2, return_scores=True)

    def run(rows):
        lo, hi = rows
        if constrained:
            return m.sample_constrained_op(lg[lo:hi], cons[lo:hi], steps[lo:hi], r=r[lo:hi], **kw)
        return m.sample_logprob_op(lg[lo:hi], r=r[lo:hi], **kw)

    toks, info, z, lp, top_ids, top_lp = run((0, n))
    want = S[('block_draw' if not greedy else 'block_argmax') + ('_cons' if constrained else '') + '_lp'].plan
    want = want[:2] + ((0, 0) if greedy else (1, 1)) + want[4:]          # top_k 20 of 515, top_p 0.9: both filters
    p = m.select_last_plan()
    assert tuple(p['select'].values()) == want and p['generate'] is None and p['round'] is None
    a_toks, a_info, a_z, a_lp, a_top_ids, a_top_lp = run((32, 33))
    bits = lambda t: t.cpu().view(torch.int32)
    assert int(toks[32]) == int(a_toks[0]) and torch.equal(bits(z[32]), bits(a_z[0]))
    assert torch.equal(bits(lp[32]), bits(a_lp[0])) and torch.equal(top_ids[32], a_top_ids[0]) and torch.equal(bits(top_lp[32]), bits(a_top_lp[0]))
    # the scores against torch fp32 in the same order of operations, then the token over the device's own z
    off = [CS.OFF] * n
    ref = torch.stack([CO.scores32(lg[i], (cons if constrained else off)[i], steps[i], prev, 1.3, Tm) for i in range(n)])
    torch.testing.assert_close(z.cpu(), ref, rtol=1e-6, atol=0)
    z64, tk = z.cpu().numpy().astype(np.float64), toks.cpu().numpy()
    for i in range(n):
        assert 0 <= tk[i] < V and z64[i, tk[i]] > -np.inf
        if greedy:
            assert info is None and tk[i] == int(z64[i].argmax())          # first maximal index
        else:
            assert info[i, 3] == 0
            check_row(z64[i], float(info[i, 0]), int(info[i, 1]), int(tk[i]), r[i], top_k, top_p, DELTA)
