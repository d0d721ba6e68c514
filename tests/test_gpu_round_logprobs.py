"""Per-token log-probabilities from the multi-stream rounds (mmd_sampler_set_logprobs / mmd_sampler_logprobs_read / mmd_round_multi, DESIGN.md "Log-probabilities"): three
streams in shared rounds -- plain greedy with a penalty list, constrained greedy, sampled -- each recording into its own sampler's array with its own top_n.

Tolerances, none of them new.  fp32: DELTA_E2E of tests/test_gpu_logprobs.py, on logits replayed through single-row model calls.  bf16: measured, not chosen -- BF16_MEASURED
is the largest |log_softmax| difference, at the generated ids of these three streams, between the rows of shared mmd_frame_step_multi calls (`multi_step` with logits) and
single-row replay calls (tools/round_logits_routes.py, profiles/r12_round_logprobs.md); the round is a third accumulation order of the same class, so the test allows twice
that plus logprob_oracle.bound (the convention of test_generate_end_to_end_bf16)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import constraint_oracle as CO
import logprob_oracle as LO
from helpers import hip_model, stream_cases, stream_frames, run_stream_case, tokenizer_for
from mmduet_amd import constraints as CS
from mmduet_amd._lib import lib
from test_gpu_logprobs import check_records, replay_rows, DELTA_E2E, SAMPLING, prompt, bf16_model

BF16_MEASURED = 0.0          # profiles/r12_round_logprobs.md
N_NEW = 12
PEN = 1.15
MMD_EINVAL, MMD_ERANGE = -22, -34
DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ['fp32', 'bf16']


def tol_of(dtype):
    return DELTA_E2E if dtype == torch.float32 else (lambda v: 2 * BF16_MEASURED + LO.bound(v))


_fp32 = []


def model_of(dtype):
    if dtype == torch.bfloat16:
        return bf16_model()
    if not _fp32:
        _fp32.append(hip_model('A', torch.float32)[0])
    return _fp32[0]


_cons = {}


def constraint_set(m):
    """two ids of the unconstrained greedy response suppressed, a third pushed down, one it does not hold pushed up: the constrained response leaves the free one early"""
    if m not in _cons:
        free = m.generate(inputs_embeds=prompt(), max_new_tokens=N_NEW, eos_token_id=-1)[0].tolist()
        other = next(t for t in range(m.config.vocab_size) if t not in free)
        _cons[m] = CS.merge(m.config.vocab_size, suppress_tokens=[free[0], free[2]], sequence_bias={(free[1],): -0.5, (other,): 0.25})
    return _cons[m]


def three_streams(m, tops, samplers=None):
    """plain greedy with a penalty list | constrained greedy | sampled; tops: each stream's top_n (None: it does not record).  samplers: the ones of an earlier run (a
    sampled stream's draws are its sampler's lane's)"""
    x = prompt()
    kinds = (dict(pen=PEN, prev=[]), dict(constraints=constraint_set(m)), dict(sampling=dict(seed=7, restart=True, **SAMPLING)))
    samplers = samplers or [m.new_sampler() for _ in kinds]
    return [dict(x=x, sampler=sp, top=t, **k) for k, t, sp in zip(kinds, tops, samplers)]


def run_rounds(m, streams, n_new=N_NEW):
    """The streams' responses, a shared round per token.  A stream with start = r begins in round r; rebegin = r begins AGAIN in round r (a new response on the same
    sampler: its records restart at slot 0, its tokens and cache go on).  -> (ids per stream, mmd_op_round_last_record of every round)"""
    state = [dict(ids=[], cache=None, done=False, begun=False) for _ in streams]
    rnd, seen = 0, []
    while not all(st['done'] for st in state):
        segs, who = [], []
        for i, (s, st) in enumerate(zip(streams, state)):
            if st['done'] or rnd < s.get('start', 0):
                continue
            if not st['begun'] or s.get('rebegin') == rnd:
                s['sampler'].begin(s.get('eos', -1), s.get('pen'), s.get('prev'), n_new, sampling=s.get('sampling'), constraints=s.get('constraints'))
                if s.get('top') is not None or getattr(s['sampler'], '_logprobs_top', -1) >= 0:
                    s['sampler'].set_logprobs(s.get('top'))
                st['first'] = len(st['ids'])          # the tokens of the response whose records are read at the end
            if not st['begun']:
                segs.append(dict(x=s['x'], cache=None, sampler=s['sampler'], sample=True))
                st['begun'] = True
            else:
                segs.append(dict(x=None, cache=st['cache'], sampler=s['sampler'], feed=True, sample=True))
            who.append(i)
        out = m.round_multi(segs)
        seen.append(tuple(m.round_last_record().values()))
        for i, o in zip(who, out):
            st = state[i]
            st['ids'].append(o['token']); st['cache'] = o['cache']
            st['done'] = o['token'] == streams[i].get('eos', -1) or len(st['ids']) >= n_new
        rnd += 1
    for s, st in zip(streams, state):
        s['first'] = st['first']
    return [st['ids'] for st in state], seen


def as_out(rec):
    """a sampler's records in the shape check_records reads (a batch of one)"""
    return SimpleNamespace(logprobs=rec['logprobs'][None], sampling_logprobs=rec['sampling_logprobs'][None], top_logprobs=rec['top_logprobs'][None],
                           top_logprob_ids=rec['top_logprob_ids'][None])


def read_count(sampler):
    n = C.c_int(-1)
    rc = lib().mmd_sampler_logprobs_read(sampler.h, None, None, None, None, 1 << 20, C.byref(n))
    return rc, n.value


_runs = {}


def runs(dtype):
    """(ids, rounds' records, streams) of the three streams with recording off | streams 0 and 2 recording (top_n 3 and 0) | all three (3, 2, 0) | off again, on the same
    three samplers, computed once per dtype"""
    if dtype not in _runs:
        m = model_of(dtype)
        got, samplers = {}, None
        for name, tops in (('off', (None, None, None)), ('partial', (3, None, 0)), ('all', (3, 2, 0)), ('off_again', (None, None, None))):
            streams = three_streams(m, tops, samplers)
            samplers = [s['sampler'] for s in streams]
            ids, seen = run_rounds(m, streams)
            plan = m.select_last_plan()
            got[name] = SimpleNamespace(ids=ids, seen=seen, streams=streams, plan=plan, recs=[s['sampler'].read_logprobs() for s in streams], counts=[read_count(sp) for sp in samplers])
        _runs[dtype] = got
    return _runs[dtype]


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_ids_and_counts(dtype):
    r = runs(dtype)
    off, part, full, again = r['off'], r['partial'], r['all'], r['off_again']
    assert all(len(i) == N_NEW for i in off.ids)
    assert part.ids == off.ids and full.ids == off.ids and again.ids == off.ids          # recording changes no id
    assert len({tuple(i) for i in off.ids}) == 3
    # off: nothing recorded in any round, and the selection's plan is the one of the round without this feature (select_regimes: one row per block, the sampled block last)
    assert set(off.seen) == {(0, 0, 0, -1)}
    assert tuple(off.plan['round'].values()) == (1, 2, 3, 1, 1, 0)
    assert tuple(off.plan['select'].values()) == (2, 0, 1, 1, 1, 0, 0, 0, 0, 0)
    for o in (off, again):          # (switched off again: the round is the one it was)
        assert set(o.seen) == {(0, 0, 0, -1)} and o.plan == off.plan and o.recs == [None, None, None] and o.counts == [(0, 0)] * 3
    # streams 0 and 2 record, stream 1 does not
    assert set(part.seen) == {(1, 0, 1, 3)}
    assert part.counts == [(0, N_NEW), (0, 0), (0, N_NEW)] and part.recs[1] is None
    for rec, top in ((part.recs[0], 3), (part.recs[2], 0)):
        assert tuple(rec['logprobs'].shape) == tuple(rec['sampling_logprobs'].shape) == (N_NEW,)
        assert tuple(rec['top_logprobs'].shape) == tuple(rec['top_logprob_ids'].shape) == (N_NEW, top)
        assert rec['logprobs'].dtype == rec['sampling_logprobs'].dtype == rec['top_logprobs'].dtype == torch.float32 and rec['top_logprob_ids'].dtype == torch.long
    assert tuple(part.plan['round'].values()) == (1, 2, 3, 1, 1, 0) and part.plan['select']['record'] == 1
    # all three: every block has a tail
    assert set(full.seen) == {(1, 1, 1, 3)}
    assert full.counts == [(0, N_NEW)] * 3
    # a row's numbers do not depend on which other rows record, nor on their top_n
    for a, b in ((part.recs[0], full.recs[0]), (part.recs[2], full.recs[2])):
        assert all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]) for k in a)


def check_constrained(rec, logits, ids, cons, tol, top):
    """check_records for the constrained arg-max: logprob and the alternatives over the raw logits, sampling_logprob over the constrained scores with nothing filtered"""
    lp, slp = rec['logprobs'].double().numpy(), rec['sampling_logprobs'].double().numpy()
    tol_f = tol if callable(tol) else (lambda v: tol)
    for step, tok in enumerate(ids):
        t = float(tol_f(lp[step]))
        l = logits[step].numpy()
        z = CO.scores(l, cons, step, None, None, 1.0)
        assert z[tok] >= z.max() - t, (step, tok)
        assert abs(lp[step] - LO.logprob(l, tok)) <= t, (step, lp[step])
        assert abs(slp[step] - LO.sampling_logprob(z, np.ones(len(z), bool), tok)) <= t, (step, slp[step])
        dev_ids = rec['top_logprob_ids'][step].tolist()
        _, want_top = LO.top_n(l, top)
        lse = LO.logsumexp(l)
        assert len(set(dev_ids)) == top
        for j, i in enumerate(dev_ids):
            assert abs((l[i] - lse) - want_top[j]) <= t and abs(rec['top_logprobs'][step, j].item() - (l[i] - lse)) <= t
    assert (lp <= 0).all() and (slp <= 0).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_values_against_the_oracle_on_replayed_logits(dtype):
    m, full, tol = model_of(dtype), runs(dtype)['all'], tol_of(dtype)
    x = prompt()
    logits = [replay_rows(m, x, ids) for ids in full.ids]
    check_records(as_out(full.recs[0]), logits[0], full.ids[0], False, PEN, tol, top=3)
    check_constrained(full.recs[1], logits[1], full.ids[1], full.streams[1]['constraints'], tol, 2)
    check_records(as_out(full.recs[2]), logits[2], full.ids[2], True, None, tol, top=0)
    assert (full.recs[0]['sampling_logprobs'] != full.recs[0]['logprobs']).any()          # the penalty list moves the distribution the token is taken from
    assert (full.recs[1]['sampling_logprobs'] != full.recs[1]['logprobs']).any()          # ... and so do the bias and the suppressed ids


def test_twin_streams_record_the_same_bits():
    """Two streams with the same prompt and the same plain-greedy settings share every round; one records 8 alternatives, the other 2.  The second stream is begun again in
    round 1 (a second response on its sampler, tokens and cache going on), so from then on its slot is one behind its twin's while both rows of a round carry the same
    inputs: identical logits rows, identical records -- whatever the slot, the other row's top_n, the position in the launch."""
    m, x = model_of(torch.float32), prompt()
    a, b = dict(x=x, sampler=m.new_sampler(), top=8), dict(x=x, sampler=m.new_sampler(), top=2, rebegin=1)
    ids, seen = run_rounds(m, [a, b], n_new=N_NEW)
    assert ids[0] == ids[1][:N_NEW] and len(ids[0]) == N_NEW
    assert set(seen) == {(2, 0, 0, 8)}
    ra, rb = a['sampler'].read_logprobs(), b['sampler'].read_logprobs()
    assert b['first'] == 1 and ra['logprobs'].shape[0] == N_NEW and rb['logprobs'].shape[0] == N_NEW - 1          # the second response: tokens 1..
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(ra['logprobs'][1:]), bits(rb['logprobs'])) and torch.equal(bits(ra['sampling_logprobs'][1:]), bits(rb['sampling_logprobs']))
    assert torch.equal(ra['top_logprob_ids'][1:, :2], rb['top_logprob_ids']) and torch.equal(bits(ra['top_logprobs'][1:, :2].contiguous()), bits(rb['top_logprobs']))
    assert torch.equal(bits(ra['sampling_logprobs']), bits(ra['logprobs']))          # plain route, no penalty: z is l, the same sums, the same bits
    assert (ra['top_logprobs'][:, :-1] >= ra['top_logprobs'][:, 1:]).all() and torch.equal(ra['top_logprobs'][:, 0], ra['logprobs'])          # the arg-max is the first alternative


def test_responses_eos_and_a_second_begin():
    m, x = model_of(torch.float32), prompt()
    base = runs(torch.float32)['all']
    ids0, rec0 = base.ids[0], base.recs[0]
    # EOS is a returned token: it has a record and is counted
    eos = ids0[3]
    j = ids0.index(eos)
    s = dict(x=x, sampler=m.new_sampler(), top=3, pen=PEN, prev=[], eos=eos)
    ids, _ = run_rounds(m, [s])
    assert ids[0] == ids0[:j + 1] and read_count(s['sampler']) == (0, j + 1)
    rec = s['sampler'].read_logprobs()
    assert rec['logprobs'].shape[0] == j + 1 and torch.isfinite(rec['logprobs']).all()
    # a second response on the same sampler, the penalty list carried over by the caller as the driver does: records from slot 0, only its own tokens
    first = [t for t in ids[0] if t != eos]
    s2 = dict(s, eos=-1, prev=list(first))
    ids2, _ = run_rounds(m, [s2], n_new=5)
    assert read_count(s['sampler']) == (0, 5)
    rec2 = s['sampler'].read_logprobs()
    assert rec2['logprobs'].shape[0] == 5 and tuple(rec2['top_logprobs'].shape) == (5, 3)
    logits = replay_rows(m, x, ids2[0])
    lp, slp = rec2['logprobs'].double().numpy(), rec2['sampling_logprobs'].double().numpy()
    for step, tok in enumerate(ids2[0]):
        want_lp, want_slp, _, _ = LO.record(logits[step].numpy(), tok, first + ids2[0][:step], PEN, greedy=True)
        assert abs(lp[step] - want_lp) <= DELTA_E2E and abs(slp[step] - want_slp) <= DELTA_E2E, (step, lp[step], want_lp, slp[step], want_slp)
    assert (rec2['sampling_logprobs'] != rec2['logprobs']).any()
    assert (rec0['sampling_logprobs'] != rec0['logprobs']).any()


def test_argument_checks():
    m, x = model_of(torch.float32), prompt()
    L = lib()
    s = m.new_sampler()
    assert L.mmd_sampler_set_logprobs(s.h, 9) == MMD_ERANGE and L.mmd_sampler_set_logprobs(s.h, -2) == MMD_ERANGE
    with pytest.raises(Exception):
        s.set_logprobs(9)
    assert L.mmd_sampler_set_logprobs(s.h, 2) == 0          # before the first begin
    s.begin(-1, None, None, 4)
    assert L.mmd_sampler_set_logprobs(s.h, 1) == 0          # after begin, before the response's first token
    out = m.round_multi([dict(x=x, cache=None, sampler=s, sample=True)])
    assert L.mmd_sampler_set_logprobs(s.h, 2) == MMD_EINVAL and L.mmd_sampler_set_logprobs(s.h, -1) == MMD_EINVAL          # a token has been returned
    out = m.round_multi([dict(x=None, cache=out[0]['cache'], sampler=s, feed=True, sample=True)])
    n = C.c_int(-1)
    lp = (C.c_float * 2)()
    assert L.mmd_sampler_logprobs_read(s.h, lp, None, None, None, 1, C.byref(n)) == MMD_ERANGE and n.value == 2          # room for one of two
    assert L.mmd_sampler_logprobs_read(s.h, None, None, None, None, 2, C.byref(n)) == 0 and n.value == 2          # every output may be NULL
    assert L.mmd_sampler_logprobs_read(s.h, lp, None, None, None, 2, C.byref(n)) == 0 and n.value == 2 and lp[0] <= 0 and lp[1] <= 0
    assert L.mmd_sampler_logprobs_read(s.h, lp, None, None, None, 2, None) == MMD_EINVAL
    s._logprobs_top = 1
    rec = s.read_logprobs()
    assert tuple(rec['top_logprobs'].shape) == (2, 1) and rec['logprobs'].tolist() == [lp[0], lp[1]]


def test_scheduler_driver_records_beside_the_ids():
    """MultiStreamInfer with 2 slots over the prob_keep_pen case (five responses, a penalty list carried across them), output_logprobs with two alternatives: the ids are
    the case's, the records line up with them and agree with the single-stream driver's within the fp32 tolerance of the values test."""
    from mmduet_amd.inference import LiveInferForBenchmark
    from mmduet_amd.multistream import MultiStreamInfer
    from test_gpu_multistream import _args_for
    m = model_of(torch.float32)
    meta = stream_cases()
    name = 'prob_keep_pen'
    case = meta['cases'][name]

    class WithLogprobs(LiveInferForBenchmark):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.output_logprobs, self.top_logprobs = True, 2

    single = run_stream_case(WithLogprobs, m, name, case, meta)
    assert single.response_token_ids == case['generated']
    tok = tokenizer_for(m.config)
    m.config.eos_token_id = meta['eos_token_id']
    videos = [dict(frames=stream_frames(name), conversation=case['conversation'], args=_args_for(case, 1), driver_attrs=dict(output_logprobs=True, top_logprobs=2)) for _ in range(2)]
    ms = MultiStreamInfer(videos[0]['args'], model=m, tokenizer=tok, n_slots=2)
    results = ms.run(videos)
    assert tuple(m.round_last_record().values())[3] in (2, -1)
    for res in results:
        assert res['response_token_ids'] == case['generated']
        assert len(res['response_logprobs']) == len(res['response_token_ids']) == len(single.response_logprobs)
        differ = False
        for ids, rec, ref in zip(res['response_token_ids'], res['response_logprobs'], single.response_logprobs):
            assert len(rec['logprobs']) == len(rec['sampling_logprobs']) == len(rec['top']) == len(ids)
            assert all(len(t) == 2 and t[0][1] >= t[1][1] for t in rec['top'])
            for key in ('logprobs', 'sampling_logprobs'):
                assert np.abs(np.array(rec[key]) - np.array(ref[key])).max() <= DELTA_E2E, key
            for t, u in zip(rec['top'], ref['top']):
                assert all(abs(a[1] - b[1]) <= DELTA_E2E for a, b in zip(t, u))
            differ |= rec['logprobs'] != rec['sampling_logprobs']
        assert differ          # the case carries a penalty list
    # a driver around a proxy that cannot record still refuses (tests/test_gpu_logprobs.py::test_driver_refuses_the_multi_stream_proxy), and recording is off again
    off = MultiStreamInfer(videos[0]['args'], model=m, tokenizer=tok, n_slots=2).run([dict(v, driver_attrs={}) for v in videos])
    assert all(r['response_logprobs'] == [] and r['response_token_ids'] == case['generated'] for r in off)
    assert tuple(m.round_last_record().values()) == (0, 0, 0, -1)
