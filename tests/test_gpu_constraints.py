"""Constrained decoding on the device (DESIGN.md "Constraints"): EOS sets, min_new_tokens and the (id, bias) table inside the scoring kernels of sample.hip, through
mmd_op_sample_constrained, the generate calls, mmd_round_multi and the drivers, against tests/constraint_oracle.py (pinned to HF's processors by the host test).

Bounds, none of them new: scores against torch fp32 at rtol 1e-6 (test_gpu_sampling.test_op_sample_against_oracle); tokens and kept sets through check_row with DELTA;
sampling_logprob through logprob_oracle.bound, both over the device's own z; end to end DELTA_E2E on logits replayed through other launches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import constraint_oracle as CO
import logprob_oracle as LO
import sampling_oracle as SO
from helpers import hip_model, stream_cases, stream_frames, run_stream_case, tokenizer_for
from conftest import load_npz
from mmduet_amd import constraints as CS
from mmduet_amd._lib import MmduetError
from test_gpu_sampling import PARAMS, DELTA, DELTA_E2E, words, check_row
from test_gpu_logprobs import close, kept_lse, log_softmax64, replay_rows, E2E_CASES, E2E_IDS, SAMPLING

NS = (1, 5, 32)
ALL_PARAMS = ('greedy',) + PARAMS
PEN = 1.3


@pytest.fixture(scope='module')
def model():
    return hip_model('A', torch.float32)[0]


_tables = {}


def tables(family, V):
    """The 32 rows' constraint sets and steps (built once): -> ([Constraints], [step])."""
    if (family, V) not in _tables:
        lg = LO.family_rows(family, V).numpy()
        made = [CO.table_for(V, i, lg[i]) for i in range(32)]
        _tables[(family, V)] = ([CS.merge(V, **a) for a, _ in made], [s for _, s in made])
    return _tables[(family, V)]


@pytest.mark.parametrize('params', ALL_PARAMS, ids=lambda p: p if p == 'greedy' else 'T%s-k%s-p%s' % p)
@pytest.mark.parametrize('family', LO.FAMILIES)
@pytest.mark.parametrize('V', LO.VS)
def test_op_constrained_against_oracle(model, V, family, params):
    greedy = params == 'greedy'
    T, top_k, top_p = (1.0, 0, 1.0) if greedy else params
    top_k = V + 5 if top_k == 'V+5' else top_k
    prev, pen = ([0, V - 1, 3 % V, 3 % V, 0], PEN) if family != 'equal' else (None, None)          # duplicates, both ends of the row; 3 % V is biased in rows of kind 2
    cons_all, steps_all = tables(family, V)
    rows_host, lsm = LO.family_rows(family, V), log_softmax64(family, V)
    for n in NS:
        lg, r = rows_host[:n], words(n, seed=n)
        cons, steps = cons_all[:n], steps_all[:n]
        kw = dict(temperature=T, top_k=top_k, top_p=top_p, r=r, prev_ids=prev, repetition_penalty=pen, greedy=greedy, return_scores=True)
        toks, info, z_dev, lp, top_ids, top_lp = model.sample_constrained_op(lg, cons, steps, top_n=2, **kw)
        tk, z_dev, lp = toks.cpu().numpy(), z_dev.cpu(), lp.numpy().astype(np.float64)
        # 1: the scores, against torch fp32 in the same order of operations
        want = torch.stack([CO.scores32(lg[i], cons[i], steps[i], prev, pen, T) for i in range(n)])
        torch.testing.assert_close(z_dev, want, rtol=1e-6, atol=0)
        assert torch.equal(torch.isneginf(z_dev), torch.isneginf(want))
        z64 = z_dev.numpy().astype(np.float64)
        tau = np.full(n, -np.inf) if greedy else info[:, 0].cpu().numpy().astype(np.float64)
        for i in range(n):
            tok = int(tk[i])
            assert 0 <= tok < V and z64[i, tok] > -np.inf, 'a token without a score was returned'
            masked = [t for t, b in zip(cons[i].ids, cons[i].bias) if b == -np.inf] + (list(cons[i].eos) if steps[i] < cons[i].min_new else [])
            assert tok not in masked and np.isneginf(z64[i, masked]).all()
            if cons[i].eos and steps[i] >= cons[i].min_new:          # step == min_new: the EOS ids are scored again
                assert (z64[i, list(cons[i].eos)] > -np.inf).any() or family == 'neginf'
            if greedy:
                assert info is None and tok == int(z64[i].argmax())          # first maximal index
            else:
                assert info[i, 3] == 0
                check_row(z64[i], float(info[i, 0]), int(info[i, 1]), tok, r[i], top_k, top_p, DELTA)
        rows = np.arange(n)
        assert np.isfinite(lp[:, 1]).all()
        assert close(lp[:, 1], z64[rows, tk] - kept_lse(z64, tau))
        assert close(lp[:, 0], lsm[rows, tk])          # logprob stays over the RAW logits
        # logprob (where the token is the same) and the alternatives are the bits of the same call without constraints
        t0, _, _, lp0, top_ids0, top_lp0 = model.sample_logprob_op(lg, top_n=2, **kw)
        assert torch.equal(top_ids, top_ids0) and torch.equal(top_lp.view(torch.int32), top_lp0.view(torch.int32))
        same = torch.from_numpy(tk) == t0.cpu()
        assert torch.equal(torch.from_numpy(lp[:, 0]).float()[same].view(torch.int32), lp0[:, 0][same].view(torch.int32))
        if params in ('greedy', (1.0, 0, 1.0)):
            unc = [i for i in range(n) if not cons[i].ids and not (cons[i].eos and steps[i] < cons[i].min_new)]
            assert all(same[i] for i in unc)          # an unconstrained row among constrained ones: the token of the unconstrained call


def test_forced_and_blocked_argmax(model):
    """The table kinds do what they are for, on rows with one clear maximum."""
    V = 1000
    lg = LO.family_rows('randn4', V)[:10]
    cons, steps = tables('randn4', V)
    toks = model.sample_constrained_op(lg, cons[:10], steps[:10], greedy=True)[0].cpu().tolist()
    am = lg.argmax(dim=1).tolist()
    assert toks[3] != am[3] and toks[5] != am[5] and toks[6] == am[6] and toks[9] == am[9]
    assert toks[4] == cons[4].ids[0] != am[4]          # a positive bias that changes the arg-max


def test_determinism_and_batch_independence(model):
    V, n = 152064, 32
    lg = LO.family_rows('randn4', V).cuda()
    cons, steps = tables('randn4', V)
    r = words(n, seed=99)

    def bits(out):
        return [x.cpu().view(torch.int32) if x.dtype == torch.float32 else x.cpu() for x in out if x is not None]

    for kw in (dict(temperature=1.3, top_k=20, top_p=0.5, prev_ids=[5, 5, V - 1, 3], repetition_penalty=1.2), dict(greedy=True, prev_ids=[5, 5, V - 1, 3], repetition_penalty=1.2)):
        first = bits(model.sample_constrained_op(lg, cons, steps, r=r, top_n=8, return_scores=True, **kw))
        for _ in range(19):
            again = bits(model.sample_constrained_op(lg, cons, steps, r=r, top_n=8, return_scores=True, **kw))
            assert all(torch.equal(a, b) for a, b in zip(again, first))
        alone = bits(model.sample_constrained_op(lg[3:4], cons[3:4], steps[3:4], r=[r[3]], top_n=8, return_scores=True, **kw))
        assert all(torch.equal(a, b[3:4]) for a, b in zip(alone, first))


def test_row_without_a_score_is_an_error(model):
    V = 8
    lg = torch.full((3, V), -float('inf'))
    lg[:, 2] = 1.0
    lg[0, 5] = 0.5
    cons = [CS.OFF, CS.merge(V, suppress_tokens=[2]), CS.OFF]          # row 1: its one finite logit is suppressed, the raw logits hold -inf themselves
    for kw in (dict(greedy=True), dict(temperature=0.8, top_k=3, top_p=0.9), dict()):
        with pytest.raises(ValueError):
            model.sample_constrained_op(lg, cons, 0, **kw)
        ok = model.sample_constrained_op(lg, [CS.OFF, CS.merge(V, suppress_tokens=[3]), CS.OFF], 0, **kw)[0].cpu().tolist()
        assert ok[1] == 2 and ok[2] == 2
    sup = CS.merge(model.config.vocab_size, sequence_bias={(7,): -float('inf')})
    model.set_generate_constraints(sup)
    assert model.set_generate_constraints(None) == sup          # set, read back, cleared


def test_limits_are_checked_when_set(model):
    V = model.config.vocab_size
    import ctypes as C
    from mmduet_amd._lib import lib

    def native(eos, min_new, ids, bias):
        return lib().mmd_set_generate_constraints(model._ctx, (C.c_int64 * max(1, len(eos)))(*eos), len(eos), min_new, (C.c_int32 * max(1, len(ids)))(*ids),
                                                  (C.c_float * max(1, len(bias)))(*bias), len(ids))
    assert native([1], 0, [], []) == 0 and native([], 0, [], []) == 0
    assert native(list(range(9)), 0, [], []) == -22                                         # 9 EOS ids
    assert native([], 0, list(range(257)), [0.5] * 257) == -22                              # 257 entries
    assert native([], 0, [3], [float('nan')]) == -22 and native([], 0, [3], [float('inf')]) == -22
    assert native([], 0, [3, 3], [1.0, 2.0]) == -22 and native([], 0, [V], [1.0]) == -22 and native([V], 0, [], []) == -22 and native([], -1, [], []) == -22
    assert native([], 0, [3], [-float('inf')]) == 0 and native([], 0, [], []) == 0
    small = 8
    lg = torch.zeros(1, small)
    with pytest.raises(MmduetError):          # suppressed + EOS cover the vocabulary: refused when the set is given (the Python merge is bypassed)
        model.sample_constrained_op(lg, CS.Constraints((7,), 0, tuple(range(7)), (-float('inf'),) * 7), 0, greedy=True)
    for bad in (CS.Constraints((), 0, (1,), (float('nan'),)), CS.Constraints((), 0, (1,), (float('inf'),)), CS.Constraints(tuple(range(8)) + (0,), 0, (), ())):
        with pytest.raises((MmduetError, ValueError)):
            model.sample_constrained_op(lg, bad, 0, greedy=True)
    with pytest.raises(MmduetError):
        model.sample_constrained_op(torch.zeros(1, 1000), CS.Constraints((), 0, tuple(range(257)), (0.5,) * 257), 0, greedy=True)
    for kw in (dict(eos_token_id=list(range(9))), dict(suppress_tokens=list(range(257))), dict(sequence_bias={(1,): float('nan')})):
        with pytest.raises(ValueError):
            model.set_generate_constraints(**kw)
    assert model._constraints is None


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------------------
def prompt():
    return torch.from_numpy(load_npz('cfgA_ops.npz')['step0_in'])[None].cuda()


def gen(m, x, do_sample, pen, n_new=12, **kw):
    kw.setdefault('eos_token_id', -1)
    return m.generate(inputs_embeds=x, do_sample=do_sample, max_new_tokens=n_new, repetition_penalty=pen, seed=7, return_dict_in_generate=True, output_logprobs=True, top_logprobs=3,
                      **(SAMPLING if do_sample else {}), **kw)


def check_steps(m, x, out, cons, do_sample, pen):
    """Every step of a constrained response against the oracle on logits replayed through single-row calls (the pattern of test_generate_end_to_end_fp32), within DELTA_E2E."""
    ids = out.sequences[0].tolist()
    logits = replay_rows(m, x, ids)
    lp, slp = out.logprobs[0].double().numpy(), out.sampling_logprobs[0].double().numpy()
    assert np.isfinite(slp).all() and (slp <= 0).all()
    T = SAMPLING['temperature'] if do_sample else 1.0
    for step, tok in enumerate(ids):
        l = logits[step].numpy()
        stopped = [t for t in ids[:step] if t not in cons.eos]
        z = CO.scores(l, cons, step, stopped if pen else None, pen, T)
        assert z[tok] > -np.inf, (step, tok)
        assert abs(lp[step] - LO.logprob(l, tok)) <= DELTA_E2E          # over the raw logits
        if not do_sample:
            assert z[tok] >= z.max() - DELTA_E2E, (step, tok)
            cands = [LO.sampling_logprob(z, np.ones(len(z), bool), tok)]
        else:
            rank, above, keep = SO.analyse(z, SAMPLING['top_k'], SAMPLING['top_p'])
            assert rank[tok] < SAMPLING['top_k'] and above[tok] < SAMPLING['top_p'] + DELTA_E2E, (step, tok)
            u = SO.philox_word(7, step) / 2.0 ** 64
            sets = [keep] + [(above < SAMPLING['top_p'] + d) & (rank < SAMPLING['top_k']) for d in (-DELTA_E2E, DELTA_E2E)]
            ok, cands = False, []
            for kept in sets:
                if kept[tok]:
                    lo, hi, w = SO.draw_interval(z, kept, tok)
                    ok |= w > 0 and lo - DELTA_E2E <= u <= hi + DELTA_E2E
                    cands.append(LO.sampling_logprob(z, kept, tok))
            assert ok, (step, tok)
        assert min(abs(slp[step] - c) for c in cands) <= DELTA_E2E, (step, slp[step], cands)
        # the same logits through the single-row constrained operator: the token it names scores within the tolerance of the returned one
        if not do_sample:
            t1 = int(m.sample_constrained_op(logits[step], cons, step, prev_ids=stopped if pen else None, repetition_penalty=pen, greedy=True)[0])
            assert abs(z[t1] - z[tok]) <= DELTA_E2E


@pytest.mark.parametrize('do_sample,pen', E2E_CASES, ids=E2E_IDS)
def test_generate_end_to_end_fp32(model, do_sample, pen):
    m, x = model, prompt()
    V = m.config.vocab_size
    base = gen(m, x, do_sample, pen)
    ids0 = base.sequences[0].tolist()
    assert len(ids0) == 12
    # two EOS ids, taken from the unconstrained run at steps 3 and 7: the run stops at the first token of the set, which is returned
    eos = [ids0[3], ids0[7]]
    j = next(i for i, t in enumerate(ids0) if t in eos)
    a = gen(m, x, do_sample, pen, eos_token_id=eos)
    ids_a = a.sequences[0].tolist()
    assert ids_a == ids0[:j + 1] and j <= 3
    assert torch.equal(a.logprobs, base.logprobs[:, :j + 1]) and len(a.past_key_values) == x.shape[1] + j          # EOS is not fed back
    check_steps(m, x, a, CS.merge(V, eos), do_sample, pen)
    if pen:          # ... and is not appended to the penalty list (the bare loop grows the caller's list)
        seen = []
        m.set_generate_constraints(eos_token_id=eos)
        try:
            if do_sample:
                got = m.sample_generate(x, None, -1, 12, pen, seen, seed=7, **SAMPLING)[0]
            else:
                got = m.greedy_generate(x, None, -1, 12, pen, seen)[0]
        finally:
            m.set_generate_constraints(None)
        assert got == ids_a and seen == ids_a[:-1]
    # the same EOS set with min_new_tokens = 6: the same ids up to the EOS, another token in its place, at least 6 tokens, no EOS among the first 6
    b = gen(m, x, do_sample, pen, eos_token_id=eos, min_new_tokens=6)
    ids_b = b.sequences[0].tolist()
    assert ids_b[:j] == ids0[:j] and ids_b[j] != ids0[j] and len(ids_b) >= 6 and not set(ids_b[:6]) & set(eos)
    assert all(t not in eos for t in ids_b[:-1])
    check_steps(m, x, b, CS.merge(V, eos, 6), do_sample, pen)
    # an id the unconstrained run emits, suppressed three ways: it never appears
    for kw in (dict(suppress_tokens=[ids0[2]]), dict(bad_words_ids=[[ids0[2]]]), dict(sequence_bias={(ids0[2],): -float('inf')})):
        c = gen(m, x, do_sample, pen, **kw)
        ids_c = c.sequences[0].tolist()
        k = ids0.index(ids0[2])
        assert ids0[2] not in ids_c and ids_c[:k] == ids0[:k] and len(ids_c) == 12
    check_steps(m, x, c, CS.merge(V, suppress_tokens=[ids0[2]]), do_sample, pen)
    # a bias large enough to force one id at every step (list-of-pairs form)
    forced = (ids0[5] + 1) % V
    d = gen(m, x, do_sample, pen, sequence_bias=[[[forced], 1e4]])
    assert d.sequences[0].tolist() == [forced] * 12
    check_steps(m, x, d, CS.merge(V, sequence_bias={(forced,): 1e4}), do_sample, pen)
    # set, then cleared: the ids and records of a model that never set anything
    assert m._constraints is None
    again = gen(m, x, do_sample, pen)
    fresh = gen(hip_model('A', torch.float32)[0], x, do_sample, pen)
    for o in (again, base):
        assert torch.equal(o.sequences, fresh.sequences)
        for f in ('logprobs', 'sampling_logprobs', 'top_logprobs'):
            assert torch.equal(getattr(o, f).view(torch.int32), getattr(fresh, f).view(torch.int32))
        assert torch.equal(o.top_logprob_ids, fresh.top_logprob_ids)


# ---- rounds -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_round_multi_mixes_constrained_and_plain_samplers(model):
    m = model
    H, V = m.config.hidden_size, m.config.vocab_size
    g = torch.Generator().manual_seed(21)
    xs = [torch.randn(n, H, generator=g).cuda() * 0.3 for n in (9, 5, 7)]
    n_new = 8
    sampling = [None, None, dict(temperature=0.8, top_k=20, top_p=0.9, seed=11)]
    pens = [1.15, 1.15, None]

    def rounds(cons):
        smps = [m.new_sampler() for _ in xs]
        for s, sm, pen, cs in zip(smps, sampling, pens, cons):
            s.begin(-1, pen, [3, 4], n_new, sampling=sm, constraints=cs)
        eos = [set(cs.eos) if cs is not None else set() for cs in cons]
        out = m.round_multi([dict(x=x, cache=None, sampler=s, sample=True) for x, s in zip(xs, smps)])
        ids = [[o['token']] for o in out]
        live = [i for i in range(3) if ids[i][-1] not in eos[i]]
        caches = [o['cache'] for o in out]
        while live and min(len(ids[i]) for i in live) < n_new:
            live = [i for i in live if len(ids[i]) < n_new]
            out = m.round_multi([dict(x=None, cache=caches[i], sampler=smps[i], feed=True, sample=True) for i in live])
            for i, o in zip(live, out):
                ids[i].append(o['token'])
                caches[i] = o['cache']
            live = [i for i in live if ids[i][-1] not in eos[i]]
        return ids, smps

    plain, _ = rounds([None, None, None])
    cons = [None,
            CS.merge(V, [plain[1][1], plain[1][4]], 3, [plain[1][0]], sequence_bias={(plain[1][2],): -1.0}),
            CS.merge(V, [plain[2][1], plain[2][4]], 4, [plain[2][0]])]
    ids, smps = rounds(cons)
    assert ids[0] == plain[0]
    assert plain[1][0] not in ids[1] and plain[2][0] not in ids[2] and len(ids[1]) >= 3 and len(ids[2]) >= 4
    # each stream alone through the single-stream loop
    assert m.greedy_generate(xs[0], None, -1, n_new, pens[0], [3, 4])[0] == ids[0]
    for i in (1, 2):
        m.set_generate_constraints(cons[i])
        try:
            if sampling[i] is None:
                alone = m.greedy_generate(xs[i], None, -1, n_new, pens[i], [3, 4])[0]
            else:
                alone = m.sample_generate(xs[i], None, -1, n_new, pens[i], [3, 4], lane=smps[i].lane, **sampling[i])[0]
        finally:
            m.set_generate_constraints(None)
        assert alone == ids[i], (i, alone, ids[i])
    # a sampler whose constraints are cleared decodes as one that never had any
    smps[1].begin(-1, pens[1], [3, 4], n_new, constraints=None)
    out = m.round_multi([dict(x=xs[1], cache=None, sampler=smps[1], sample=True)])
    assert out[0]['token'] == plain[1][0]


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_drivers_honour_the_constraints(model):
    from mmduet_amd.inference import LiveInferForBenchmark
    from mmduet_amd.multistream import MultiStreamInfer
    from test_gpu_multistream import _args_for
    meta = stream_cases()
    name = 'prob_keep_pen'
    case = meta['cases'][name]
    d = run_stream_case(LiveInferForBenchmark, model, name, case, meta)
    assert d.min_new_tokens == 0 and d.suppress_tokens == [] and d.response_token_ids == case['generated']          # defaults: the fixture's ids
    blocked, floor = case['generated'][0][0], min(12, min(len(r) for r in case['generated']) + 3)
    assert any(len(r) < floor for r in case['generated'])          # (the floor binds: a response of the fixture is shorter)

    class Constrained(LiveInferForBenchmark):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.min_new_tokens, self.suppress_tokens = floor, [blocked]

    got = run_stream_case(Constrained, model, name, case, meta).response_token_ids
    assert len(got) >= 1 and all(len(r) >= floor for r in got) and all(blocked not in r for r in got)
    assert model._constraints is None
    # the 2-slot scheduler: constraints ride on the per-video args and reach the slot's sampler; a default video beside it keeps the fixture's ids
    tok = tokenizer_for(model.config)
    model.config.eos_token_id = meta['eos_token_id']
    a_cons, a_plain = _args_for(case, 1), _args_for(case, 1)
    a_cons.min_new_tokens, a_cons.suppress_tokens = floor, [blocked]
    videos = [dict(frames=stream_frames(name), conversation=case['conversation'], args=a) for a in (a_cons, a_plain)]
    res = MultiStreamInfer(a_plain, model=model, tokenizer=tok, n_slots=2).run(videos)
    assert res[0]['response_token_ids'] == got
    assert res[1]['response_token_ids'] == case['generated']
