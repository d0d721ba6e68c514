"""Temperature / top-k / top-p sampling on the device (sample.hip through mmd_op_sample, mmd_sample_generate, mmd_round_multi) against the float64 restatement of the
contract in tests/sampling_oracle.py.

Tolerance on probability mass: DELTA = 1e-5.  fp32 exp is good to about 2 ulp (2.4e-7 relative), sums of positive terms keep relative error, fixed-point truncation adds
at most V * 2^-40 ~ 1.4e-7: more than 20x margin, and far below any probability a test here tells apart.  Rank is integer arithmetic and gets no tolerance.
End to end the logits are replayed through other launches (accumulation order: ~1e-6 on logits of scale 4, times 1/T), so DELTA_E2E = 1e-4 there.

The tiny golden config has head_dim 16, so its bf16 context does not meet the captured-graph conditions of the decode loop: the graph route of mmd_sample_generate
is tested at true width in tests/test_gpu_trueshape.py (test_sampled_replay_*), not here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import sampling_oracle as SO
from helpers import hip_model, stream_cases, run_stream_case
from conftest import load_npz

DELTA, DELTA_E2E = 1e-5, 1e-4
VS, NS = (152064, 1000, 257, 8, 1), (1, 5, 32)
FAMILIES = ('randn', 'randn4', 'equal', 'spike', 'ties', 'neginf')
PARAMS = ((1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, 0.9), (1.3, 20, 0.5), (1.0, 1, 1.0), (1.0, 'V+5', 1e-6))
CHI_LOGITS = [2.0, 1.0, 0.0, -1.0, -2.0, 0.5, 0.5, -float('inf')]


@pytest.fixture(scope='module')
def model():
    return hip_model('A', torch.float32)[0]


_rows = {}


def family_rows(family, V):
    """32 rows [32, V] fp32 of one input family (built once per module; the tests slice the first n rows and never write to them)."""
    if (family, V) not in _rows:
        g = torch.Generator().manual_seed(VS.index(V) * 16 + FAMILIES.index(family))
        x = torch.randn(32, V, generator=g)
        if family == 'randn4':
            x = x * 4
        elif family == 'equal':
            x = torch.full((32, V), 0.7)
        elif family == 'spike':
            x[torch.arange(32), torch.randint(0, V, (32,), generator=g)] += 80.0
        elif family == 'ties':
            x = torch.round(x * 2)
        elif family == 'neginf':
            x[torch.rand(32, V, generator=g) < 0.1] = -float('inf')
            x[:, V // 2] = 0.25          # (never a row without a finite entry)
        _rows[(family, V)] = x
    return _rows[(family, V)]


def words(n, seed):
    r = [int(v) for v in np.random.default_rng(seed).integers(0, 1 << 64, size=n, dtype=np.uint64)]
    r[0] = 0
    if n > 1:
        r[-1] = (1 << 64) - 1
    return r


def check_row(z, tau, kept_cnt, token, r, top_k, top_p, delta):
    """Checks 2 and 3 of one row: z the device's scores (float64 copy), tau / kept_cnt / token what the device reported for the word r."""
    V = len(z)
    rank, above, _ = SO.analyse(z, top_k, top_p)
    k_on = 0 < top_k < V
    inside = above < top_p - delta if top_p < 1.0 else np.ones(V, bool)
    outside = above > top_p + delta if top_p < 1.0 else np.zeros(V, bool)
    if k_on:
        inside &= rank < top_k
        outside |= rank >= top_k
    assert (z[inside] >= tau).all(), 'a token the contract keeps lies below tau'
    assert (z[outside] < tau).all(), 'a token the contract drops lies at or above tau'
    kept = z >= tau
    assert kept_cnt == int(kept.sum())
    assert kept[token], 'the drawn token is not kept'
    lo, hi, w = SO.draw_interval(z, kept, token)
    u = r / 2.0 ** 64
    assert w > 0, 'a token without mass was drawn'
    assert lo - delta <= u <= hi + delta, (lo, u, hi)


@pytest.mark.parametrize('params', PARAMS, ids=lambda p: 'T%s-k%s-p%s' % p)
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('V', VS)
def test_op_sample_against_oracle(model, V, family, params):
    T, top_k, top_p = params
    top_k = V + 5 if top_k == 'V+5' else top_k
    prev, pen = ([0, V - 1, 3 % V, 3 % V, 0], 1.3) if family != 'equal' else (None, None)          # duplicates, both ends of the row
    for n in NS:
        lg = family_rows(family, V)[:n]
        r = words(n, seed=n)
        toks, info, z_dev = model.sample_op(lg, temperature=T, top_k=top_k, top_p=top_p, r=r, prev_ids=prev, repetition_penalty=pen, return_scores=True)
        toks, info, z_dev = toks.cpu().numpy(), info.cpu().numpy().astype(np.float64), z_dev.cpu()
        # 1: the scores, in torch fp32
        want = lg.clone()
        if prev is not None:
            ids = torch.tensor(sorted(set(prev)))
            want[:, ids] = torch.where(want[:, ids] > 0, want[:, ids] / pen, want[:, ids] * pen)
        torch.testing.assert_close(z_dev, want / T, rtol=1e-6, atol=0)
        z64 = z_dev.numpy().astype(np.float64)
        for i in range(n):
            assert info[i, 3] == 0
            check_row(z64[i], info[i, 0], int(info[i, 1]), int(toks[i]), r[i], top_k, top_p, DELTA)
            # 4: k = 1 on a row with one maximum is arg-max; the all-equal row is uniform in index order
            if params == (1.0, 1, 1.0) and (z64[i] == z64[i].max()).sum() == 1:
                assert toks[i] == int(z64[i].argmax())
            if family == 'equal':
                assert abs(int(toks[i]) - int(r[i] * V >> 64)) <= 1 and int(info[i, 1]) == V


def test_determinism_and_batch_independence(model):
    V, n = 152064, 32
    lg = family_rows('randn4', V).cuda()
    r = words(n, seed=99)
    kw = dict(temperature=1.3, top_k=20, top_p=0.5, prev_ids=[5, 5, V - 1], repetition_penalty=1.2)
    t0, i0, _ = model.sample_op(lg, r=r, **kw)
    for _ in range(19):
        t, i, _ = model.sample_op(lg, r=r, **kw)
        assert torch.equal(t, t0) and torch.equal(i.view(torch.int32), i0.view(torch.int32))
    t3, i3, _ = model.sample_op(lg[3:4], r=[r[3]], **kw)
    assert torch.equal(t3, t0[3:4]) and torch.equal(i3.view(torch.int32), i0[3:4].view(torch.int32))
    # the same with the filters off (another launch sequence)
    a, ia, _ = model.sample_op(lg, r=r, temperature=0.9)
    b, ib, _ = model.sample_op(lg[3:4], r=[r[3]], temperature=0.9)
    assert torch.equal(b, a[3:4]) and torch.equal(ib.view(torch.int32), ia[3:4].view(torch.int32))


@pytest.mark.parametrize('seed', [1, (1 << 40) + 3])
def test_philox_on_the_device(model, seed):
    n, off = 4096, (1 << 32) - 7          # (the offset's high word counts too)
    z = SO.scores(CHI_LOGITS)
    keep = SO.analyse(z)[2]
    want = [SO.draw(z, keep, SO.philox_word(seed, off, lane)) for lane in range(n)]
    excused = [lane for lane, (_, dist) in enumerate(want) if dist <= DELTA]
    assert len(excused) <= 4, excused          # from the oracle alone (about 0.6 expected), before any device output is looked at
    toks, info, _ = model.sample_op(torch.tensor(CHI_LOGITS).repeat(n, 1), seed=seed, offset=off)
    toks = toks.cpu().tolist()
    bad = [lane for lane in range(n) if toks[lane] != want[lane][0] and lane not in excused]
    assert not bad, bad[:8]
    assert 7 not in toks


def test_nan_is_flagged_not_drawn(model, monkeypatch):
    lg = family_rows('randn', 1000)[:5].clone()
    lg[2, 417] = float('nan')
    for kw in (dict(), dict(top_k=5, top_p=0.8)):
        toks, info, _ = model.sample_op(lg, r=words(5, 3), **kw)
        toks, info = toks.cpu(), info.cpu()
        assert toks[2] == -1 and info[2, 3] == 1
        assert (toks[[0, 1, 3, 4]] >= 0).all() and (info[[0, 1, 3, 4], 3] == 0).all()
    # the Python layer turns the native NaN code into ValueError (the native call is replaced: no NaN is pushed through the model)
    from mmduet_amd import _lib
    monkeypatch.setattr(_lib.lib(), 'mmd_sample_generate', lambda *a: _lib.MMD_EDOM, raising=False)
    x = torch.from_numpy(load_npz('cfgA_ops.npz')['step0_in'])[None].cuda()
    with pytest.raises(ValueError):
        model.generate(inputs_embeds=x, do_sample=True, max_new_tokens=3)


def _replay_check(m, x, ids, seed, T, top_k, top_p):
    """Every returned id passes checks 2 and 3 against the oracle on logits replayed through plain model calls on a fresh cache, with the step's Philox word."""
    out = m(inputs_embeds=x)
    for step, tok in enumerate(ids):
        z = SO.scores(out.logits[0, -1].float().cpu().numpy(), temperature=T)
        rank, above, keep = SO.analyse(z, top_k, top_p)
        assert rank[tok] < top_k and above[tok] < top_p + DELTA_E2E, (step, tok)
        u = SO.philox_word(seed, step) / 2.0 ** 64
        sets = [keep, (above < top_p - DELTA_E2E) & (rank < top_k), (above < top_p + DELTA_E2E) & (rank < top_k)]          # (a boundary token within the tolerance may be in or out)
        ok = False
        for kept in sets:
            if kept[tok]:
                lo, hi, w = SO.draw_interval(z, kept, tok)
                ok |= w > 0 and lo - DELTA_E2E <= u <= hi + DELTA_E2E
        assert ok, (step, tok)
        out = m(inputs_embeds=m.get_input_embeddings()(torch.tensor([[tok]], device=m.device)).view(1, 1, -1), past_key_values=out.past_key_values)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_generate_end_to_end(model, dtype):
    from mmduet_amd.modeling_live import fast_greedy_generate
    m = model if dtype == torch.float32 else hip_model('A', torch.bfloat16)[0]
    x = torch.from_numpy(load_npz('cfgA_ops.npz')['step0_in'])[None].cuda()
    kw = dict(inputs_embeds=x, do_sample=True, temperature=0.8, top_k=20, top_p=0.9, max_new_tokens=12, eos_token_id=-1)
    a = m.generate(seed=7, **kw)
    assert a.dtype == torch.long and tuple(a.shape) == (1, 12)
    _replay_check(m, x, a[0].tolist(), 7, 0.8, 20, 0.9)
    assert torch.equal(m.generate(seed=7, **kw), a)
    assert not torch.equal(m.generate(seed=8, **kw), a)
    # greedy through generate == the greedy path; with input_ids the prompt comes first; the dict form carries the cache
    g = m.generate(inputs_embeds=x, do_sample=False, max_new_tokens=12, eos_token_id=-1)
    ref, _, _ = fast_greedy_generate(model=m, inputs_embeds=x, past_key_values=None, eos_token_id=-1, inplace_output_ids=torch.zeros(1, 12, dtype=torch.long, device=m.device))
    assert torch.equal(g, ref)
    ids = torch.from_numpy(load_npz('cfgA_ops.npz')['ids0']).long()
    o = m.generate(input_ids=ids, do_sample=True, seed=3, max_new_tokens=4, eos_token_id=-1, return_dict_in_generate=True)
    assert tuple(o.sequences.shape) == (1, ids.shape[1] + 4) and torch.equal(o.sequences[0, :ids.shape[1]].cpu(), ids[0]) and len(o.past_key_values) == ids.shape[1] + 3
    assert tuple(m.generate_after_embed(ids, None, do_sample=True, seed=3, max_new_tokens=4, eos_token_id=-1).shape) == (1, 4)
    # neither quirk of the greedy proxy: zero new tokens posts nothing, the list grows only under a penalty
    cache = m(inputs_embeds=x).past_key_values
    seen = [1, 2]
    ids0, c0, off = m.sample_generate(x, cache, -1, 0, 1.1, seen, seed=1)
    assert ids0 == [] and c0 is cache and off == 0 and len(cache) == x.shape[1] and seen == [1, 2]
    ids1, _, off = m.sample_generate(x, None, -1, 3, 0.0, seen, seed=1, offset=5)
    assert len(ids1) == 3 and off == 8 and seen == [1, 2]
    ids2, _, _ = m.sample_generate(x, None, -1, 3, 1.1, seen, seed=1)
    assert seen == [1, 2] + ids2


def test_round_multi_mixes_sampling_and_greedy(model):
    m = model
    H = m.config.hidden_size
    g = torch.Generator().manual_seed(21)
    xs = [torch.randn(n, H, generator=g).cuda() * 0.3 for n in (9, 5, 7)]
    n_new = 6
    sampling = [dict(temperature=0.8, top_k=20, top_p=0.9, seed=11), dict(temperature=1.2, top_k=0, top_p=0.8, seed=12), None]
    pens = [1.15, None, 1.15]

    def rounds(sampling):
        smps = [m.new_sampler() for _ in xs]
        for s, sm, pen in zip(smps, sampling, pens):
            s.begin(-1, pen, [3, 4], n_new, sampling=sm)
        out = m.round_multi([dict(x=x, cache=None, sampler=s, sample=True) for x, s in zip(xs, smps)])
        ids = [[o['token']] for o in out]
        for _ in range(n_new - 1):
            out = m.round_multi([dict(x=None, cache=o['cache'], sampler=s, feed=True, sample=True) for o, s in zip(out, smps)])
            for l, o in zip(ids, out):
                l.append(o['token'])
        return ids, smps

    ids, smps = rounds(sampling)
    assert [s.offset for s in smps] == [n_new, n_new, 0] and len({s.lane for s in smps}) == 3
    for x, sm, pen, s, got in zip(xs[:2], sampling, pens, smps, ids):          # alone, through the single-stream loop, on the sampler's lane
        alone, _, _ = m.sample_generate(x, None, -1, n_new, pen, [3, 4], lane=s.lane, **sm)
        if alone != got:          # rule 3's escape only: the first differing token must be one the oracle cannot call
            step = next(i for i in range(n_new) if alone[i] != got[i])
            out = m(inputs_embeds=x[None])
            for t in got[:step]:
                out = m(inputs_embeds=m.get_input_embeddings()(torch.tensor([[t]], device=m.device)).view(1, 1, -1), past_key_values=out.past_key_values)
            z = SO.scores(out.logits[0, -1].float().cpu().numpy(), prev_ids=[3, 4] + got[:step], penalty=pen, temperature=sm['temperature'])
            keep = SO.analyse(z, sm['top_k'], sm['top_p'])[2]
            assert SO.draw(z, keep, SO.philox_word(sm['seed'], step, s.lane))[1] <= DELTA_E2E, (alone, got)
    greedy_alone, _ = m.greedy_generate(xs[2], None, -1, n_new, pens[2], [3, 4])
    assert ids[2] == greedy_alone
    assert rounds([None, None, None])[0][2] == ids[2]


def test_drivers_default_and_sampled(model):
    from mmduet_amd.inference import LiveInferForBenchmark
    meta = stream_cases()
    name = 'prob_keep_pen'          # a case that responds (five responses) and carries a penalty list across them
    case = meta['cases'][name]
    d = run_stream_case(LiveInferForBenchmark, model, name, case, meta)
    assert d.do_sample is False
    assert d.response_token_ids == case['generated']

    def sampled(seed):
        class Sampled(LiveInferForBenchmark):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                self.do_sample, self.temperature, self.top_k, self.top_p, self.sampling_seed = True, 0.9, 30, 0.95, seed
        return run_stream_case(Sampled, model, name, case, meta).response_token_ids

    a = sampled(5)
    assert len(a) >= 1 and all(len(r) >= 1 for r in a)
    assert a == sampled(5)
