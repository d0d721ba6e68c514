"""Per-token log-probabilities on the device (the log-probability kernels of sample.hip through mmd_op_sample_logprobs, the native generate loop and the stream driver)
against the float64 restatement of the contract in tests/logprob_oracle.py.

Bound on a raw-operator log-probability: 5e-6 + 2^-21 |lp| (logprob_oracle.bound): fp32 exp is good to about 2 ulp (2.4e-7 relative on the mass), fixed-point truncation adds at
most V 2^-40 ~ 1.4e-7, one log, and two subtractions whose rounding scales with |lp|.  Top-n ids are integer work and get no tolerance.
End to end in fp32 the logits are replayed through other launches: DELTA_E2E = 1e-4, the figure tests/test_gpu_sampling.py argues.
End to end in bf16 the tolerance on the logits is measured, not chosen: see test_generate_end_to_end_bf16.

The tiny golden config has head_dim 16, so the decode loop takes its eager route here; the captured step is tested at true width in tests/test_gpu_logprobs_trueshape.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import logprob_oracle as LO
import sampling_oracle as SO
from helpers import hip_model, stream_cases, run_stream_case
from conftest import load_npz
from test_gpu_sampling import PARAMS, words

DELTA_E2E = 1e-4
# bf16 end to end: largest |log_softmax| difference, at the generated ids of the four cases below, between single-row replay calls and one teacher-forced chunk call,
# measured on the parent commit (profiles/r08_logprobs.md): BF16_MEASURED; the tolerance is twice that (the native loop is a third accumulation order of the same class).
# The figure is 0.0: in the tiny bf16 model both replay routes give the same logits bit for bit, so the native loop is held to the same -- no tolerance at all
BF16_MEASURED = 0.0
TOL_BF16 = 2 * BF16_MEASURED
NS, TOPS = (1, 5, 32), (0, 1, 8)
PEN = 1.3
ALL_PARAMS = PARAMS + ('greedy',)
E2E_CASES = [(False, None), (False, 1.15), (True, None), (True, 1.15)]
E2E_IDS = ['greedy', 'greedy-pen', 'sampled', 'sampled-pen']
SAMPLING = dict(temperature=0.8, top_k=20, top_p=0.9)


@pytest.fixture(scope='module')
def model():
    return hip_model('A', torch.float32)[0]


_dev, _lsm = {}, {}


def rows_on_device(family, V):
    if (family, V) not in _dev:
        _dev[(family, V)] = LO.family_rows(family, V).cuda()
    return _dev[(family, V)]


def log_softmax64(family, V):
    """float64 log_softmax of the family's 32 rows (computed once, never written to)."""
    if (family, V) not in _lsm:
        _lsm[(family, V)] = torch.log_softmax(LO.family_rows(family, V).double(), dim=-1).numpy()
    return _lsm[(family, V)]


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    inf = np.isinf(want)
    with np.errstate(invalid='ignore'):          # (-inf against -inf compares equal before the difference is looked at)
        return bool(((got == want) | (~inf & (np.abs(got - want) <= LO.bound(want)))).all())


def kept_lse(z, tau):
    """logsumexp over {z >= tau} per row, float64 (z [n, V], tau [n])."""
    with np.errstate(invalid='ignore', over='ignore'):
        zk = np.where(z >= tau[:, None], z, -np.inf)
        m = zk.max(axis=1)
        return m + np.log(np.where(np.isneginf(zk), 0.0, np.exp(zk - m[:, None])).sum(axis=1))


@pytest.mark.parametrize('params', ALL_PARAMS, ids=lambda p: p if p == 'greedy' else 'T%s-k%s-p%s' % p)
@pytest.mark.parametrize('family', LO.FAMILIES)
@pytest.mark.parametrize('V', LO.VS)
def test_op_logprobs_against_oracle(model, V, family, params):
    greedy = params == 'greedy'
    T, top_k, top_p = (1.0, 0, 1.0) if greedy else params
    top_k = V + 5 if top_k == 'V+5' else top_k
    lsm, lg_host = log_softmax64(family, V), LO.family_rows(family, V).numpy()
    tops = {}
    for n in NS:
        lg, r = rows_on_device(family, V)[:n], words(n, seed=n)
        for prev, pen in ((None, None), ([0, V - 1, 3 % V, 3 % V, 0], PEN)):
            first = None
            for top_n in TOPS:
                toks, info, z, lp, top_ids, top_lp = model.sample_logprob_op(lg, temperature=T, top_k=top_k, top_p=top_p, r=r, prev_ids=prev, repetition_penalty=pen, greedy=greedy,
                                                                             top_n=top_n, return_scores=True)
                rows = np.arange(n)
                if first is None:
                    # logprob: float64 log_softmax of the same fp32 logits at the device's token
                    tk, z64 = toks.cpu().numpy(), z.cpu().numpy().astype(np.float64)
                    assert ((tk >= 0) & (tk < V)).all()
                    # sampling_logprob: the oracle over the device's own scores and threshold (arg-max: nothing filtered, and the token is the first maximum of pen(l))
                    if greedy:
                        assert info is None and (tk == z64.argmax(axis=1)).all()
                        tau = np.full(n, -np.inf)
                    else:
                        assert (info[:, 3] == 0).all()
                        tau = info[:, 0].cpu().numpy().astype(np.float64)
                    first = (toks, info, z, tk, lsm[rows, tk], z64[rows, tk] - kept_lse(z64, tau))
                else:          # (the number of alternatives changes neither the token nor the scores: the oracle's numbers of the first call stand)
                    assert torch.equal(toks, first[0]) and torch.equal(z, first[2]) and (greedy or torch.equal(info, first[1]))
                tk, want_lp, want_slp = first[3:]
                lp = lp.numpy().astype(np.float64)
                assert close(lp[:, 0], want_lp), (lp[:, 0], want_lp)
                assert close(lp[:, 1], want_slp), (lp[:, 1], want_slp)
                if pen is None and (greedy or params == (1.0, 0, 1.0)):
                    assert (lp[:, 1] == lp[:, 0]).all()          # T = 1, no penalty, no filter: z is l, the same sums, the same bits
                if family == 'equal':
                    assert close(lp[:, 0], np.full(n, -np.log(V)))
                if V == 1:
                    assert (lp == 0).all()
                # the alternatives: ids exactly the oracle's order, values within the bound, padding beyond V
                assert tuple(top_ids.shape) == tuple(top_lp.shape) == (n, top_n)
                for i in range(n):
                    if (i, top_n) not in tops:
                        tops[(i, top_n)] = LO.top_order(lg_host[i], top_n)
                    o = tops[(i, top_n)]
                    assert top_ids[i, :len(o)].tolist() == o.tolist(), (i, top_ids[i], o)
                    assert close(top_lp[i, :len(o)].numpy(), lsm[i, o])
                    assert (top_ids[i, len(o):] == -1).all() and torch.isneginf(top_lp[i, len(o):]).all()


def test_determinism_and_batch_independence(model):
    V, n = 152064, 32
    lg = rows_on_device('randn4', V)
    r = words(n, seed=99)

    def same(a, b, rows=slice(None)):
        return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y[rows].view(torch.int32) if y.dtype == torch.float32 else y[rows]) for x, y in zip(a, b))

    for kw in (dict(temperature=1.3, top_k=20, top_p=0.5, prev_ids=[5, 5, V - 1], repetition_penalty=1.2), dict(temperature=0.9), dict(greedy=True, prev_ids=[5, 5, V - 1], repetition_penalty=1.2)):
        first = model.sample_logprob_op(lg, r=r, top_n=8, **kw)
        first = (first[0].cpu(),) + first[3:]
        for _ in range(19 if 'top_k' in kw else 1):
            again = model.sample_logprob_op(lg, r=r, top_n=8, **kw)
            assert same((again[0].cpu(),) + again[3:], first)
        alone = model.sample_logprob_op(lg[3:4], r=[r[3]], top_n=8, **kw)
        assert same((alone[0].cpu(),) + alone[3:], first, slice(3, 4))


def test_nan_rows_and_argument_checks(model):
    lg = LO.family_rows('randn', 1000)[:5].clone()
    lg[2, 417] = float('nan')
    for kw in (dict(), dict(top_k=5, top_p=0.8), dict(greedy=True)):
        toks, info, _, lp, top_ids, top_lp = model.sample_logprob_op(lg, r=words(5, 3), top_n=2, **kw)
        assert torch.isnan(lp[2]).all() and torch.isnan(top_lp[2]).all()
        assert torch.isfinite(lp[[0, 1, 3, 4]]).all() and torch.isfinite(top_lp[[0, 1, 3, 4]]).all()
        toks = toks.cpu()
        assert toks[2] == -1 and (toks[[0, 1, 3, 4]] >= 0).all()          # the arg-max too: no index is made up for a row with a NaN
    with pytest.raises(Exception):
        model.sample_logprob_op(lg, top_n=9)
    with pytest.raises(Exception):
        model.set_generate_logprobs(9)
    model.set_generate_logprobs(-1)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------------------
def prompt():
    return torch.from_numpy(load_npz('cfgA_ops.npz')['step0_in'])[None].cuda()


def generate_pair(m, x, do_sample, pen, n_new=12, eos=-1, top=3):
    kw = dict(inputs_embeds=x, do_sample=do_sample, max_new_tokens=n_new, eos_token_id=eos, repetition_penalty=pen, seed=7, **(SAMPLING if do_sample else {}))
    plain = m.generate(**kw)
    assert m.last_generate_logprobs() is None
    out = m.generate(return_dict_in_generate=True, output_logprobs=True, top_logprobs=top, **kw)
    assert torch.equal(out.sequences, plain)          # recording changes no id
    n = plain.shape[1]
    assert tuple(out.logprobs.shape) == tuple(out.sampling_logprobs.shape) == (1, n) and tuple(out.top_logprobs.shape) == tuple(out.top_logprob_ids.shape) == (1, n, top)
    assert out.logprobs.dtype == out.sampling_logprobs.dtype == out.top_logprobs.dtype == torch.float32 and out.top_logprob_ids.dtype == torch.long
    rec = m.last_generate_logprobs()
    assert torch.equal(rec['logprobs'], out.logprobs[0]) and torch.equal(rec['top_logprob_ids'], out.top_logprob_ids[0])
    assert m.generate(**kw).equal(plain) and m.last_generate_logprobs() is None          # and it is off again afterwards
    return out


def replay_rows(m, x, ids):
    """The logits of every step through plain single-row model calls on a fresh cache: fp32 [n, V] (CPU)."""
    out = m(inputs_embeds=x)
    rows = []
    for tok in ids:
        rows.append(out.logits[0, -1].float().cpu())
        out = m(inputs_embeds=m.get_input_embeddings()(torch.tensor([[tok]], device=m.device)).view(1, 1, -1), past_key_values=out.past_key_values)
    return torch.stack(rows)


def chunk_hidden(m, x, ids):
    """The hidden rows of every step from ONE teacher-forced call over the prompt and the generated tokens: [n, hidden]."""
    S = x.shape[1]
    fed = m.get_input_embeddings()(torch.tensor([ids[:-1]], device=m.device)).view(1, len(ids) - 1, -1)
    return m(inputs_embeds=torch.cat([x.to(fed.dtype), fed], dim=1))._hidden[S - 1:]


def check_records(out, logits, ids, do_sample, pen, tol, top=3):
    """Every record against the oracle on replayed logits.  A token at the edge of the kept set within the tolerance may be in or out (as in test_gpu_sampling._replay_check)."""
    lp, slp = out.logprobs[0].double().numpy(), out.sampling_logprobs[0].double().numpy()
    tol_of = tol if callable(tol) else (lambda v: tol)          # (a bound that scales with the value: logprob_oracle.bound)
    for step, tok in enumerate(ids):
        tol = float(tol_of(lp[step]))
        l = logits[step].numpy()
        prev = ids[:step] if pen else None
        want_lp, want_slp, _, _ = LO.record(l, tok, prev, pen, greedy=not do_sample, **(SAMPLING if do_sample else {}))
        assert abs(lp[step] - want_lp) <= tol, (step, lp[step], want_lp)
        cands = [want_slp]
        if do_sample:
            z = SO.scores(l, prev, pen, SAMPLING['temperature'])
            rank, above, _ = SO.analyse(z, SAMPLING['top_k'], SAMPLING['top_p'])
            for d in (-tol, tol):
                kept = (above < SAMPLING['top_p'] + d) & (rank < SAMPLING['top_k'])
                if kept[tok]:
                    cands.append(LO.sampling_logprob(z, kept, tok))
        assert min(abs(slp[step] - c) for c in cands) <= tol, (step, slp[step], cands)
        # alternatives: the ids the device names are the oracle's top values (replayed logits may swap near-ties), their logprobs the oracle's at those ids
        dev_ids = out.top_logprob_ids[0, step].tolist()
        want_ids, want_top = LO.top_n(l, top)
        lse = LO.logsumexp(l)
        assert len(set(dev_ids)) == top
        for j, i in enumerate(dev_ids):
            assert abs((l[i] - lse) - want_top[j]) <= tol, (step, j, dev_ids, want_ids)
            assert abs(out.top_logprobs[0, step, j].item() - (l[i] - lse)) <= tol
    assert (lp <= 0).all() and (slp <= 0).all()


@pytest.mark.parametrize('do_sample,pen', E2E_CASES, ids=E2E_IDS)
def test_generate_end_to_end_fp32(model, do_sample, pen):
    m, x = model, prompt()
    out = generate_pair(m, x, do_sample, pen)
    ids = out.sequences[0].tolist()
    assert len(ids) == 12
    check_records(out, replay_rows(m, x, ids), ids, do_sample, pen, DELTA_E2E)
    if pen:
        assert (out.sampling_logprobs != out.logprobs).any()
    elif not do_sample:
        assert torch.equal(out.sampling_logprobs, out.logprobs)
    # teacher-forced scoring of the same tokens: per token through token_nll, and the mean through forward(labels=...)
    S = x.shape[1]
    nll = m.token_nll(chunk_hidden(m, x, ids), torch.tensor(ids)).cpu()
    assert (nll + out.logprobs[0]).abs().max().item() <= DELTA_E2E
    labels = torch.full((1, S + 11), -100, dtype=torch.long)
    labels[0, S - 1:] = torch.tensor(ids)
    fed = m.get_input_embeddings()(torch.tensor([ids[:-1]], device=m.device)).view(1, 11, -1)
    scored = m(inputs_embeds=torch.cat([x, fed], dim=1), labels=labels)
    assert abs(float(scored.lm_loss) + out.logprobs.mean().item()) <= DELTA_E2E


def test_generate_eos_empty_and_argument_checks(model):
    m, x = model, prompt()
    ids = m.generate(inputs_embeds=x, max_new_tokens=12, eos_token_id=-1)[0].tolist()
    eos = ids[3]
    j = ids.index(eos)
    out = generate_pair(m, x, False, None, eos=eos)
    assert out.sequences[0].tolist() == ids[:j + 1] and out.logprobs.shape[1] == j + 1          # EOS is a returned token: it has a record
    out = generate_pair(m, x, True, 1.15, eos=m.generate(inputs_embeds=x, max_new_tokens=12, eos_token_id=-1, do_sample=True, seed=7, repetition_penalty=1.15, **SAMPLING)[0, 2].item())
    assert out.logprobs.shape[1] == out.sequences.shape[1] <= 3
    for do_sample in (False, True):
        out = m.generate(inputs_embeds=x, max_new_tokens=0, do_sample=do_sample, return_dict_in_generate=True, output_logprobs=True, top_logprobs=3)
        assert tuple(out.sequences.shape) == tuple(out.logprobs.shape) == tuple(out.sampling_logprobs.shape) == (1, 0)
        assert tuple(out.top_logprobs.shape) == tuple(out.top_logprob_ids.shape) == (1, 0, 3)
    out = m.generate(inputs_embeds=x, max_new_tokens=2, return_dict_in_generate=True)
    assert out.logprobs is None and out.sampling_logprobs is None and out.top_logprobs is None and out.top_logprob_ids is None
    with pytest.raises(ValueError):
        m.generate(inputs_embeds=x, max_new_tokens=2, output_logprobs=True)
    with pytest.raises(NotImplementedError):
        m.generate(inputs_embeds=x, max_new_tokens=2, output_scores=True)          # what was refused by name still is
    # the bare loops: signatures and tuples as they were, the record on the side
    m.set_generate_logprobs(2)
    try:
        got, _ = m.greedy_generate(x, None, -1, 5)
        rec = m.last_generate_logprobs()
        assert got == ids[:5] and tuple(rec['top_logprobs'].shape) == (5, 2) and rec['logprobs'].shape == (5,)
    finally:
        m.set_generate_logprobs(-1)
    m.greedy_generate(x, None, -1, 5)
    assert m.last_generate_logprobs() is None


@pytest.mark.parametrize('do_sample,pen', E2E_CASES, ids=E2E_IDS)
def test_generate_end_to_end_bf16(do_sample, pen):
    """Ids and counts as in fp32.  Values: BF16_MEASURED is the largest |log_softmax| difference at the generated ids of these four cases between single-row replay calls
    and one teacher-forced chunk call, measured on the parent commit: 0.0 in all four -- the tiny bf16 model gives the same logits bit for bit on both routes.  The
    tolerance TOL_BF16 = 2 x 0.0 = 0 is therefore taken literally for what it measures, the logits: the native loop's records must equal, bit for bit, the records of the
    log-probability operator on the replayed logits (same penalty list, same Philox word), token included.  The operator's own arithmetic against float64 is what
    test_op_logprobs_against_oracle bounds (logprob_oracle.bound, the raw operator's bound); the float64 oracle is checked here with that bound and nothing added."""
    m = bf16_model()
    x = prompt()
    out = generate_pair(m, x, do_sample, pen)
    ids = out.sequences[0].tolist()
    assert len(ids) == 12
    logits = replay_rows(m, x, ids)
    for step, tok in enumerate(ids):
        toks, _, _, lp, top_ids, top_lp = m.sample_logprob_op(logits[step], r=[SO.philox_word(7, step)], greedy=not do_sample, prev_ids=ids[:step] if pen else None, repetition_penalty=pen,
                                                               top_n=3, **(SAMPLING if do_sample else {}))
        assert toks.item() == tok
        got = torch.stack([out.logprobs[0, step], out.sampling_logprobs[0, step]])
        assert (got - lp[0]).abs().max().item() <= TOL_BF16, (step, got, lp[0])
        assert torch.equal(out.top_logprob_ids[0, step], top_ids[0]) and (out.top_logprobs[0, step] - top_lp[0]).abs().max().item() <= TOL_BF16
    check_records(out, logits, ids, do_sample, pen, LO.bound)


_bf16 = []


def bf16_model():
    if not _bf16:
        _bf16.append(hip_model('A', torch.bfloat16)[0])
    return _bf16[0]


def test_driver_records_beside_the_ids(model):
    from mmduet_amd.inference import LiveInferForBenchmark
    meta = stream_cases()
    name = 'prob_keep_pen'          # five responses, a penalty list carried across them
    case = meta['cases'][name]

    class WithLogprobs(LiveInferForBenchmark):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.output_logprobs, self.top_logprobs = True, 2

    d = run_stream_case(WithLogprobs, model, name, case, meta)
    assert d.response_token_ids == case['generated']
    assert len(d.response_logprobs) == len(d.response_token_ids)
    differ = False
    for ids, rec in zip(d.response_token_ids, d.response_logprobs):
        assert len(rec['logprobs']) == len(rec['sampling_logprobs']) == len(rec['top']) == len(ids)
        vals = np.array(rec['logprobs'] + rec['sampling_logprobs'])
        assert np.isfinite(vals).all() and (vals <= 0).all()
        assert all(len(t) == 2 and t[0][1] >= t[1][1] for t in rec['top'])
        differ |= rec['logprobs'] != rec['sampling_logprobs']
    assert differ          # the case carries a penalty list
    off = run_stream_case(LiveInferForBenchmark, model, name, case, meta)
    assert off.output_logprobs is False and off.top_logprobs == 0 and off.response_logprobs == [] and off.response_token_ids == case['generated']
    assert model.last_generate_logprobs() is None


def test_driver_refuses_the_multi_stream_proxy(model):
    from mmduet_amd.inference import LiveInferForBenchmark
    from mmduet_amd.multistream import _ModelProxy
    d = LiveInferForBenchmark.__new__(LiveInferForBenchmark)
    d.model, d.output_logprobs, d.top_logprobs = _ModelProxy(model, None, 512), True, 0
    d._added_stream_generation_ids, d._issue_vit_burst = None, lambda: None
    with pytest.raises(NotImplementedError, match='_ModelProxy'):
        d._generate_response()
