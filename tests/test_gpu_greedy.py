"""The kernels of the plain greedy token loop, called directly (mmd_op_argmax, mmd_op_advance_state, mmd_op_embed_feed, mmd_embed_tokens) against tests/greedy_oracle.py.

  arg-max   argmax_penalty_kernel + argmax_final_kernel with the list length in the kernel argument (form 0, the eager steps) and in a device StepState (form 1, the captured
            decode step), argmax_penalty_multi_kernel + argmax_final_multi_kernel with per-row lists, penalties, token slots and append slots (form 2, mmd_round_multi), and
            mmd_op_sample_logprobs(greedy=1) where its one-list-for-all-rows interface can express the rows.  The oracle is fp32 (see its docstring); tokens are integers and
            get no tolerance.  The rows are greedy_oracle.cases(V): families, ties planted across lanes, strides, waves and slices, ties the penalty makes, lists with
            duplicates / foreign ids / every id / 2048 ids, and NaN rows, which every form answers with -1.
  advance   advance_state_kernel against greedy_oracle.advance, the whole list buffer and its guard slots compared.
  embedding embed_kernel and embed_feed_kernel against table[clamp(id, 0, vocab - 1)], bit for bit, in guarded outputs.
  end to end  a model whose lm_head has one NaN row: greedy_generate and a round_multi round with a plain arg-max sampler fail like the sampled route.

Every output sits between guard slots holding a sentinel that is asserted afterwards."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import greedy_oracle as GO
from rawops import RawOps, guarded, sentinel_intact
from helpers import hip_model
from conftest import load_npz, load_golden_weights

SENT = 0x5AA55AA55AA55AA5          # no token id, no list entry
ROWS = 32                          # MMD_ROUND_MAX_SAMPLERS: the most rows of one form-2 launch
EINVAL = -22


@pytest.fixture(scope='module')
def model():
    return hip_model('A', torch.float32)[0]


@pytest.fixture(scope='module')
def ops(model):
    return RawOps.around(model)


def slots(n, dev, before=8, after=64):
    """int64 [before + n + after] of SENT -> (buffer, the [n] view in its middle)"""
    buf = torch.full((before + n + after,), SENT, dtype=torch.long, device=dev)
    return buf, buf[before:before + n]


def guards_intact(buf, n, before=8):
    return bool((buf[:before] == SENT).all()) and bool((buf[before + n:] == SENT).all())


def pack(cases, dev):
    """-> (logits [n, V] on the device, all lists back to back (or None), offsets, penalties)"""
    lg = torch.stack([c.row for c in cases]).to(dev)
    ids, off, pens = [], [0], []
    for c in cases:
        ids += c.prev
        off.append(len(ids))
        pens.append(float(c.penalty) if c.penalty is not None else 0.0)
    prev = torch.tensor(ids, dtype=torch.long, device=dev) if ids else None
    return lg, prev, off, pens


def run_form(ops, form, cases):
    """One mmd_op_argmax call over at most 32 cases, every output guarded: -> tokens as a list.  Form 2: the token slots hold the tokens, the append slots hold them where the
    row's penalty is on and keep the sentinel where it is off."""
    n = len(cases)
    lg, prev, off, pens = pack(cases, ops.dev)
    tb, toks = slots(n, ops.dev)
    sb, tslots = slots(n, ops.dev)
    ab, app = slots(n, ops.dev)
    assert ops.argmax(form, lg, prev, off, pens, toks, tslots if form == 2 else None, app if form == 2 else None) == 0
    assert guards_intact(tb, n) and guards_intact(sb, n) and guards_intact(ab, n)
    out = toks.cpu().tolist()
    if form == 2:
        assert tslots.cpu().tolist() == out
        assert app.cpu().tolist() == [t if p > 0 else SENT for t, p in zip(out, pens)]
    else:
        assert bool((tslots == SENT).all()) and bool((app == SENT).all())
    if prev is not None:
        assert prev.cpu().tolist() == [t for c in cases for t in c.prev]          # the lists are read, never written
    return out


def run_all(ops, form, cases):
    out = []
    for i in range(0, len(cases), ROWS):
        out += run_form(ops, form, cases[i:i + ROWS])
    return out


_want = {}


def oracle_tokens(V):
    """the oracle's token of every case of V, computed once"""
    if V not in _want:
        _want[V] = [GO.pick(c.row.numpy(), c.prev, c.penalty) for c in GO.cases(V)]
    return _want[V]


def split(V, nan):
    cs, want = GO.cases(V), oracle_tokens(V)
    keep = [i for i, c in enumerate(cs) if c.has_nan == nan]
    return [cs[i] for i in keep], [want[i] for i in keep]


def check(cases, got, want, what):
    assert len(cases) == len(got) == len(want) > 0
    bad = [(c.name, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, (what, bad[:8])


@pytest.mark.parametrize('V', GO.VS)
def test_argmax_forms_against_oracle(ops, V):
    """Every row without a NaN, through forms 0, 1 and 2 (32 rows of mixed lists and penalties per form-2 launch): the oracle's token, and so the same token from all three.
    Form 1 passes 0 as the kernel's list length: a kernel that did not read the StepState would apply no penalty and miss the penalised rows."""
    cases, want = split(V, nan=False)
    assert all(0 <= w < V for w in want)
    for form in (0, 1, 2):
        check(cases, run_all(ops, form, cases), want, 'form %d' % form)


@pytest.mark.parametrize('V', GO.VS)
def test_argmax_nan_rows_give_minus_one(ops, V):
    """A NaN at column 0, V - 1, a slice boundary, on a penalised id, beside a +inf, and rows of NaN only: -1 from every form, while the NaN-free rows sharing the form-2
    launch keep their tokens."""
    nan_cases, nan_want = split(V, nan=True)
    assert len(nan_cases) >= 5 and all(w == -1 for w in nan_want)
    clean, clean_want = split(V, nan=False)
    mixed, want = [], []
    for i, (c, w) in enumerate(zip(nan_cases, nan_want)):          # interleaved: every launch of 32 holds both kinds
        mixed += [c, clean[i % len(clean)]]
        want += [w, clean_want[i % len(clean)]]
    for form in (0, 1, 2):
        check(mixed, run_all(ops, form, mixed), want, 'form %d' % form)


@pytest.mark.parametrize('V', GO.VS)
def test_form2_row_alone_and_in_pairs(ops, V):
    """Form 2 with n = 1 and n = 2: a row's token does not depend on what shares its launch."""
    cases, want = GO.cases(V), oracle_tokens(V)
    step = 1 if V <= 4097 else 3          # (the large rows: every third case, the NaN-all and list_2048 rows among them by name)
    pick = [i for i in range(len(cases)) if i % step == 0 or cases[i].name in ('list_2048', 'nan_all', 'list_out_of_range')]
    for i in pick:
        check([cases[i]], run_form(ops, 2, [cases[i]]), [want[i]], 'alone')
    for i in pick[::2]:
        j = (i + 7) % len(cases)
        check([cases[i], cases[j]], run_form(ops, 2, [cases[i], cases[j]]), [want[i], want[j]], 'pair')


@pytest.mark.parametrize('V', GO.VS)
def test_cross_route_with_the_logprob_operator(model, ops, V):
    """NaN-free rows that share one list and penalty (what mmd_op_sample_logprobs can express), ids in range: its greedy token equals forms 0, 1 and 2."""
    cases, want = split(V, nan=False)
    groups = {}
    for c, w in zip(cases, want):
        if all(0 <= t < V for t in c.prev):
            groups.setdefault((tuple(c.prev), c.penalty), []).append((c, w))
    big = sorted(groups.items(), key=lambda kv: -len(kv[1]))[:3]
    assert len(big[0][1]) >= 4
    for (prev, pen), members in big:
        cs, ws = [c for c, _ in members][:ROWS], [w for _, w in members][:ROWS]
        lg = torch.stack([c.row for c in cs]).to(ops.dev)
        toks = model.sample_logprob_op(lg, greedy=True, prev_ids=list(prev) or None, repetition_penalty=pen, top_n=0)[0].cpu().tolist()
        check(cs, toks, ws, 'sample_logprobs')
        for form in (0, 1, 2):
            check(cs, run_form(ops, form, cs), toks, 'form %d against sample_logprobs' % form)


def test_argmax_refusals(ops):
    cases = GO.cases(65)[:3]
    lg, prev, off, pens = pack(cases, ops.dev)
    tb, toks = slots(40, ops.dev)
    sb, ts = slots(40, ops.dev)
    ab, ap = slots(40, ops.dev)
    assert ops.argmax(3, lg, prev, off, pens, toks, ts, ap) == EINVAL and ops.argmax(-1, lg, prev, off, pens, toks, ts, ap) == EINVAL
    assert ops.argmax(2, lg, prev, off, pens, toks, None, ap) == EINVAL and ops.argmax(2, lg, prev, off, pens, toks, ts, None) == EINVAL
    assert ops.argmax(0, lg, prev, off, pens, None) == EINVAL and ops.argmax(0, None, prev, off, pens, toks, n=3, V=65) == EINVAL
    assert ops.argmax(0, lg, prev, [1] + off[1:], pens, toks) == EINVAL          # offsets start at 0
    assert ops.argmax(0, lg, prev, [0, 5, 4, 6], [1.3] * 3, toks) == EINVAL      # and do not decrease
    assert ops.argmax(0, lg, None, [0, 1, 2, 3], [1.3] * 3, toks) == EINVAL      # lists without ids
    assert ops.argmax(0, lg, prev, off, pens, toks, n=0) == EINVAL and ops.argmax(0, lg, prev, off, pens, toks, V=0) == EINVAL
    many = torch.zeros(ROWS + 1, 8, device=ops.dev)
    assert ops.argmax(2, many, None, [0] * (ROWS + 2), [0.0] * (ROWS + 1), toks, ts, ap) == EINVAL          # above the cap of one launch
    assert ops.argmax(0, many, None, [0] * (ROWS + 2), [0.0] * (ROWS + 1), toks) == 0                       # (the per-row forms take them)
    assert toks[:ROWS + 1].cpu().tolist() == [0] * (ROWS + 1)
    for b in (sb, ab):
        assert bool((b == SENT).all())          # nothing refused, and no per-row form, touched the slots
    assert guards_intact(tb, 40) and bool((toks[ROWS + 1:] == SENT).all())


# ---- advance_state_kernel ---------------------------------------------------------------------------------------------------------------------------------------------
CAP = 6
ADVANCE = [          # (token, eos, use_penalty, n_prev before)
    ('plain', 41, 2, 1, 3),
    ('eos', 2, 2, 1, 3),
    ('penalty_off', 41, 2, 0, 3),
    ('full', 41, 2, 1, CAP),
    ('last_slot', 41, 2, 1, CAP - 1),
    ('empty_list', 41, 2, 1, 0),
    ('eos_with_penalty_off', 2, 2, 0, 0),
    ('negative_token', -7, 2, 1, 2),          # (ids are data to this kernel)
    ('wide_token', (1 << 40) + 5, 2, 1, 2),
]


def list_buffer(dev):
    buf, prev = slots(CAP, dev)
    prev.copy_(torch.arange(100, 100 + CAP, device=dev))
    return buf, prev


@pytest.mark.parametrize('case', ADVANCE, ids=lambda c: c[0])
def test_advance_state_against_oracle(ops, case):
    _, tok, eos, use_pen, n_prev = case
    buf, prev = list_buffer(ops.dev)
    before = buf.cpu().tolist()
    s0 = dict(prev=before[8:], n_prev=n_prev, n_ctx=(1 << 33) + 9, step=4)          # (n_ctx is 64 bits wide; the slots behind the list are part of what is compared)
    want = GO.advance(s0, tok, eos, use_pen, CAP)
    rc, a, b, c = ops.advance_state(tok, eos, use_pen, prev, CAP, s0['n_prev'], s0['n_ctx'], s0['step'])
    assert rc == 0 and (a, b, c) == (want['n_prev'], want['n_ctx'], want['step'])
    assert (b, c) == (s0['n_ctx'] + 1, s0['step'] + 1)
    assert buf.cpu().tolist() == before[:8] + want['prev']          # the one appended slot, nothing else: not the list, not the guard behind slot prev_cap - 1
    assert guards_intact(buf, CAP)


def test_advance_state_sequence_and_refusals(ops):
    buf, prev = list_buffer(ops.dev)
    s = dict(prev=buf.cpu().tolist()[8:], n_prev=CAP - 2, n_ctx=500, step=1)
    for tok, eos, use_pen in ((11, 2, 1), (2, 2, 1), (12, 2, 0), (13, 2, 1), (14, 2, 1)):          # append, EOS, penalty off, the last slot, full
        want = GO.advance(s, tok, eos, use_pen, CAP)
        rc, a, b, c = ops.advance_state(tok, eos, use_pen, prev, CAP, s['n_prev'], s['n_ctx'], s['step'])
        assert rc == 0 and (a, b, c) == (want['n_prev'], want['n_ctx'], want['step'])
        assert buf.cpu().tolist()[8:] == want['prev']
        s = want
    assert s['n_prev'] == CAP and s['prev'][CAP - 2:CAP] == [11, 13] and (s['n_ctx'], s['step']) == (505, 6) and guards_intact(buf, CAP)
    before = buf.cpu().tolist()
    assert ops.advance_state(5, 2, 1, prev, CAP, CAP + 1, 0, 0)[0] == EINVAL and ops.advance_state(5, 2, 1, prev, CAP, -1, 0, 0)[0] == EINVAL
    assert ops.advance_state(5, 2, 1, None, CAP, 0, 0, 0)[0] == EINVAL and ops.advance_state(5, 2, 1, prev, -1, 0, 0, 0)[0] == EINVAL
    assert buf.cpu().tolist() == before


# ---- embedding gathers ------------------------------------------------------------------------------------------------------------------------------------------------
INT_MAX = 0x7fffffff
_models = {}


def model_of(dtype, model):
    if dtype == torch.float32:
        return model
    if dtype not in _models:
        _models[dtype] = hip_model('A', dtype)[0]
    return _models[dtype]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_embedding_rows_and_clamp(model, dtype):
    """embed_kernel (mmd_embed_tokens) and embed_feed_kernel (mmd_op_embed_feed): rows bit-equal to table[clamp(id, 0, vocab - 1)] for ids at and far beyond both ends (an id
    cut to 32 bits would land inside the table: 2^40 -> row 0 happens to be right, 2^40 + 5 and -2^40 + 3 are not); feed rows land at scattered rows of a guarded output and
    the rows not listed keep the sentinel."""
    m = model_of(dtype, model)
    o = RawOps.around(m)
    table = load_golden_weights('A')[1]['model.embed_tokens.weight'].to(dtype)
    vocab, H = table.shape
    ids = [0, 1, vocab - 1, vocab, INT_MAX, 1 << 40, -1, -(1 << 40), (1 << 40) + 5, -(1 << 40) + 3, (1 << 32) + 7]
    want = table[torch.tensor(ids).clamp(0, vocab - 1)]
    as_int = torch.int32 if dtype == torch.float32 else torch.int16
    ids_dev = torch.tensor(ids, dtype=torch.long, device=m.device)
    # embed_kernel
    buf, out = guarded(len(ids), H, dtype, m.device)
    m.get_input_embeddings()(ids_dev, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(as_int), want.view(as_int))
    assert sentinel_intact(buf[:16]) and sentinel_intact(buf[16 + len(ids):])
    # embed_feed_kernel: one token slot per row, scattered rows
    rows = [5, 0, 17, 3, 30, 9, 12, 22, 31, 1, 26]
    n_rows = 32
    buf, out = guarded(n_rows, H, dtype, m.device)
    assert o.embed_feed(ids_dev, rows, out) == 0
    got = out.cpu()
    assert torch.equal(got[rows].view(as_int), want.view(as_int))
    rest = [r for r in range(n_rows) if r not in rows]
    assert sentinel_intact(out[rest]) and sentinel_intact(buf[:16]) and sentinel_intact(buf[16 + n_rows:])
    assert ids_dev.cpu().tolist() == ids
    # refusals: before any launch
    assert o.embed_feed(ids_dev, [0, n_rows], out) == EINVAL and o.embed_feed(ids_dev, [-1], out) == EINVAL
    assert o.embed_feed(ids_dev, [], out) == EINVAL and o.embed_feed(torch.zeros(33, dtype=torch.long, device=m.device), list(range(33)), out, out_rows=40) == EINVAL
    assert o.embed_feed(None, [0], out) == EINVAL
    assert torch.equal(out.cpu().view(as_int), got.view(as_int))


# ---- end to end: a NaN logit -------------------------------------------------------------------------------------------------------------------------------------------
NAN_ROW = 200


@pytest.fixture(scope='module')
def nan_model():
    """The tiny fp32 model with ONE lm_head row set to NaN: logit 200 of every step is NaN, nothing non-finite goes through the decoder."""
    w = dict(load_golden_weights('A')[1])
    head = w['lm_head.weight'].clone()
    head[NAN_ROW] = float('nan')
    w['lm_head.weight'] = head
    return hip_model('A', torch.float32, weights=w)[0]


def test_generate_fails_on_nan_like_the_sampled_route(nan_model):
    """greedy_generate on a model whose logits hold a NaN: ValueError (the native MMD_EDOM), no token, and the arena as long as the sampled route leaves it in the same
    situation.  The prompt's own token already fails, so the captured decode step is not reached this way: its arg-max (the list length read from a StepState) is covered by
    form 1 of mmd_op_argmax in test_argmax_nan_rows_give_minus_one."""
    m = nan_model
    x = torch.from_numpy(load_npz('cfgA_ops.npz')['step0_in'])[None].cuda()
    lg = m(inputs_embeds=x).logits[0, -1].float().cpu()
    assert bool(torch.isnan(lg[NAN_ROW])) and int(torch.isnan(lg).sum()) == 1          # the situation is the one meant: one NaN logit, the rest finite
    lengths = {}
    for route in ('greedy', 'greedy_pen', 'sampled'):
        cache = m(inputs_embeds=x).past_key_values
        seen = [3, 4]
        with pytest.raises(ValueError, match='NaN') as err:
            if route == 'sampled':
                m.sample_generate(x, cache, -1, 5, 1.15, seen, temperature=0.8, top_k=20, top_p=0.9, seed=7)
            else:
                m.greedy_generate(x, cache, -1, 5, 1.15 if route == 'greedy_pen' else None, seen)
        assert ('mmd_sample_generate' if route == 'sampled' else 'mmd_greedy_generate') in str(err.value)
        assert seen == [3, 4]
        lengths[route] = cache.arena.length()
    assert lengths['greedy'] == lengths['greedy_pen'] == lengths['sampled'] > x.shape[1]
    with pytest.raises(ValueError, match='NaN'):
        m.generate(inputs_embeds=x, do_sample=False, max_new_tokens=3)


def test_round_with_a_plain_sampler_fails_on_nan(nan_model):
    """One plain arg-max sampler on the NaN model plus a segment that only steps: the round fails with the native MMD_EDOM (ValueError naming mmd_round_multi), and a following
    round without the sampler runs."""
    m = nan_model
    H = m.config.hidden_size
    g = torch.Generator().manual_seed(5)
    x1, x2 = torch.randn(6, H, generator=g).cuda() * 0.3, torch.randn(4, H, generator=g).cuda() * 0.3
    for pen in (None, 1.15):
        s = m.new_sampler()
        s.begin(-1, pen, [3, 4], 4)
        with pytest.raises(ValueError, match='mmd_round_multi.*NaN'):
            m.round_multi([dict(x=x1, cache=None, sampler=s, sample=True), dict(x=x2, cache=None, head_rows=[3])])
        out = m.round_multi([dict(x=x2, cache=None, head_rows=[3])])
        assert out[0]['token'] is None and len(out[0]['cache']) == 4 and bool(torch.isfinite(out[0]['heads']).all())
