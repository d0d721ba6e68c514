"""How logits rows become tokens (select_plan / generate_plan / round_blocks of mmduet_amd/csrc/select_plan.h), one row per case: the plan it must take, over the full
cross of the three switches -- sampled, constrained, log-probabilities recorded -- on every route, on both sides of every threshold.  Plain data (imports without a GPU):
tests/test_select_plan_host.py asks the three functions about every row on the host, tests/test_gpu_select_regimes.py runs the rows a context reaches on the device and
compares `select_last_plan()`.

SELECT rows (name, inputs, plan, refusal): inputs are the SelectRows fields; plan is what mmd_op_select_last_plan reports first -- SELECT_FIELDS; refusal is None or
(return code, message).  The 24 plans of the cross are written out: they restate, launch by launch, what the prompt step of generate_impl, decode_step_enqueue, the blocks of
mmd_round_multi and the chunk loop of the raw operator launched before select_plan existed.

GENERATE rows (name, inputs, select, plan): inputs are the GenerateShape fields (gate: the GraphGate ones that differ from the open gate of a bf16 true-width context
created with MMDUET_GRAPH=1); select names the SELECT row of the steps behind the first token; plan is GENERATE_FIELDS.  The plans come from `generate_was`, the
conditions of generate_impl as they stood before generate_plan existed, copied term by term; five of them are also written out in the host test.

ROUND rows (name, segs, V, order, plan, refusal): segs are (feed, sample, sampling, constrained, rows, sampler, top_k, top_p); order lists the sampling segments in the
order of their logits rows; plan is ROUND_FIELDS."""
from collections import namedtuple

ARGMAX, CONS_ARGMAX, DRAW = 0, 1, 2
MMD_OK, MMD_EINVAL, MMD_ERANGE = 0, -22, -34
F32, BF16 = 0, 1
SELECT_FIELDS = ('kind', 'single', 'any_k', 'any_p', 'needs_row', 'needs_cons', 'record', 'scores_after_argmax', 'record_greedy', 'advance')
GENERATE_FIELDS = ('can_graph', 'upload_state', 'post_row_dynamic', 'post_row_each_eager_step', 'post_cons_dynamic', 'post_cons_each_eager_step', 'host_appends_penalty',
                   'pen_key_is_value', 'key_sel', 'key_lp', 'key_cons_gen')
ROUND_FIELDS = ('n_plain', 'n_greedy', 'n_sample', 'any_k', 'any_p', 'any_cons_sampled')
V = 2048                        # of the device tests' true-width context
MAX_V = 1 << 18
ROUND_MAX = 32
BELOW_ONE = 1.0 - 2.0 ** -24    # the largest fp32 below 1

SelectRow = namedtuple('SelectRow', 'name inputs plan refusal')
GenerateRow = namedtuple('GenerateRow', 'name inputs select plan')
RoundRow = namedtuple('RoundRow', 'name segs V order plan refusal')


def switches_name(s, c, r):
    return ('draw' if s else 'argmax') + ('_cons' if c else '') + ('_lp' if r else '')


# ---- one block of logits rows ---------------------------------------------------------------------------------------------------------------------
#        sampled, constrained, record: kind         single any_k any_p row cons rec scores_after rec_greedy
CROSS = {(0, 0, 0): (ARGMAX,       None, 0, 0, 0, 0, 0, 0, 0),
         (0, 0, 1): (ARGMAX,       None, 0, 0, 1, 0, 1, 1, 1),          # the unfiltered scores run behind the arg-max, for the record alone
         (0, 1, 0): (CONS_ARGMAX,  None, 0, 0, 1, 1, 0, 0, 0),
         (0, 1, 1): (CONS_ARGMAX,  None, 0, 0, 1, 1, 1, 0, 1),          # the record reads the scores the arg-max was taken from
         (1, 0, 0): (DRAW,         None, 0, 0, 1, 0, 0, 0, 0),
         (1, 0, 1): (DRAW,         None, 0, 0, 1, 0, 1, 0, 0),          # the draw records sampling_logprob itself
         (1, 1, 0): (DRAW,         None, 0, 0, 1, 1, 0, 0, 0),
         (1, 1, 1): (DRAW,         None, 0, 0, 1, 1, 1, 0, 0)}
# advance (launch_advance_state behind a decode step): a sampled step always, an arg-max step only when captured; never behind a block
ROUTES = {'eager': dict(single=1, dyn=0, n=1), 'dyn': dict(single=1, dyn=1, n=1), 'block': dict(single=0, dyn=0, n=8)}
ADVANCE = {'eager': lambda s: s, 'dyn': lambda s: 1, 'block': lambda s: 0}


def _select(name, plan, refusal=None, **inputs):
    a = dict(sampled=0, constrained=0, record=0, n=1, single=0, dyn=0, V=V, top_k=0, top_p=1.0)
    a.update(inputs)
    return SelectRow(name, a, tuple(plan) if plan is not None else None, refusal)


SELECT_ROWS = []
for _route, _kw in ROUTES.items():
    for (_s, _c, _r), _p in CROSS.items():
        SELECT_ROWS.append(_select(f'{_route}_{switches_name(_s, _c, _r)}', (_p[0], _kw['single']) + _p[2:] + (ADVANCE[_route](_s),), sampled=_s, constrained=_c, record=_r, **_kw))
_draw = lambda k, p: (DRAW, 0, k, p, 1, 0, 0, 0, 0, 0)
SELECT_ROWS += [
    _select('top_k_0', _draw(0, 0), sampled=1, n=4, top_k=0),                  # top_k: off | 1 .. V - 1 | V and above keep every entry
    _select('top_k_1', _draw(1, 0), sampled=1, n=4, top_k=1),
    _select('top_k_V-1', _draw(1, 0), sampled=1, n=4, top_k=V - 1),
    _select('top_k_V', _draw(0, 0), sampled=1, n=4, top_k=V),
    _select('top_k_V+1', _draw(0, 0), sampled=1, n=4, top_k=V + 1),
    _select('top_p_1', _draw(0, 0), sampled=1, n=4, top_p=1.0),                # top_p: 1 keeps every entry | just below
    _select('top_p_below_1', _draw(0, 1), sampled=1, n=4, top_p=BELOW_ONE),
    _select('top_k_and_p', _draw(1, 1), sampled=1, n=4, top_k=50, top_p=0.9),
    _select('arg-max_ignores_filters', (ARGMAX, 0, 0, 0, 0, 0, 0, 0, 0, 0), n=4, top_k=50, top_p=0.9),
    # the chain's kernels take vocabularies up to 2^18: each feature on both sides; the plain arg-max has no limit
    _select('V_max_draw', (DRAW, 1, 0, 0, 1, 0, 0, 0, 0, 1), sampled=1, single=1, V=MAX_V),
    _select('V_max_cons', (CONS_ARGMAX, 1, 0, 0, 1, 1, 0, 0, 0, 0), constrained=1, single=1, V=MAX_V),
    _select('V_max_lp', (ARGMAX, 1, 0, 0, 1, 0, 1, 1, 1, 0), record=1, single=1, V=MAX_V),
    _select('V_over_draw', None, (MMD_ERANGE, 'sampling handles vocabularies up to 2^18 entries'), sampled=1, single=1, V=MAX_V + 1),
    _select('V_over_cons', None, (MMD_ERANGE, 'constraints handle vocabularies up to 2^18 entries'), constrained=1, single=1, V=MAX_V + 1),
    _select('V_over_lp', None, (MMD_ERANGE, 'log-probabilities handle vocabularies up to 2^18 entries'), record=1, single=1, V=MAX_V + 1),
    _select('V_over_all', None, (MMD_ERANGE, 'sampling handles vocabularies up to 2^18 entries'), sampled=1, constrained=1, record=1, single=1, V=MAX_V + 1),
    _select('V_over_cons_lp', None, (MMD_ERANGE, 'constraints handle vocabularies up to 2^18 entries'), constrained=1, record=1, single=1, V=MAX_V + 1),
    _select('V_over_argmax', (ARGMAX, 1, 0, 0, 0, 0, 0, 0, 0, 0), single=1, V=MAX_V + 1),
]


# ---- one generate call ------------------------------------------------------------------------------------------------------------------------------
OPEN_GATE = dict(no_graph=0, no_fuse=0, prof_on=0, dtype=BF16, qkv_p=1, H=3584, d=128)
CLOSED_GATES = {'no_graph': dict(no_graph=1), 'no_fuse': dict(no_fuse=1), 'prof_on': dict(prof_on=1), 'fp32': dict(dtype=F32), 'no_packed_qkv': dict(qkv_p=0),
                'H_4097': dict(H=4097), 'd_64': dict(d=64)}
CONTINUATIONS = {'one': dict(max_new=1, first_is_eos=0), 'eos': dict(max_new=4, first_is_eos=1), 'more': dict(max_new=4, first_is_eos=0)}
LP_TOP, CONS_GEN = 2, 1


def generate_was(samp, cons_on, lp_on, pen, max_new, stop, gate_open, any_k=0, any_p=0, lp_top=LP_TOP, cons_gen=CONS_GEN):
    """generate_impl's own conditions before generate_plan existed, term by term (samp / cons_on / lp_on / stop / more / can_graph are its names)"""
    more = (not stop) and max_new > 1
    can_graph = more and gate_open
    eager_loop = more and not can_graph          # the `else` arm of the token loop runs
    return tuple(int(v) for v in (
        can_graph,
        can_graph or (samp and more),                                                            # if (can_graph || (samp && more)) ... hipMemcpyAsync(c->step_dev, ...)
        (samp and more) or ((lp_on or cons_on) and not samp and can_graph),                      # post_row(true) | post_lp_row(true)
        eager_loop and (lp_on or cons_on) and not samp,                                          # post_lp_row(false) in the loop
        cons_on and (can_graph or (samp and more)),                                              # post_cons(true, 1)
        eager_loop and cons_on and not samp,                                                     # post_cons(false, i) in the loop
        eager_loop and pen and not samp,                                                         # if (!samp && !can_graph ...) the host copy behind the list
        not samp,                                                                                # key_pen = pen ? (samp ? 1.f : rep_penalty) : 0.f
        (1 if any_k else 0) | (2 if any_p else 0),
        lp_top if lp_on else -1,
        cons_gen if cons_on else 0))


def _generate(name, s, c, r, pen, cont, gate, gate_open, **sampling):
    a = dict(sampled=s, constrained=c, record=r, pen=pen, V=V, top_k=0, top_p=1.0, lp_top=LP_TOP if r else -1, cons_gen=CONS_GEN if c else 0, **CONTINUATIONS[cont])
    a.update(sampling)
    a['gate'] = dict(OPEN_GATE, **gate)
    any_k, any_p = 0 < a['top_k'] < V, a['top_p'] < 1.0
    plan = generate_was(s, c, r, pen, a['max_new'], a['first_is_eos'], gate_open, any_k, any_p)
    return GenerateRow(name, a, ('dyn_' if plan[0] else 'eager_') + switches_name(s, c, r), plan)


GENERATE_ROWS = []
for (_s, _c, _r) in CROSS:
    for _pen in (0, 1):
        for _cont in CONTINUATIONS:
            for _gname, _gate, _open in (('graph', {}, True), ('fp32', CLOSED_GATES['fp32'], False)):
                GENERATE_ROWS.append(_generate(f'{_gname}_{switches_name(_s, _c, _r)}_{"pen" if _pen else "nopen"}_{_cont}', _s, _c, _r, _pen, _cont, _gate, _open))
GENERATE_ROWS += [_generate(f'gate_{k}', 0, 0, 0, 1, 'more', g, False) for k, g in CLOSED_GATES.items() if k != 'fp32']
GENERATE_ROWS += [_generate('gate_H_4096', 0, 0, 0, 1, 'more', dict(H=4096), True),
                  _generate('key_sel_k', 1, 0, 0, 0, 'more', {}, True, top_k=50), _generate('key_sel_p', 1, 0, 0, 0, 'more', {}, True, top_p=0.9),
                  _generate('key_sel_kp', 1, 0, 0, 0, 'more', {}, True, top_k=50, top_p=0.9)]


def generate_gpu_rows(gate):
    """the cross x penalty at max_new = 4 behind a gate: 'fp32' (eager; first token EOS or not) or 'graph' (captured; more tokens to come)"""
    return [r for r in GENERATE_ROWS if r.name.startswith(gate + '_') and r.inputs['max_new'] == 4 and (gate == 'fp32' or not r.inputs['first_is_eos'])]


# ---- the sampling segments of a round ----------------------------------------------------------------------------------------------------------------
def seg(feed=0, sample=0, sampling=0, constrained=0, rows=1, sampler=-1, top_k=0, top_p=1.0):
    return (feed, sample, sampling, constrained, rows, sampler, top_k, top_p)


PLAIN, CONS, SAMPLED, FEED_ONLY = dict(sample=1), dict(sample=1, constrained=1), dict(sample=1, sampling=1), dict(feed=1)


def _round(name, kinds, order, plan, refusal=None, V=V):
    return RoundRow(name, tuple(seg(**dict(dict(sampler=i), **k)) for i, k in enumerate(kinds)), V, tuple(order) if order is not None else None,
                    tuple(plan) if plan is not None else None, refusal)


MIXED = (SAMPLED, PLAIN, CONS, FEED_ONLY, PLAIN)          # the device test runs this round
ROUND_ROWS = [
    _round('empty', (), (), (0, 0, 0, 0, 0, 0)),
    _round('prompt_only', (dict(rows=3),), (), (0, 0, 0, 0, 0, 0)),
    _round('one_plain', (PLAIN,), (0,), (1, 1, 1, 0, 0, 0)),
    _round('one_cons', (CONS,), (0,), (0, 1, 1, 0, 0, 0)),
    _round('one_sampled', (SAMPLED,), (0,), (0, 0, 1, 0, 0, 0)),
    _round('one_sampled_cons', (dict(SAMPLED, constrained=1, top_k=5),), (0,), (0, 0, 1, 1, 0, 1)),
    _round('one_feed_sample', (dict(PLAIN, feed=1),), (0,), (1, 1, 1, 0, 0, 0)),
    _round('mixed', MIXED, (1, 4, 2, 0), (2, 3, 4, 0, 0, 0)),          # plain 1, 4 | constrained arg-max 2 | sampled 0; segment 3 feeds without sampling
    _round('mixed_filters', (dict(SAMPLED, top_p=0.5), PLAIN, dict(SAMPLED, top_k=V), dict(SAMPLED, constrained=1), CONS, PLAIN), (1, 5, 4, 0, 2, 3), (2, 3, 6, 0, 1, 1)),
    _round('mixed_top_k', (dict(SAMPLED, top_k=V - 1), dict(SAMPLED)), (0, 1), (0, 0, 2, 1, 0, 0)),
    _round('32_sampling', (PLAIN,) * 16 + (SAMPLED,) * 16, tuple(range(32)), (16, 16, 32, 0, 0, 0)),
    _round('33_sampling', (PLAIN,) * 16 + (SAMPLED,) * 17, None, None, (MMD_ERANGE, 'more than 32 sampling segments')),
    _round('33_segments_32_sampling', (PLAIN,) * 16 + (FEED_ONLY,) + (SAMPLED,) * 16, tuple(range(16)) + tuple(range(17, 33)), (16, 16, 32, 0, 0, 0)),
    _round('sampler_twice', (PLAIN, SAMPLED, dict(CONS, sampler=0)), None, None, (MMD_EINVAL, 'a sampler may appear once per round')),
    _round('sampler_feeds_and_samples_apart', (dict(FEED_ONLY, sampler=7), dict(PLAIN, sampler=7)), (1,), (1, 1, 1, 0, 0, 0)),          # once among the SAMPLING segments
    _round('feed_two_rows', (PLAIN, dict(FEED_ONLY, rows=2)), None, None, (MMD_EINVAL, 'a feed segment is one row (segment 1 has 2)')),
]


def by_name(rows):
    return {r.name: r for r in rows}
