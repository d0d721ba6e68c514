"""The state of a response in progress (mmduet_amd/csrc/response_plan.h), one row per case.  Plain data (imports without a GPU): tests/test_response_plan_host.py walks the
rows through the header on the host -- through a ctypes shim, and through a stand-alone program built with the address and undefined-behaviour sanitizers.

CONS rows (name, V, eos, min_new, ids, bias, n_eos, n, null_eos, null_tab, refusal, oracle): the arguments of constraint_set().  n_eos / n default to the lists' lengths and
null_* hand a null pointer in place of a list; refusal is None or (return code, message), the messages transcribed from cons_validate as it stood in model.hip before the
header existed.  oracle: mmduet_amd.constraints.merge can be asked the same question (it takes dicts and lists, so it cannot be handed a duplicate table id, a null pointer
or a negative count; it drops duplicate EOS ids, which the native set keeps as given)."""
import math
from collections import namedtuple

MMD_OK, MMD_EINVAL = 0, -22
MAX_EOS, MAX_TABLE, MAX_TOP = 8, 256, 8
# the four first sizes: the context's penalty list (MODEL_PREV_CAP) and records, a sampler's list and records
CTX_PREV_FIRST, SAMPLER_PREV_FIRST, CTX_RECORDS_FIRST, SAMPLER_RECORDS_FIRST = 16384, 1024, 1024, 256
INF, NAN = math.inf, math.nan

ConsRow = namedtuple('ConsRow', 'name V eos min_new ids bias n_eos n null_eos null_tab refusal oracle')


def cons(name, V, eos=(), min_new=0, table=(), n_eos=None, n=None, null_eos=False, null_tab=False, refusal=None, oracle=True):
    ids, bias = [t[0] for t in table], [float(t[1]) for t in table]
    return ConsRow(name, V, list(eos), min_new, ids, bias, len(eos) if n_eos is None else n_eos, len(ids) if n is None else n, null_eos, null_tab, refusal, oracle)


def refuse(msg):
    return (MMD_EINVAL, msg)


COVER = 'the suppressed ids and the EOS ids cover the whole vocabulary of %d: no token could be returned'
CONS_ROWS = [
    cons('off', 40),
    cons('off_null_pointers', 40, null_eos=True, null_tab=True, oracle=False),
    cons('one_eos', 40, eos=[7]),
    cons('min_new_alone', 40, min_new=3),
    cons('eos_8', 40, eos=range(3, 11)),
    cons('eos_9', 40, eos=range(3, 12), refusal=refuse('at most 8 EOS ids, got 9')),
    cons('table_256', 300, table=[(299 - i, -INF if i % 3 == 0 else 0.25 * (i % 7) - 0.5) for i in range(256)]),          # (descending: the set sorts)
    cons('table_257', 300, table=[(i, 1.0) for i in range(257)], refusal=refuse('at most 256 biased / suppressed ids, got 257')),
    cons('table_unsorted', 40, eos=[2], min_new=1, table=[(9, 1.5), (3, -INF), (30, -2.0), (0, 0.0)]),
    cons('duplicate_table_id', 40, table=[(5, 1.0), (9, 2.0), (5, -INF)], refusal=refuse('table id 5 is listed twice'), oracle=False),
    cons('table_id_V', 40, table=[(3, 1.0), (40, 1.0)], refusal=refuse('table id 40 outside the vocabulary of 40')),
    cons('table_id_minus_1', 40, table=[(-1, 1.0)], refusal=refuse('table id -1 outside the vocabulary of 40')),
    cons('eos_id_V', 40, eos=[3, 40], refusal=refuse('EOS id 40 outside the vocabulary of 40')),
    cons('eos_id_minus_1', 40, eos=[-1], refusal=refuse('EOS id -1 outside the vocabulary of 40')),
    cons('bias_nan', 40, table=[(3, NAN)], refusal=refuse('the bias of id 3 is NaN: finite or -inf only')),
    cons('bias_plus_inf', 40, table=[(2, 1.0), (3, INF)], refusal=refuse('the bias of id 3 is +inf: finite or -inf only')),
    cons('bias_minus_inf', 40, table=[(3, -INF)]),
    cons('min_new_negative', 40, min_new=-1, refusal=refuse('min_new_tokens -1 is negative')),
    cons('duplicate_eos_ids', 40, eos=[7, 9, 7]),
    # suppressed {0, 1, 2, 3} and EOS ids that share id 3 with them: V ids covered, then V - 1
    cons('cover_V', 6, eos=[3, 4, 5], table=[(i, -INF) for i in range(4)], refusal=refuse(COVER % 6)),
    cons('cover_V_minus_1', 6, eos=[3, 4], table=[(i, -INF) for i in range(4)]),
    cons('cover_V_biased_id_is_free', 6, eos=[4, 5], table=[(0, -INF), (1, -INF), (2, -INF), (3, 1.0)]),          # a finite bias suppresses nothing
    cons('cover_V_duplicate_eos', 3, eos=[1, 1, 1], table=[(0, -INF)]),          # two distinct ids of three
    cons('cover_by_eos_alone', 2, eos=[0, 1], refusal=refuse(COVER % 2)),
    cons('negative_count', 40, n=-1, refusal=refuse('bad constraint arguments'), oracle=False),
    cons('null_eos_with_count', 40, n_eos=2, null_eos=True, refusal=refuse('bad constraint arguments'), oracle=False),
    cons('null_table_with_count', 40, n=1, null_tab=True, refusal=refuse('bad constraint arguments'), oracle=False),
    # two rules broken at once: the order of cons_validate decides the message
    cons('eos_9_and_table_257', 300, eos=range(9), table=[(i, 1.0) for i in range(257)], refusal=refuse('at most 8 EOS ids, got 9')),
    cons('eos_id_V_and_duplicate_table_id', 40, eos=[40], table=[(5, 1.0), (5, 2.0)], refusal=refuse('EOS id 40 outside the vocabulary of 40'), oracle=False),
]
# every refusal of cons_validate, once (the bias message counts once for its two spellings)
REFUSALS_ONCE = ('bad constraint arguments', 'at most 8 EOS ids, got 9', 'at most 256 biased / suppressed ids, got 257', 'min_new_tokens -1 is negative',
                 'EOS id 40 outside the vocabulary of 40', 'table id 40 outside the vocabulary of 40', 'the bias of id 3 is NaN: finite or -inf only',
                 'table id 5 is listed twice', COVER % 6)

# ---- the EOS ids of a response: (name, the set's EOS ids, the call's / sampler's own eos_id, V) -> the ids the response stops on ------------------------------------
EOS_ROWS = [
    ('set_given', [5, 9], 3, 40, [5, 9]),          # the set's ids, not the call's
    ('fallback_inside', [], 3, 40, [3]),
    ('fallback_first_id', [], 0, 40, [0]),
    ('fallback_last_id', [], 39, 40, [39]),
    ('fallback_minus_1', [], -1, 40, []),
    ('fallback_V', [], 40, 40, []),
    ('fallback_beyond_V', [], 1 << 40, 40, []),
]
EOS_PROBES = (0, 3, 5, 9, 39)          # tokens asked of response_is_eos under every row

# ---- growth: (cap, need, first) -> capacity ------------------------------------------------------------------------------------------------------------------------
FIRSTS = (CTX_PREV_FIRST, SAMPLER_PREV_FIRST, CTX_RECORDS_FIRST, SAMPLER_RECORDS_FIRST)
GROW_ROWS = ([(1024, 1, 1024, 1024), (1024, 1024, 1024, 1024), (1024, 1025, 1024, 2048), (1024, 9000, 1024, 16384), (256, 257, 1024, 512), (3000, 3001, 256, 6000)]
             + [(0, need, f, want) for f in FIRSTS for need, want in ((0, 0), (1, f), (f, f), (f + 1, 2 * f), (5 * f, 8 * f))])

# ---- the counters: (name, max_new, prev_cap, n_prev at the start, is_eos of each token read) under penalty on / off and records on / off ---------------------------------
NOTE_ROWS = [
    ('eos_first', 12, 64, 3, [1]),
    ('eos_in_the_middle', 12, 64, 3, [0, 0, 0, 1]),
    ('no_eos_up_to_max_new', 5, 64, 3, [0, 0, 0, 0, 0]),
    ('max_new_1', 1, 64, 0, [0]),
    ('rounds_behind_max_new_reach_the_capacity', 2, 6, 3, [0, 0, 0, 0, 0]),          # a sampler sized n_prev + max_new + 1 whose rounds go on: the list stays at 6
]


def note_model(max_new, prev_cap, n_prev, eos_flags, pen, record):
    """the rule of response_note_token: -> [(step, lp_n, n_prev, ended, joins)] after each token"""
    step = lp_n = 0
    ended, out = False, []
    for e in eos_flags:
        step += 1
        lp_n += 1 if record else 0
        joins = bool(pen and not e and n_prev < prev_cap)
        n_prev += 1 if joins else 0
        ended = ended or bool(e) or step >= max_new
        out.append((step, lp_n, n_prev, int(ended), int(joins)))
    return out
