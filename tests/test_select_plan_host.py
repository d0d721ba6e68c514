"""The token-selection table (tests/select_regimes.py) against the decisions themselves, without a GPU: select_plan() / generate_plan() / round_blocks() of
mmduet_amd/csrc/select_plan.h are pure host functions, so tests/select_plan_shim.cpp is compiled with the host C++ compiler into a temporary directory, loaded with ctypes,
and asked about every row.  Then the refusals with their messages, that every field moves somewhere in the table, and that no switch acts outside its fields."""
import ctypes as C
import os
import shutil
import subprocess
import pytest

import select_regimes as T

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler')
SELECT, GENERATE, ROUND = 0, 1, 2


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('select_plan') / 'select_plan_shim.so')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', os.path.join(HERE, 'select_plan_shim.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.select_shim_field_name.restype = C.c_char_p
    names = {w: [lib.select_shim_field_name(w, i).decode().lower() for i in range(lib.select_shim_fields(w))] for w in (SELECT, GENERATE, ROUND)}          # the shim's own lists
    assert all(len(set(n)) == len(n) > 0 for n in names.values())
    assert [lib.select_shim_outputs(w) for w in (SELECT, GENERATE, ROUND)] == [len(T.SELECT_FIELDS), len(T.GENERATE_FIELDS), len(T.ROUND_FIELDS)]
    assert lib.select_shim_round_max() == T.ROUND_MAX

    def ints(which, a):
        a = {k.lower(): v for k, v in a.items() if k != 'top_p'}
        assert set(a) == set(names[which]), set(a) ^ set(names[which])
        return [int(a[f]) for f in names[which]]

    class Ask:
        @staticmethod
        def select(**a):
            out, err = (C.c_int * (1 + len(T.SELECT_FIELDS)))(), C.create_string_buffer(128)
            lib.select_plan_shim((C.c_longlong * len(names[SELECT]))(*ints(SELECT, a)), C.c_double(a['top_p']), out, err, len(err))
            return out[0], tuple(out[1:]), err.value.decode()

        @staticmethod
        def generate(**a):
            a = dict(a)
            a.update(a.pop('gate'))
            out = (C.c_int * len(T.GENERATE_FIELDS))()
            lib.generate_plan_shim((C.c_longlong * len(names[GENERATE]))(*ints(GENERATE, a)), C.c_double(a['top_p']), out)
            return tuple(out)

        @staticmethod
        def round(segs, V):
            """-> (rc, ROUND_FIELDS, order, the three blocks' SelectPlans, message)"""
            keys = ('feed', 'sample', 'sampling', 'constrained', 'rows', 'sampler', 'top_k', 'top_p')
            flat = [v for s in segs for v in ints(ROUND, dict(zip(keys, s)))]
            n, ns = len(segs), len(T.SELECT_FIELDS)
            out, order, plans, err = (C.c_int * (1 + len(T.ROUND_FIELDS)))(), (C.c_int * T.ROUND_MAX)(), (C.c_int * (3 * ns))(), C.create_string_buffer(128)
            lib.round_blocks_shim((C.c_longlong * max(1, len(flat)))(*flat), (C.c_double * max(1, n))(*[s[7] for s in segs]), n, V, out, order, plans, err, len(err))
            return out[0], tuple(out[1:]), tuple(order[:out[3]]) if out[0] == 0 else None, [tuple(plans[k * ns:(k + 1) * ns]) for k in range(3)], err.value.decode()
    return Ask


def test_the_table_covers_the_cross_and_every_field_moves():
    for rows in (T.SELECT_ROWS, T.GENERATE_ROWS, T.ROUND_ROWS):
        assert len({r.name for r in rows}) == len(rows)
    crossed = {(r.inputs['sampled'], r.inputs['constrained'], r.inputs['record'], r.inputs['single'], r.inputs['dyn']) for r in T.SELECT_ROWS}
    assert len({x for x in crossed if x[3:] in ((1, 0), (1, 1), (0, 0))}) == 24
    for fields, plans in ((T.SELECT_FIELDS, [r.plan for r in T.SELECT_ROWS if r.plan]), (T.GENERATE_FIELDS, [r.plan for r in T.GENERATE_ROWS]),
                          (T.ROUND_FIELDS, [r.plan for r in T.ROUND_ROWS if r.plan])):
        for i, f in enumerate(fields):
            assert len({p[i] for p in plans}) > 1, f          # every field takes more than one value
    assert {r.plan[0] for r in T.SELECT_ROWS if r.plan} == {T.ARGMAX, T.CONS_ARGMAX, T.DRAW}
    assert {k for r in T.GENERATE_ROWS for k, v in r.inputs['gate'].items() if v != T.OPEN_GATE[k]} == set(T.OPEN_GATE)          # every gate input closes it in some row
    assert {r.select for r in T.GENERATE_ROWS} <= set(T.by_name(T.SELECT_ROWS))


@pytest.mark.parametrize('row', T.SELECT_ROWS, ids=[r.name for r in T.SELECT_ROWS])
def test_select_plan_of_every_row(shim, row):
    rc, p, err = shim.select(**row.inputs)
    if row.refusal:
        assert (rc, err) == row.refusal, row.name
    else:
        assert (rc, err) == (T.MMD_OK, ''), (row.name, rc, err)
        assert p == row.plan, (row.name, dict(zip(T.SELECT_FIELDS, p)))


@pytest.mark.parametrize('row', T.GENERATE_ROWS, ids=[r.name for r in T.GENERATE_ROWS])
def test_generate_plan_of_every_row(shim, row):
    p = shim.generate(**row.inputs)
    assert p == row.plan, (row.name, dict(zip(T.GENERATE_FIELDS, p)))
    assert bool(p[0]) == row.select.startswith('dyn_')          # the steps' selection is planned as captured exactly when the call replays a captured step


def test_generate_plans_written_out(shim):
    """five rows by hand, so that the table's own restatement of the old conditions is checked too: (can_graph, upload_state, post_row_dynamic,
    post_row_each_eager_step, post_cons_dynamic, post_cons_each_eager_step, host_appends_penalty, pen_key_is_value, key_sel, key_lp, key_cons_gen)"""
    R = T.by_name(T.GENERATE_ROWS)
    assert R['fp32_argmax_pen_more'].plan == (0, 0, 0, 0, 0, 0, 1, 1, 0, -1, 0)                 # the plain eager loop: the host grows the list, nothing is posted
    assert R['fp32_argmax_cons_lp_pen_more'].plan == (0, 0, 0, 1, 0, 1, 1, 1, 0, 2, 1)          # eager arg-max: both descriptors before every step
    assert R['fp32_draw_cons_lp_pen_more'].plan == (0, 1, 1, 0, 1, 0, 0, 0, 0, 2, 1)            # eager draw: device state, both descriptors once, the device grows the list
    assert R['graph_argmax_cons_lp_pen_more'].plan == (1, 1, 1, 0, 1, 0, 0, 1, 0, 2, 1)
    assert R['graph_draw_pen_eos'].plan == (0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0)                   # the first token ended the response: nothing follows
    assert R['graph_draw_pen_one'].plan == R['graph_draw_pen_eos'].plan
    assert R['key_sel_kp'].plan[8] == 3 and R['key_sel_k'].plan[8] == 1 and R['key_sel_p'].plan[8] == 2
    for r in T.GENERATE_ROWS:
        assert shim.generate(**r.inputs) == r.plan, r.name


@pytest.mark.parametrize('row', T.ROUND_ROWS, ids=[r.name for r in T.ROUND_ROWS])
def test_round_blocks_of_every_row(shim, row):
    rc, p, order, plans, err = shim.round(row.segs, row.V)
    if row.refusal:
        assert (rc, err) == row.refusal, row.name
        return
    assert (rc, err) == (T.MMD_OK, ''), (row.name, rc, err)
    assert p == row.plan and order == row.order, (row.name, dict(zip(T.ROUND_FIELDS, p)), order)
    # the blocks' launches: block rows, not a generate step; the sampled block carries the filters any row needs and takes constraint descriptors when any sampled row has a set
    S = T.by_name(T.SELECT_ROWS)
    n_plain, n_greedy, n_sample, any_k, any_p, any_cons = p
    assert plans[T.ARGMAX] == S['block_argmax'].plan and plans[T.CONS_ARGMAX] == S['block_argmax_cons'].plan
    want = list(S['block_draw_cons' if any_cons else 'block_draw'].plan)
    want[T.SELECT_FIELDS.index('any_k')], want[T.SELECT_FIELDS.index('any_p')] = any_k, any_p
    assert plans[T.DRAW] == tuple(want)


def test_a_switch_acts_on_its_fields_alone(shim):
    """over every route: each of sampled / constrained / record changes its own fields in at least one row and no other field in any.  sampled: the kind, and with it whether
    an arg-max's record needs scores of its own, whose sampling_logprob the record takes, whether a row descriptor exists at all, and the advance of an eager step.
    constrained: the kind of an arg-max, the descriptors, and again the scores behind a plain arg-max.  record: the record's own three fields and the row descriptor."""
    own = {'sampled': {'kind', 'needs_row', 'scores_after_argmax', 'record_greedy', 'advance'},
           'constrained': {'kind', 'needs_row', 'needs_cons', 'scores_after_argmax'},
           'record': {'record', 'needs_row', 'scores_after_argmax', 'record_greedy'}}
    base = [r for r in T.SELECT_ROWS if r.name.split('_')[0] in T.ROUTES]
    assert len(base) == 24
    for switch, fields in own.items():
        acted = set()
        for r in base:
            if r.inputs[switch]:
                continue
            a, b = shim.select(**r.inputs)[1], shim.select(**dict(r.inputs, **{switch: 1}))[1]
            diff = {f for f, x, y in zip(T.SELECT_FIELDS, a, b) if x != y}
            assert diff <= fields, (switch, r.name, diff)
            acted |= diff
        assert acted == fields, (switch, fields - acted)
    # the route acts on `single` and `advance` alone
    S = T.by_name(T.SELECT_ROWS)
    for r in base:
        if r.name.startswith('eager_'):
            for other in ('dyn_', 'block_'):
                diff = {f for f, x, y in zip(T.SELECT_FIELDS, r.plan, S[other + r.name[len('eager_'):]].plan) if x != y}
                assert diff <= {'single', 'advance'}, (r.name, other, diff)
