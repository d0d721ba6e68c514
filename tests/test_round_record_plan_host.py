"""The recording rows of a round against round_blocks() itself, without a GPU: tests/round_record_shim.cpp is compiled with the host C++ compiler into a temporary
directory, loaded with ctypes, and asked about every row of tests/round_record_regimes.py.  First: with RoundSeg's recording fields at their defaults, every row of
select_regimes.ROUND_ROWS gives what it gives through tests/select_plan_shim.cpp -- the round without records is the round it was."""
import ctypes as C
import os
import shutil
import subprocess
import pytest

import select_regimes as T
import round_record_regimes as R

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler')
KEYS = ('feed', 'sample', 'sampling', 'constrained', 'rows', 'sampler', 'top_k', 'top_p', 'record', 'lp_top')


@pytest.fixture(scope='module')
def ask(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('round_record') / 'round_record_shim.so')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', os.path.join(HERE, 'round_record_shim.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.record_shim_field_name.restype = C.c_char_p
    names = [lib.record_shim_field_name(i).decode().lower() for i in range(lib.record_shim_fields())]          # the shim's own list
    assert set(names) == set(KEYS) - {'top_p'} and len(names) == len(KEYS) - 1
    assert [lib.record_shim_outputs(w) for w in range(3)] == [len(T.SELECT_FIELDS), len(T.ROUND_FIELDS), len(R.RECORD_FIELDS)]
    assert lib.record_shim_round_max() == T.ROUND_MAX

    def round_(segs, V, defaults=False):
        """-> (rc, ROUND_FIELDS, order, the three blocks' SelectPlans, rec0, RECORD_FIELDS, message)"""
        segs = [tuple(s) + (0, -1) if len(s) == 8 else tuple(s) for s in segs]
        flat = [int(dict(zip(KEYS, s))[f]) for s in segs for f in names]
        n, ns = len(segs), len(T.SELECT_FIELDS)
        out, order, plans = (C.c_int * (1 + len(T.ROUND_FIELDS)))(), (C.c_int * T.ROUND_MAX)(), (C.c_int * (3 * ns))()
        rec0, record, err = (C.c_int * 3)(), (C.c_int * len(R.RECORD_FIELDS))(), C.create_string_buffer(128)
        lib.round_record_shim((C.c_longlong * max(1, len(flat)))(*flat), (C.c_double * max(1, n))(*[s[7] for s in segs]), n, V, int(defaults), out, order, plans, rec0, record,
                              err, len(err))
        ok = out[0] == 0
        return (out[0], tuple(out[1:]), tuple(order[:out[3]]) if ok else None, [tuple(plans[k * ns:(k + 1) * ns]) for k in range(3)], tuple(rec0) if ok else None,
                tuple(record) if ok else None, err.value.decode())
    return round_


def test_the_table_covers_every_kind_in_every_way():
    rows = R.RECORD_ROWS
    assert len({r.name for r in rows}) == len(rows)
    seen = set()
    for r in rows:
        if r.refusal:
            continue
        by_kind = {}
        for s in r.segs:
            if s[1]:
                by_kind.setdefault(T.DRAW if s[2] else T.CONS_ARGMAX if s[3] else T.ARGMAX, []).append(bool(s[8]))
        for kind, rec in by_kind.items():
            interleaved = any(a and not b for a, b in zip(rec, rec[1:]))          # a recording row in front of one that records nothing: the order has to change
            seen.add((kind, 'all' if all(rec) else 'none' if not any(rec) else 'interleaved' if interleaved else 'mixed'))
    assert seen >= {(k, w) for k in (T.ARGMAX, T.CONS_ARGMAX, T.DRAW) for w in ('all', 'none', 'interleaved')}, seen


@pytest.mark.parametrize('row', T.ROUND_ROWS, ids=[r.name for r in T.ROUND_ROWS])
def test_defaults_give_the_round_without_records(ask, row):
    """the new fields left as RoundSeg declares them, and set to their defaults by hand: today's outputs, an empty tail behind every block, nothing recorded"""
    for defaults in (True, False):
        rc, p, order, plans, rec0, record, err = ask(row.segs, row.V, defaults)
        if row.refusal:
            assert (rc, err) == row.refusal, row.name
            continue
        assert (rc, err) == (T.MMD_OK, ''), (row.name, rc, err)
        assert p == row.plan and order == row.order, (row.name, p, order)
        n_plain, n_greedy, n_sample, any_k, any_p, any_cons = p
        assert rec0 == (n_plain, n_greedy, n_sample) and record == (0, 0, 0, -1)
        S = T.by_name(T.SELECT_ROWS)
        assert plans[T.ARGMAX] == S['block_argmax'].plan and plans[T.CONS_ARGMAX] == S['block_argmax_cons'].plan
        want = list(S['block_draw_cons' if any_cons else 'block_draw'].plan)
        want[T.SELECT_FIELDS.index('any_k')], want[T.SELECT_FIELDS.index('any_p')] = any_k, any_p
        assert plans[T.DRAW] == tuple(want)


@pytest.mark.parametrize('row', R.RECORD_ROWS, ids=[r.name for r in R.RECORD_ROWS])
def test_round_blocks_of_every_recording_row(ask, row):
    rc, p, order, plans, rec0, record, err = ask(row.segs, row.V)
    if row.refusal:
        assert (rc, err) == row.refusal, row.name
        return
    assert (rc, err) == (T.MMD_OK, ''), (row.name, rc, err)
    assert p == row.plan and order == row.order, (row.name, dict(zip(T.ROUND_FIELDS, p)), order)
    assert rec0 == row.rec0 and record == row.record, (row.name, rec0, record)
    # the order, from its definition: three blocks; inside each the rows that record nothing, then the recording ones; each group in segment order
    n_plain, n_greedy, n_sample, any_k, any_p, any_cons = p
    ends = (n_plain, n_greedy, n_sample)
    kind_of = lambda s: T.DRAW if s[2] else T.CONS_ARGMAX if s[3] else T.ARGMAX
    for kind, (r0, end) in enumerate(zip((0, n_plain, n_greedy), ends)):
        block = [row.segs[j] for j in order[r0:end]]
        assert all(s[1] and kind_of(s) == kind for s in block)
        quiet, loud = order[r0:rec0[kind]], order[rec0[kind]:end]
        assert r0 <= rec0[kind] <= end and list(quiet) == sorted(quiet) and list(loud) == sorted(loud)
        assert not any(row.segs[j][8] for j in quiet) and all(row.segs[j][8] for j in loud)
        assert record[kind] == len(loud)
    assert sorted(order) == [j for j, s in enumerate(row.segs) if s[1]]
    assert record[3] == max([s[9] for s in row.segs if s[1] and s[8]], default=-1)
    # each block's launches: the table's block plan with or without the record's three fields; the sampled block carries the round's filters
    S = T.by_name(T.SELECT_ROWS)
    for kind in (T.ARGMAX, T.CONS_ARGMAX, T.DRAW):
        want = list(S[row.kinds[kind]].plan)
        if kind == T.DRAW:
            want[T.SELECT_FIELDS.index('any_k')], want[T.SELECT_FIELDS.index('any_p')] = any_k, any_p
        assert plans[kind] == tuple(want), (row.name, kind, dict(zip(T.SELECT_FIELDS, plans[kind])))
        f = dict(zip(T.SELECT_FIELDS, plans[kind]))
        has_tail = record[kind] > 0
        assert f['record'] == has_tail and f['scores_after_argmax'] == (has_tail and kind == T.ARGMAX) and f['record_greedy'] == (has_tail and kind != T.DRAW)


def test_recording_moves_rows_inside_their_block_only(ask):
    """the same segments with and without records: the blocks' sizes, filters and refusals are the same, and a row never leaves its block"""
    for row in R.RECORD_ROWS:
        if row.refusal:
            continue
        quiet = [s[:8] + (0, -1) for s in row.segs]
        a, b = ask(row.segs, row.V), ask(quiet, row.V)
        assert a[0] == b[0] == 0 and a[1] == b[1]
        n_plain, n_greedy, n_sample = a[1][:3]
        for r0, end in ((0, n_plain), (n_plain, n_greedy), (n_greedy, n_sample)):
            assert sorted(a[2][r0:end]) == list(b[2][r0:end])
