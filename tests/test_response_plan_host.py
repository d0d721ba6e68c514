"""The state of a response in progress (tests/response_cases.py) against the rules themselves, without a GPU: mmduet_amd/csrc/response_plan.h is pure host code, so
tests/response_plan_shim.cpp is compiled with the host C++ compiler into a temporary directory, loaded with ctypes and asked about every row.  constraint_set() is held to
mmduet_amd.constraints.merge -- the Python twin whose docstring promises that "the native call checks them again" -- and to the messages of the cons_validate it replaced;
the EOS rule, the doubling rule and the per-token counters to what the table and a ten-line model say.  Then the same table goes through a stand-alone build of the same
file under the address and undefined-behaviour sanitizers, which must answer the same and exit clean."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess
import pytest

import response_cases as T
from mmduet_amd import constraints as CS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'response_plan_shim.cpp')
CXX = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler')
FLAGS = ['-std=c++17', '-O1', '-Wall', '-Werror']


def bits(x):
    return struct.unpack('<I', struct.pack('<f', x))[0]


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('response_plan') / 'response_plan_shim.so')
    subprocess.run([CXX, *FLAGS, '-shared', '-fPIC', SRC, '-o', so], check=True)
    lib = C.CDLL(so)

    class Ask:
        @staticmethod
        def constants():
            out = (C.c_int * 7)()
            lib.response_shim_constants(out)
            return tuple(out)

        @staticmethod
        def cons(row):
            """-> (rc, message, None) or (0, '', dict(on, eos, min_new, table [(id, bias bits)]))"""
            eos = None if row.null_eos else (C.c_int64 * max(1, len(row.eos)))(*row.eos)
            ids = None if row.null_tab else (C.c_int32 * max(1, len(row.ids)))(*row.ids)
            bias = None if row.null_tab else (C.c_float * max(1, len(row.bias)))(*row.bias)
            meta, eo, io, bo, err = (C.c_int * 5)(), (C.c_int64 * T.MAX_EOS)(), (C.c_int32 * T.MAX_TABLE)(), (C.c_float * T.MAX_TABLE)(), C.create_string_buffer(256)
            lib.constraint_set_shim(row.V, eos, row.n_eos, row.min_new, ids, bias, row.n, meta, eo, io, bo, err, len(err))
            rc, on, n, n_eos, min_new = meta
            if rc:
                return rc, err.value.decode(), None
            return rc, err.value.decode(), dict(on=on, eos=list(eo[:n_eos]), min_new=min_new, table=[(io[k], bits(bo[k])) for k in range(n)])

        @staticmethod
        def eos(set_eos, eos_id, V, probes):
            out, stops = (C.c_int64 * T.MAX_EOS)(), (C.c_int * len(probes))()
            n = lib.response_eos_shim((C.c_int64 * max(1, len(set_eos)))(*set_eos), len(set_eos), C.c_int64(eos_id), V, out, (C.c_int64 * len(probes))(*probes), len(probes), stops)
            return list(out[:n]), list(stops)

        grow = staticmethod(lambda cap, need, first: lib.grow_capacity_shim(cap, need, first))

        @staticmethod
        def needs(n_prev, max_new):
            out = (C.c_int * 3)()
            lib.response_needs_shim(n_prev, max_new, out)
            return tuple(out)

        @staticmethod
        def note(max_new, prev_cap, n_prev, eos_flags, pen, record):
            count, out = (C.c_int * 5)(0, 0, n_prev, max_new, 0), []
            for e in eos_flags:
                joins = lib.response_note_shim(count, int(e), int(pen), int(record), prev_cap)
                assert count[3] == max_new
                out.append((count[0], count[1], count[2], count[4], joins))
            return out
    return Ask


def test_the_limits_and_first_sizes_have_one_value(shim):
    assert shim.constants() == (T.MAX_EOS, T.MAX_TABLE, T.MAX_TOP, T.CTX_PREV_FIRST, T.SAMPLER_PREV_FIRST, T.CTX_RECORDS_FIRST, T.SAMPLER_RECORDS_FIRST)
    assert (CS.MAX_EOS, CS.MAX_TABLE) == (T.MAX_EOS, T.MAX_TABLE)


def test_the_table_covers_what_it_promises():
    R = {r.name: r for r in T.CONS_ROWS}
    assert len(R) == len(T.CONS_ROWS)
    said = [r.refusal[1] for r in T.CONS_ROWS if r.refusal]
    for msg in T.REFUSALS_ONCE:
        assert msg in said, msg
    assert len(R['eos_8'].eos) == 8 and len(R['eos_9'].eos) == 9 and len(R['table_256'].ids) == 256 and len(R['table_257'].ids) == 257
    assert {r.name for r in T.CONS_ROWS if not r.oracle} == {'off_null_pointers', 'duplicate_table_id', 'negative_count', 'null_eos_with_count', 'null_table_with_count',
                                                           'eos_id_V_and_duplicate_table_id'}


def merged(row):
    """the row through mmduet_amd.constraints.merge: Constraints, or None when it raises ValueError"""
    try:
        return CS.merge(row.V, eos_token_id=list(row.eos), min_new_tokens=row.min_new, sequence_bias=[[[i], b] for i, b in zip(row.ids, row.bias)])
    except ValueError:
        return None


@pytest.mark.parametrize('row', T.CONS_ROWS, ids=[r.name for r in T.CONS_ROWS])
def test_constraint_set_of_every_row(shim, row):
    rc, err, got = shim.cons(row)
    if row.refusal:
        assert (rc, err) == row.refusal and got is None
    else:
        assert (rc, err) == (T.MMD_OK, '')
        want = sorted(zip(row.ids, row.bias))
        assert got['table'] == [(i, bits(b)) for i, b in want] and got['eos'] == row.eos and got['min_new'] == row.min_new          # sorted by id, nothing else changed
        assert got['on'] == int(bool(row.ids or row.eos or row.min_new > 0))
    if not row.oracle:
        return
    ref = merged(row)
    assert (ref is None) == (row.refusal is not None), (row.name, ref)          # accept / refuse agreement
    if ref is not None:
        assert got['table'] == [(i, bits(b)) for i, b in zip(ref.ids, ref.bias)]
        assert list(dict.fromkeys(got['eos'])) == list(ref.eos) and got['min_new'] == ref.min_new and bool(got['on']) == ref.on


@pytest.mark.parametrize('name,set_eos,eos_id,V,want', T.EOS_ROWS, ids=[r[0] for r in T.EOS_ROWS])
def test_the_eos_ids_of_a_response(shim, name, set_eos, eos_id, V, want):
    ids, stops = shim.eos(set_eos, eos_id, V, T.EOS_PROBES)
    assert ids == want and stops == [int(t in want) for t in T.EOS_PROBES]


def test_grow_capacity(shim):
    for cap, need, first, want in T.GROW_ROWS:
        assert shim.grow(cap, need, first) == want, (cap, need, first)
    # the four first sizes from nothing, and what the two owners ask for
    assert [shim.grow(0, 1, f) for f in T.FIRSTS] == [16384, 1024, 1024, 256]
    assert shim.needs(1020, 8) == (1028, 1029, 8) and shim.needs(0, 0) == (0, 1, 1)


@pytest.mark.parametrize('pen,record', [(p, r) for p in (0, 1) for r in (0, 1)], ids=lambda v: str(v))
@pytest.mark.parametrize('row', T.NOTE_ROWS, ids=[r[0] for r in T.NOTE_ROWS])
def test_note_token_against_the_model(shim, row, pen, record):
    name, max_new, prev_cap, n_prev, flags = row
    got = shim.note(max_new, prev_cap, n_prev, flags, pen, record)
    assert got == T.note_model(max_new, prev_cap, n_prev, flags, pen, record)
    step, lp_n, np_end, ended, _ = got[-1]
    assert step == len(flags) and lp_n == (len(flags) if record else 0)          # records count every token, EOS included
    assert np_end == (min(prev_cap, n_prev + flags.count(0)) if pen else n_prev)          # EOS is neither appended nor counted
    assert ended == int(any(flags) or len(flags) >= max_new)
    # a generate call reserves n_prev + max_new and reads at most max_new tokens: the capacity is never the reason a token stays out
    room = shim.needs(n_prev, max_new)[0]
    fits = shim.note(max_new, room, n_prev, flags[:max_new], pen, record)
    assert fits == T.note_model(max_new, 1 << 30, n_prev, flags[:max_new], pen, record)


def fmt(x):
    return 'nan' if math.isnan(x) else 'inf' if x == math.inf else '-inf' if x == -math.inf else float(x).hex()


def test_standalone_program_under_sanitizers(shim, tmp_path):
    """the same table through a program of its own (no Python in the process): same answers, clean exit"""
    exe, table = str(tmp_path / 'response_plan_main'), str(tmp_path / 'table.txt')
    # (the sanitizer runtime linked into the program itself: it then does not care which other libraries the loader brings first)
    static = ['-static-libsan'] if 'clang' in os.path.basename(CXX) else ['-static-libasan', '-static-libubsan']
    r = subprocess.run([CXX, *FLAGS, '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', *static, '-DRESPONSE_PLAN_MAIN', SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines, want = [], ['K ' + ' '.join(str(v) for v in shim.constants())]
    for row in T.CONS_ROWS:
        vals = ([] if row.null_eos else [str(v) for v in row.eos]) + ([] if row.null_tab else [str(v) for v in row.ids] + [fmt(b) for b in row.bias])
        lines.append(' '.join(['C', row.name, str(row.V), str(row.n_eos), str(int(row.null_eos)), str(row.min_new), str(row.n), str(int(row.null_tab))] + vals))
        rc, err, got = shim.cons(row)
        body = ' | ' + err
        if got is not None:
            body = ''.join(' %d' % t for t in got['eos']) + ' |' + ''.join(' %d:%08x' % t for t in got['table']) + body
        meta = (rc, got['on'], len(got['table']), len(got['eos']), got['min_new']) if got else (rc, 0, 0, 0, 0)
        want.append('C %s %d %d %d %d %d |' % ((row.name,) + meta) + body)
    for name, set_eos, eos_id, V, ids in T.EOS_ROWS:
        lines.append(' '.join(['E', name, str(len(set_eos))] + [str(v) for v in set_eos] + [str(eos_id), str(V), str(len(T.EOS_PROBES))] + [str(v) for v in T.EOS_PROBES]))
        want.append('E %s %d |' % (name, len(ids)) + ''.join(' %d' % v for v in ids) + ' |' + ''.join(' %d' % int(t in ids) for t in T.EOS_PROBES))
    for cap, need, first, cap_want in T.GROW_ROWS:
        lines.append('G %d %d %d' % (cap, need, first))
        want.append('G %d' % cap_want)
    for name, max_new, prev_cap, n_prev, flags in T.NOTE_ROWS:
        for pen in (0, 1):
            for record in (0, 1):
                lines.append(' '.join(['N', name, str(max_new), str(prev_cap), str(n_prev), str(pen), str(record), str(len(flags))] + [str(e) for e in flags]))
                want.append('N ' + name + ''.join(' %d,%d,%d,%d,%d' % t for t in T.note_model(max_new, prev_cap, n_prev, flags, pen, record)))
    with open(table, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    r = subprocess.run([exe, table], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == '', (r.returncode, r.stderr[-2000:])
    assert r.stdout.splitlines() == want
