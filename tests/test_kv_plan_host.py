"""The KV arena table (tests/kv_plan_cases.py) against the plan itself, without a GPU: kv_plan() and the growth functions of mmduet_amd/csrc/kv_plan.h are pure host functions,
so tests/kv_plan_shim.cpp is compiled with the host C++ compiler into a temporary directory, loaded with ctypes, and asked about every row.  Then the geometry's accessors,
the V span against the layout's own index formula, the capacities growth tries, and that the table moves every field and names every operation."""
import ctypes as C
import os
import shutil
import subprocess
import pytest

import kv_layout as L
import kv_plan_cases as T

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler')


def _ll(values):
    return (C.c_longlong * len(values))(*values)


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('kv_plan') / 'kv_plan_shim.so')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', os.path.join(HERE, 'kv_plan_shim.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.kv_shim_field_name.restype = lib.kv_shim_constant_name.restype = C.c_char_p
    for f in (lib.kv_shim_constant, lib.kv_initial_tokens_shim, lib.kv_vmm_chunk_tokens_shim):
        f.restype = C.c_longlong
    lib.kv_initial_tokens_shim.argtypes = [C.c_longlong]
    lib.kv_vmm_chunk_tokens_shim.argtypes = [C.c_longlong] * 2
    lib.kv_vmm_reservations_shim.argtypes = [C.c_longlong] * 3 + [C.c_void_p]
    lib.kv_geom_shim.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
    lib.kv_grow_shim.argtypes = [C.c_void_p] + [C.c_longlong] * 3 + [C.c_void_p]
    lib.kv_plan_shim.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    assert tuple(lib.kv_shim_field_name(i).decode() for i in range(lib.kv_shim_fields())) == T.FIELDS          # the shim's own list, in its order
    assert {lib.kv_shim_constant_name(i).decode(): lib.kv_shim_constant(i) for i in range(lib.kv_shim_constants())} == T.CONSTANTS

    class Ask:
        @staticmethod
        def plan(row):
            """-> (rc, {field: value}, message)"""
            out, err = (C.c_longlong * (1 + len(T.FIELDS)))(), C.create_string_buffer(320)
            lib.kv_plan_shim(row.op, _ll(row.geom), _ll(row.state), row.a, row.b, _ll(row.src) if row.src else None, row.bufs, out, err, len(err))
            return out[0], dict(zip(T.FIELDS, out[1:])), err.value.decode()

        @staticmethod
        def geom(g, cap):
            out = (C.c_longlong * 6)()
            lib.kv_geom_shim(_ll(g), cap, out)
            return tuple(out)

        @staticmethod
        def reservations(initial, requested, chunk):
            out = (C.c_longlong * T.CONSTANTS['KV_MAX_RESERVATIONS'])()
            return list(out[:lib.kv_vmm_reservations_shim(initial, requested, chunk, out)])

        @staticmethod
        def grow(g, cap, need, length):
            out = (C.c_longlong * 3)()
            lib.kv_grow_shim(_ll(g), cap, need, length, out)
            return tuple(out)
        initial_tokens = staticmethod(lib.kv_initial_tokens_shim)
        chunk_tokens = staticmethod(lib.kv_vmm_chunk_tokens_shim)
    return Ask


def test_the_table_names_every_operation_and_moves_every_field():
    assert len({r.name for r in T.ROWS}) == len(T.ROWS)
    assert {r.op for r in T.ROWS} == set(range(len(T.OPS)))
    assert {r.op for r in T.ROWS if r.plan} == set(range(len(T.OPS)))          # ... each with a plan, and each that can refuse with a refusal
    assert {r.op for r in T.ROWS if r.refusal} == set(range(len(T.OPS))) - {T.RESET, T.DEBUG_SET_LEN}
    assert {r.geom for r in T.ROWS} >= {T.TINY, T.B7}
    plans = [r.plan for r in T.ROWS if r.plan]
    for f in T.FIELDS:
        assert all(set(p) == set(T.FIELDS) for p in plans)
        assert len({p[f] for p in plans}) > 1, f          # every field takes more than one value
    assert {p['launch'] for p in plans} == {T.NONE, T.ROWS_OUT, T.ROWS_IN, T.LAUNCH_DROP, T.CANON_GATHER, T.CANON_SCATTER}
    assert {r.refusal[0] for r in T.ROWS if r.refusal} == {T.MMD_EINVAL, T.MMD_ERANGE}
    assert {r.bufs for r in T.ROWS} == {T.BUF_OK, T.BUF_MISSING, T.BUF_MISALIGNED}


@pytest.mark.parametrize('row', T.ROWS, ids=[r.name for r in T.ROWS])
def test_kv_plan_of_every_row(shim, row):
    rc, p, err = shim.plan(row)
    if row.refusal:
        assert rc == row.refusal[0] and row.refusal[1] in err, (row.name, rc, err)
    else:
        assert (rc, err) == (T.MMD_OK, ''), (row.name, rc, err)
        assert p == row.plan, (row.name, {f: (p[f], row.plan[f]) for f in T.FIELDS if p[f] != row.plan[f]})


def test_the_geometry(shim):
    assert shim.geom(T.TINY, 256)[:3] == (L.BLK, 32, 6) and shim.geom(T.B7, 256)[:3] == (L.BLK, 256, 112)
    for g in (T.TINY, T.B7):
        for cap in (256, 8192, 4 << 20, 1 << 30):
            blk, tok, rows, pitch, layer, arena = shim.geom(g, cap)
            # one kv head's row is cap tokens of head_dim elements; a layer is its kv heads' rows; K (and V) is the layers
            assert pitch == cap * g.head_dim * g.elem and layer == g.kv_heads * pitch and arena == g.layers * layer == rows * cap * tok


@pytest.mark.parametrize('row', [r for r in T.ROWS if r.plan and r.plan['launch'] in (T.ROWS_OUT, T.ROWS_IN) and r.plan['k_bytes']],
                         ids=lambda r: r.name)
def test_the_v_span_holds_its_tokens_in_the_layout(shim, row):
    """kv_layout.v_index places every (token, dim) of the span inside the V bytes the plan moves, the span starts and ends on a block's first and last element, and a block
    less at either end would lose a token"""
    _, p, _ = shim.plan(row)
    g, e = row.geom, row.geom.elem
    frm ={T.STASH: row.a, T.UNSTASH: row.state.stash_from}.get(row.op, 0)
    to = frm + p['k_bytes'] // (g.head_dim * e)
    row0 = p['k_off'] - frm * g.head_dim * e          # where the head's row starts (the layer's offset of a debug_read)
    lo, hi = p['v_off'] - row0, p['v_off'] - row0 + p['v_bytes']
    idx = [L.v_index(t, d, g.head_dim) * e for t in (frm, to - 1) for d in (0, g.head_dim - 1)]
    assert lo <= min(idx) and max(idx) + e <= hi
    assert lo == L.v_index(frm - frm % L.BLK, 0, g.head_dim) * e and hi == (L.v_index(to - 1 | (L.BLK - 1), g.head_dim - 1, g.head_dim) + 1) * e
    assert lo + L.BLK * g.head_dim * e > min(idx) and hi - L.BLK * g.head_dim * e < max(idx) + e


def test_growth_chunk(shim):
    for t, gran in T.CHUNK_CASES:
        got = shim.chunk_tokens(t, gran)
        assert got == T.chunk_tokens(t, gran), (t, gran, got)
        assert got % L.BLK == 0 and got * t % gran == 0 and got * t >= 2 * T.MiB
        if (t, gran) in T.CHUNK_KNOWN:
            assert got == T.CHUNK_KNOWN[(t, gran)]


def test_growth_first_backing(shim):
    assert [shim.initial_tokens(n) for n in (-5, 0, 1, 256, 257, 320, 1000, 100000)] == [256, 256, 256, 256, 320, 320, 1024, 100032]


@pytest.mark.parametrize('initial', T.RESERVATION_INITIALS)
def test_growth_reservations(shim, initial):
    ct = T.RESERVATION_CHUNK
    for name, requested in T.reservation_requests(initial):
        tries = shim.reservations(initial, requested, ct)
        assert 1 <= len(tries) <= 64, (name, tries)
        assert all(v % ct == 0 for v in tries), (name, tries)
        assert all(a > b for a, b in zip(tries, tries[1:])), (name, tries)          # strictly decreasing: the list ends
        assert tries[0] == T.up(max(requested, initial), ct) and tries[-1] == T.up(initial, ct), (name, tries)
        for a, b in zip(tries, tries[1:]):
            assert b == max(T.up(a // 2, ct), tries[-1]), (name, tries)          # each a half of the one before, in whole chunks, never below the first backing
    assert shim.reservations(256, 4 << 20, 8192) == [8192 << k for k in range(9, -1, -1)]


def test_growth_fallback(shim):
    for cap, need, doubled in T.GROW_CASES:
        first, second, _ = shim.grow(T.B7, cap, need, 0)
        assert first == doubled and first >= need and first // cap & (first // cap - 1) == 0, (cap, need, first)          # cap times a power of two
        assert first // 2 < need or first == 2 * cap
        assert second == T.up(need + need // 8, L.BLK), (cap, need, second)
    # what the reallocation carries over per row: the live tokens in whole V blocks
    for g in (T.TINY, T.B7):
        assert [shim.grow(g, 256, 257, n)[2] for n in (0, 1, 64, 65, 200)] == [b * L.BLK * g.head_dim * g.elem for b in (0, 1, 1, 2, 4)]
