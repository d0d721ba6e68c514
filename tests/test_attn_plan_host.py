"""The attention regime table (tests/attn_regimes.py) against the dispatch decision itself, without a GPU: attn_plan() and attn_plan_decode_multi() of
mmduet_amd/csrc/attn_plan.h are pure host functions, so tests/attn_plan_shim.cpp is compiled with the host C++ compiler into a temporary directory, loaded with ctypes,
and asked about the AttnArgs that the row's caller builds.  Checked per row: form and key splits (what tests/test_gpu_attn_regimes.py reads back on the device), the
geometry the table derives by hand, and the plan's own consistency -- grid against form, the statistics' offset, the workspace, the key ranges, the chunk table.  Then the two
A/B switches and what AttnArgs::plan_out receives."""
import ctypes as C
import os
import shutil
import subprocess
import pytest

import attn_regimes as T

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler')

FIELDS = ('dtype S nh nkv d n_ctx causal batch variant ldq ldo k_hs k_ts v_hs v_ts v_transposed q_bstride kv_bstride o_bstride q K V ws ws_bytes dyn dyn_splits qkv_slabs n_slabs '
          'segs nseg decode_ring vit_ring multi').split()
OUT = 'form kernel splits kv_per_split block_rows gx gy gz threads lds dp nc dvt exact f16 rt nslot waves merge merge_gx merge_rows nb off_hi off_lo qblocks'.split()
K_SIMPLE, K_MFMA, K_ROWMAJOR, K_D72_RING, K_GQA128, K_GQA128_W1, K_GQA128_CHUNK = range(7)          # ATTN_K_*
M_NONE, M_GENERIC, M_ROWS, M_128, M_CHUNK = range(5)                                                # ATTN_MERGE_*
KERNEL_OF_FORM = {1: K_SIMPLE, 2: K_MFMA, 3: K_GQA128, 4: K_GQA128, 5: K_GQA128_W1, 6: K_ROWMAJOR, 7: K_D72_RING, 8: K_GQA128_CHUNK, 9: K_GQA128}


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('attn_plan') / 'attn_plan_shim.so')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', os.path.join(HERE, 'attn_plan_shim.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    assert lib.attn_plan_shim_fields() == len(FIELDS) and lib.attn_plan_shim_outputs() == len(OUT)
    tab, units = lib.attn_plan_shim_tab(), lib.attn_plan_shim_units()

    def ask(a):
        assert set(a) <= set(FIELDS), set(a) - set(FIELDS)
        a = {**dict.fromkeys(FIELDS, 0), **a}
        out = (C.c_int * len(OUT))(); start = (C.c_int * (tab + 1))(); b0 = (C.c_int * units)(); b1 = (C.c_int * units)()
        lib.attn_plan_shim((C.c_longlong * len(FIELDS))(*[a[f] for f in FIELDS]), out, start, b0, b1)
        p = dict(zip(OUT, out))
        p['ws_ml_off'] = p.pop('off_hi') * 2 ** 31 + p.pop('off_lo')
        if p['form'] == 8:
            n = p['qblocks'] * a['nkv']
            p.update(start=list(start), b0=list(b0)[:n], b1=list(b1)[:n])
        return p
    return ask


@pytest.mark.parametrize('row', T.ROWS, ids=[r.name for r in T.ROWS])
def test_plan_of_every_row(plan, row):
    a = T.build_args(row)
    p = plan(a)
    if row.form == T.INVALID:
        assert p['form'] == T.INVALID, (row.name, p)
        return
    assert (p['form'], p['splits']) == (row.form, row.splits), (row.name, p)
    S, nh, nkv, d, n_tot = row.S, row.nh, row.nkv, row.d, row.n_ctx + row.S
    G = nh // nkv
    form, splits, batch, nseg = p['form'], p['splits'], a['batch'], a.get('nseg', 0)
    assert p['kernel'] == KERNEL_OF_FORM[form], (row.name, p)
    # ---- the geometry the table derives by hand
    for k, v in row.geom.items():
        got = {'qblocks': p['gx'], 'block_rows': p['block_rows'], 'nb': p['nb'], 'dp': p['dp'],
               'inst': (p['nc'], p['dvt'], p['exact']) if form == 6 else (p['rt'], p['nslot'], p['waves'])}[k]
        assert got == v, (row.name, k, got, v)
    # ---- grid against form: every query row in exactly one block row, every split a grid plane
    grid = (p['gx'], p['gy'], p['gz'])
    if form == 1:
        assert grid == (S, nh, batch) and p['threads'] == 64
    elif form == 2:
        assert grid == (cdiv(S * G, 64), nkv * batch, splits) and p['dp'] in (32, 64, 96, 128) and p['dp'] - 32 < d <= p['dp']
    elif form in (3, 4):
        rows_per_block = {(1, 2, 4): 64, (1, 4, 4): 64, (2, 2, 4): 128, (2, 4, 8): 256}[(p['rt'], p['nslot'], p['waves'])]
        assert grid == (cdiv(S * G, rows_per_block), nkv, splits) and p['threads'] == 64 * p['waves'] and p['lds'] == 32768 * p['nslot']
        assert (form == 3) == (S * G <= 64) and (p['waves'] == 8) == (S * G >= 1024)
    elif form == 5:
        assert grid == (cdiv(S * G, p['block_rows']), nkv, splits) and p['block_rows'] % 16 == 0 and 16 <= p['block_rows'] <= 256
        assert p['gx'] == cdiv(S * G, 256)                         # the fewest blocks of <= 256 rows
        assert p['threads'] == 512 and p['lds'] == 4 * 32768
    elif form in (6, 7):
        assert grid == (cdiv(S, 128), nh, batch) and splits == 1 and p['threads'] == 256
        assert p['f16'] == int(row.dtype == T.F16)
    elif form == 8:
        assert grid == (p['nb'], 1, 1) and 1 <= p['nb'] <= 256 and p['threads'] == 512 and p['lds'] == 4 * 32768
    elif form == 9:
        assert grid == (nseg, nkv, splits) and (p['rt'], p['nslot'], p['waves']) == (1, 4, 4) and nseg * nkv * splits <= 512 and splits >= 2
    # ---- partials, statistics and the merge launch
    rows_all = (nseg or 1) * nkv * batch * S * G if form in (2, 3, 4, 5, 8, 9) else 0
    width = p['dp'] if form == 2 else 128
    if rows_all and a['ws']:
        assert p['ws_ml_off'] == splits * rows_all * width, (row.name, p)
    elif not rows_all:
        assert p['ws_ml_off'] == -1 and p['merge'] == M_NONE, (row.name, p)
    if splits > 1:
        assert a['ws'] and splits * rows_all * (width + 2) * 4 <= a['ws_bytes'], (row.name, 'partials + statistics exceed the workspace', p)
        assert splits <= 64
    if form == 8:
        assert (p['merge'], p['merge_gx'], p['merge_rows']) == (M_CHUNK, cdiv(rows_all, 4), rows_all)
    elif form == 9:
        assert (p['merge'], p['merge_gx'], p['merge_rows']) == (M_ROWS, rows_all, rows_all // nseg)
    elif splits > 1:
        want = (M_GENERIC, rows_all) if form == 2 else (M_ROWS, rows_all) if form in (3, 4) and rows_all <= 64 else (M_128, cdiv(rows_all, 4))
        assert (p['merge'], p['merge_gx'], p['merge_rows']) == (*want, rows_all), (row.name, p)
    else:
        assert p['merge'] == M_NONE, (row.name, p)
    # ---- the splits' key ranges cover every key (the chunk form, form 9 and the unsplit tower kernels cut theirs in the kernel)
    if form in (2, 3, 4, 5):
        assert p['kv_per_split'] * splits >= n_tot and p['kv_per_split'] % (32 if form == 2 else 64) == 0, (row.name, p)
        if not a.get('dyn'):
            assert p['kv_per_split'] * (splits - 1) < n_tot, (row.name, 'an empty split', p)
    else:
        assert p['kv_per_split'] == 0
    # ---- the chunk table: units in key order, every unit inside the blocks that share it
    if form == 8:
        qb, nb, st = p['qblocks'], p['nb'], p['start']
        assert qb == cdiv(S * G, 256) and st[0] == 0
        assert all(st[i] <= st[i + 1] for i in range(len(st) - 1)) and all(v == st[qb] for v in st[qb:])
        for b in range(qb):          # a unit's tiles: the keys its last row sees
            last_row = min(b * 256 + 255, S * G - 1)
            assert st[b + 1] - st[b] == cdiv(min(row.n_ctx + last_row // G + 1, n_tot), 64), (row.name, b)
        W = st[qb] * nkv
        assert nb == min(256, W)
        for u, (b0, b1) in enumerate(zip(p['b0'], p['b1'])):
            assert 0 <= b0 <= b1 < nb, (row.name, u, b0, b1)
            kvh, bx = divmod(u, qb)
            first, last = kvh * st[qb] + st[bx], kvh * st[qb] + st[bx + 1] - 1
            assert W * b0 // nb <= first < W * (b0 + 1) // nb and W * b1 // nb <= last < W * (b1 + 1) // nb, (row.name, u)          # block b owns linear tiles [W b / nb, W (b + 1) / nb)
            assert b1 - b0 + 1 <= splits, (row.name, 'a unit with more parts than partial slots', u)
        assert all(x <= y for x, y in zip(p['b0'], p['b0'][1:])), row.name


def _row(name):
    return T.build_args(T.rows_by_name()[name])


def test_the_decode_ring_switch(plan):
    """MMDUET_ATTN_DECODE_RING=0 keeps the decode geometry on the two-slot kernel: same form, same splits, same merge; every other geometry ignores the switch"""
    on, off = plan(_row('llm_S1_n15000')), plan(dict(_row('llm_S1_n15000'), decode_ring=0))
    assert (on['rt'], on['nslot'], on['waves'], on['lds']) == (1, 4, 4, 131072) and (off['rt'], off['nslot'], off['waves'], off['lds']) == (1, 2, 4, 65536)
    assert all(on[k] == off[k] for k in OUT[:10] + ['merge', 'merge_gx', 'ws_ml_off'] if k != 'lds')
    for name in ('llm_S3_n100', 'llm_S49_n15000', 'llm_S1274_n15000', 'llm_S1911_n15000', 'tower_d72', 'op_v2_d32'):
        assert plan(_row(name)) == plan(dict(_row(name), decode_ring=0)), name
    assert plan(dict(_row('multi_4_streams'), decode_ring=0)) == plan(_row('multi_4_streams'))          # form 9 exists on the ring only


def test_the_tower_ring_switch(plan):
    """MMDUET_VIT_ATTN_RING=0 sends d = 72 non-causal to the register-staged kernel (form 6, <3, 5, EXACT>) over the same grid; nothing else moves"""
    on, off = plan(_row('tower_d72')), plan(dict(_row('tower_d72'), vit_ring=0))
    assert (on['form'], on['kernel'], on['lds']) == (7, K_D72_RING, 40960) and (off['form'], off['kernel'], off['lds']) == (6, K_ROWMAJOR, 0)
    assert (off['nc'], off['dvt'], off['exact']) == (3, 5, 1) and all(on[k] == off[k] for k in ('gx', 'gy', 'gz', 'threads', 'splits'))
    for name in ('tower_d64', 'tower_d96', 'op_v4_d72_causal', 'llm_S1_n15000', 'llm_S1274_n15000'):
        assert plan(_row(name)) == plan(dict(_row(name), vit_ring=0)), name


def test_plan_out_is_form_and_splits():
    """launch_plan (attn.hip) writes AttnArgs::plan_out = {form, splits} of a valid plan and {0, 1} otherwise; an empty launch (S <= 0) writes nothing.  The statement is read
    from the source here; tests/test_gpu_attn_regimes.py observes it through mmd_op_attention_last_form."""
    src = open(os.path.join(HERE, '..', 'mmduet_amd', 'csrc', 'attn.hip')).read()
    assert 'if (a.plan_out) { a.plan_out[0] = pl.valid() ? pl.form : 0; a.plan_out[1] = pl.valid() ? pl.splits : 1; }' in src
    assert 'if (pl.form == ATTN_PLAN_EMPTY) return hipSuccess;' in src


def test_nothing_to_launch(plan):
    assert plan(dict(_row('llm_S1_n15000'), S=0))['form'] == -2          # ATTN_PLAN_EMPTY


def test_the_table_covers_every_form_and_both_sides_of_the_edges():
    forms = {r.form for r in T.ROWS}
    assert forms >= set(range(1, 10)) | {T.INVALID}
    assert {r.form for r in T.OP_ROWS} >= {1, 2, 3, 4, 5, 6, 7, 8}
    by = T.rows_by_name()
    for lo, hi in (('llm_S2_n15000', 'llm_S3_n15000'), ('llm_S9_n1000', 'llm_S10_n1000'), ('llm_S10_n4085', 'llm_S10_n4086'), ('llm_S109_n15000', 'llm_S110_n15000'),
                   ('llm_S146_n15000', 'llm_S147_n15000'), ('llm_S329_n15000', 'llm_S330_n15000'), ('llm_S1274_n950', 'llm_S1274_n951'), ('llm_S1865_n15000', 'llm_S1866_n15000'),
                   ('llm_S1274_n15000_ws_under_3_parts', 'llm_S1274_n15000_ws_3_parts')):
        a, b = by[lo], by[hi]
        assert (a.form, a.splits, a.geom) != (b.form, b.splits, b.geom), (lo, hi)
