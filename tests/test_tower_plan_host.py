"""The tower regime table (tests/tower_regimes.py) against the schedule decision itself, without a GPU: tower_plan() of mmduet_amd/csrc/tower_plan.h is a pure host
function, so tests/tower_plan_shim.cpp is compiled with the host C++ compiler into a temporary directory, loaded with ctypes, and asked about every row with the
TowerModel / TowerShape that mmd_create, mmd_finalize_weights and the tower's entry points would build.  Then the refusals, the stand-alone projector plan, the contexts
that lack a packed matrix, and that no input acts on a field it does not govern."""
import ctypes as C
import os
import shutil
import subprocess
import pytest

import gemm_regimes as G
import tower_regimes as T

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler')

MMD_OK = 0
OK_ROWS = [r for r in T.ROWS if r.plan is not None]


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('tower_plan') / 'tower_plan_shim.so')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', os.path.join(HERE, 'tower_plan_shim.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.tower_plan_shim_field_name.restype = C.c_char_p
    lib.FIELDS = [lib.tower_plan_shim_field_name(i).decode() for i in range(lib.tower_plan_shim_fields())]          # the shim's own list, in its order
    assert len(set(lib.FIELDS)) == len(lib.FIELDS) > 0 and lib.tower_plan_shim_outputs() == 1 + len(T.FIELDS)
    return lib


def _pack(lib, args):
    assert set(args) == set(lib.FIELDS), set(args) ^ set(lib.FIELDS)
    return (C.c_longlong * len(lib.FIELDS))(*[int(args[f]) for f in lib.FIELDS])


@pytest.fixture(scope='module')
def plan(shim):
    def ask(args):
        out = (C.c_int * (1 + len(T.FIELDS)))()
        err = C.create_string_buffer(128)
        shim.tower_plan_shim(_pack(shim, args), out, err, len(err))
        return out[0], tuple(out[1:]), err.value.decode()
    return ask


def model_args(mode, tower, **over):
    """the TowerModel of a finalized context: tokens = grid^2 (+ 1 row with a class token); fc1 [ipad, C] / fc2 [C, ipad] have a packed copy in a bf16 context when
    N % 16 == 0 and K % 32 == 0 (make_packed) -- the half towers are bf16 contexts"""
    dtype, tower_f16 = T.MODES[mode]
    m = dict(T.TOWERS[tower], pool_mode=T.POOL_BILINEAR, class_token=False, pre_ln=False, post_ln=False, act=0, vision_only=False)
    m.update(over)
    tokens = m['grid'] ** 2
    packed = lambda N, K: dtype == T.BF16 and N % 16 == 0 and K % 32 == 0
    return dict(m, dtype=dtype, tower_f16=tower_f16, tokens=tokens, seq=tokens + (1 if m['class_token'] else 0), fc1_p=packed(m['ipad'], m['C']), fc2_p=packed(m['C'], m['ipad']),
                ws_bytes=T.TOWER_WS_BYTES)


def row_args(r, **change):
    """... and the TowerShape of the run: mmd_create's reading of MMDUET_NO_FUSE ('1' | '2': no piece-major intermediates), mmd_set_tower_share's ring cap (flags 16 at its
    first call, -1 before)"""
    a = dict(model_args(r.mode, r.tower, **r.model), B=r.B, for_pool=r.for_pool, full_tower=r.full_tower, no_pm=r.env.get('MMDUET_NO_FUSE', '')[:1] in ('1', '2'),
             ring_flags=-1 if r.ring is None else 16, ring_max_blocks=r.ring or 0, ksplit_short=2)
    assert set(change) <= set(a), set(change) - set(a)
    a.update(change)
    return a


def test_the_table_covers_every_term_and_form():
    R = T.rows_by_name()
    assert len(R) == len(T.ROWS)
    for i, f in enumerate(T.FIELDS):
        assert len({r.plan[i] for r in OK_ROWS}) > 1, f          # every field takes more than one value
    assert {r.mode for r in T.ROWS} == set(T.MODES)
    assert {r.plan[1] for r in OK_ROWS} == {T.RESID_EPI, T.RESID_F32, T.RESID_F16} and {r.plan[2] for r in OK_ROWS} == {T.EMBED_ADD_ROWS, T.EMBED_CLS, T.EMBED_F32}
    assert {r.plan[T.FIELDS.index('final_convert')] for r in OK_ROWS if r.plan[0] == T.F16} == {0, 1}          # both half forms
    # both sides of every term of the sparse-last rule: a row with the term alone against it, whose default side is a sparse row of the same mode and geometry
    alone = dict(bf16_true_full_tower=dict(full_tower=True), bf16_true_not_for_pool=dict(for_pool=False), bf16_true_average=dict(pool_mode=T.POOL_AVERAGE),
                 bf16_true_stride1=dict(pool_stride=1), bf16_true_class_token=dict(class_token=True, pre_ln=True), bf16_true_post_ln=dict(post_ln=True),
                 bf16_true_vision_only=dict(vision_only=True))
    base = R['bf16_true_b3']
    assert base.plan[3] == 1
    for name, term in alone.items():
        r = R[name]
        assert r.plan[3] == 0 and (r.mode, r.tower, r.B) == (base.mode, base.tower, base.B), name
        assert dict(r.model, for_pool=r.for_pool, full_tower=r.full_tower) == {**base.model, 'for_pool': base.for_pool, 'full_tower': base.full_tower, **term}, name
    assert R['bf16_true_quick_gelu_b17'].plan[3] == 0 and R['bf16_true_b17'].plan[3] == 1 and R['bf16_true_zero_layers_b17'].plan[3] == 0
    # the half guard: U = 64 at B = 1 | 2, U = 36 at any B, and neither in bf16
    assert [R[n].plan[3] for n in ('fp16_g16_b1', 'fp16_g16_b2', 'fp16_g12_b1', 'fp16_g12_b2', 'fp16_g12_b3', 'bf16_g16_b1', 'bf16_g12_b1')] == [0, 1, 0, 0, 0, 1, 1]
    # the piece-major rows stand on the GEMM table's rows that pin the ring's tile rule at N = 1152 (five tile columns): ring from 11 777 and from 20 225 rows, not below
    g = {r.name: r for r in G.ROWS}
    assert G.WIDTHS['fc2'][0] == G.WIDTHS['vit_o'][0] == T.TOWERS['true']['C'] and G.WIDTHS['fc1'][0] == T.TOWERS['true']['ipad']
    assert [g[n].plan[0] for n in ('gemm_vit_o_11776', 'gemm_vit_o_11777', 'gemm_vit_o_20224', 'gemm_vit_o_20225')] == [G.BIG128, G.RING256, G.BIG128, G.RING256]
    seq = T.TOWERS['true']['grid'] ** 2
    assert 16 * seq <= 11776 < 11777 <= 17 * seq <= 13056 < 18 * seq and 27 * seq <= 20224 < 20225 <= 28 * seq and 60 * 196 <= 11776 < 11777 <= 61 * 196
    pm, pm_last = T.FIELDS.index('mlp_pm'), T.FIELDS.index('mlp_pm_last')
    assert [R[f'bf16_true_b{b}'].plan[pm] for b in (16, 17, 18, 27, 28)] == [0, 1, 0, 0, 1] and [R[f'bf16_true_b{b}'].plan[pm_last] for b in (60, 61)] == [0, 1]
    assert {r.env.get('MMDUET_NO_FUSE') for r in T.ROWS} >= {'0', '1', '2'} and any(r.ring for r in T.ROWS)


@pytest.mark.parametrize('row', T.ROWS, ids=[r.name for r in T.ROWS])
def test_plan_of_every_row(plan, row):
    rc, p, err = plan(row_args(row))
    if row.plan is None:
        assert (rc, err) == (T.MMD_ERANGE, row.refusal), (row.name, rc, err)
        return
    assert (rc, err) == (MMD_OK, ''), (row.name, rc, err)
    assert p == row.plan, (row.name, dict(zip(T.FIELDS, p)))


def test_the_batch_bound_is_the_only_refusal(plan):
    for r in OK_ROWS:
        a = row_args(r)
        assert plan(dict(a, B=a['max_batch']))[0] == MMD_OK, r.name
        assert plan(dict(a, B=a['max_batch'] + 1))[::2] == (T.MMD_ERANGE, f"vit batch {a['max_batch'] + 1} exceeds max_vit_batch {a['max_batch']}"), r.name


def test_the_thresholds_are_the_named_constants(shim):
    out = (C.c_int * 3)()
    shim.tower_plan_shim_constants(out)
    assert tuple(out) == (4, 64, 64)          # 2 x 2 taps per pool output; the half kernels' S >= 64 queries and M > 64 rows


@pytest.mark.parametrize('row', T.PROJECTOR_ROWS, ids=[r.name for r in T.PROJECTOR_ROWS])
def test_projector_plan_without_a_tower_run(shim, plan, row):
    args = dict(model_args('bf16', row.tower, **row.model), B=1, for_pool=1, full_tower=1, no_pm=0, ring_flags=-1, ring_max_blocks=0, ksplit_short=2)
    out = (C.c_int * 3)()
    shim.tower_projector_plan_shim(_pack(shim, args), int(row.all_tokens), 0, out)
    assert tuple(out) == row.plan, row.name
    if not row.all_tokens:          # ... and it is the rule the tower's own plan reports: the full tower leaves every token, the projector gathers
        p = dict(zip(T.FIELDS, plan(args)[1]))
        assert (p['proj_compact'], p['proj_gather'], p['pout']) == row.plan, row.name
        shim.tower_projector_plan_shim(_pack(shim, args), 0, 1, out)          # behind a sparse last layer: the same rows, already there
        assert tuple(out) == (row.plan[0], 0, row.plan[2]), row.name


def test_contexts_that_lack_a_packed_matrix(plan):
    R = T.rows_by_name()
    for name in ('bf16_true_b17', 'bf16_true_b61', 'fp16_true_b61'):
        for missing in ('fc1_p', 'fc2_p'):          # piece-major needs both GEMMs on the ring, and the ring reads packed weights
            p = dict(zip(T.FIELDS, R[name].plan), mlp_pm=0, mlp_pm_last=0)
            assert plan(row_args(R[name], **{missing: 0}))[1] == tuple(p.values()), (name, missing)
        for change in (dict(ws_bytes=0), dict(ksplit_short=1), dict(ksplit_short=4)):          # the plain ring splits nothing: no workspace, no GEMV tuning in it
            assert plan(row_args(R[name], **change))[1] == R[name].plan, (name, change)


# input -> the fields it may change; every other field must stay in every row
GOVERNS = {
    'full_tower': ('sparse_last', 'compact_rows', 'proj_gather', 'mlp_pm_last'),
    'for_pool': ('sparse_last', 'compact_rows', 'proj_compact', 'proj_gather', 'mlp_pm_last'),
    'no_pm': ('mlp_pm', 'mlp_pm_last'),
    'post_ln': ('sparse_last', 'compact_rows', 'proj_gather', 'mlp_pm_last'),
    'act': ('sparse_last', 'compact_rows', 'proj_gather', 'mlp_pm', 'mlp_pm_last'),
    'vision_only': ('sparse_last', 'compact_rows', 'proj_compact', 'proj_gather', 'mlp_pm_last'),
    'fc1_p': ('mlp_pm', 'mlp_pm_last'),
    'fc2_p': ('mlp_pm', 'mlp_pm_last'),
    # govern nothing: the ring cap changes a ring GEMM's grid, never which kernel runs; pre_layrnorm runs in place in every form; heads only shape the attention launch
    'ring_max_blocks': (), 'pre_ln': (), 'heads': (), 'max_batch': (), 'ws_bytes': (), 'ksplit_short': (),
}


@pytest.mark.parametrize('field', list(GOVERNS))
def test_an_input_acts_on_its_fields_alone(plan, field):
    acted = set()
    for r in OK_ROWS:
        a = row_args(r)
        if field == 'ring_max_blocks':
            b = dict(a, ring_flags=16, ring_max_blocks=a['ring_max_blocks'] + 64)
        elif field in ('heads', 'max_batch', 'ws_bytes', 'ksplit_short'):
            b = dict(a, **{field: a[field] * 2})
        else:
            b = dict(a, **{field: 0 if a[field] else 1})
        (rc_a, pa, _), (rc_b, pb, _) = plan(a), plan(b)
        assert rc_a == rc_b == MMD_OK, r.name
        diff = {f for f, x, y in zip(T.FIELDS, pa, pb) if x != y}
        assert diff <= set(GOVERNS[field]), (r.name, field, diff)
        acted |= diff
    assert acted == set(GOVERNS[field]), (field, acted)
