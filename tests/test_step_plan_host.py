"""The step regime table (tests/step_regimes.py) against the schedule decision itself, without a GPU: step_plan() of mmduet_amd/csrc/step_plan.h is a pure host
function, so tests/step_plan_shim.cpp is compiled with the host C++ compiler into a temporary directory, loaded with ctypes, and asked about every row with the
StepModel / StepShape / StepSwitches that llm_step_segs and mmd_create would build.  Then the refusals, the contexts that lack a buffer or a packed matrix, and
that no switch acts outside its field."""
import ctypes as C
import os
import shutil
import subprocess
import pytest

import step_regimes as T

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler')

F32, BF16 = 0, 1
MMD_OK, MMD_EINVAL = 0, -22

@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('step_plan') / 'step_plan_shim.so')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', os.path.join(HERE, 'step_plan_shim.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.step_plan_shim_field_name.restype = C.c_char_p
    FIELDS = [lib.step_plan_shim_field_name(i).decode().lower() for i in range(lib.step_plan_shim_fields())]          # the shim's own list, in its order
    assert len(set(FIELDS)) == len(FIELDS) > 0 and lib.step_plan_shim_outputs() == 1 + len(T.FIELDS)

    def ask(segs, **kw):
        a = dict.fromkeys(FIELDS, 0)
        a.update(ksplit_short=2, s=sum(segs), nseg=len(segs))
        kw = {k.lower(): v for k, v in kw.items()}
        assert set(kw) <= set(FIELDS), set(kw) - set(FIELDS)
        a.update(kw)
        out = (C.c_int * (1 + len(T.FIELDS)))()
        err = C.create_string_buffer(128)
        lib.step_plan_shim((C.c_longlong * len(FIELDS))(*[int(a[f]) for f in FIELDS]), (C.c_int * len(segs))(*segs), out, err, len(err))
        return out[0], tuple(out[1:]), err.value.decode()
    return ask


def model_args(name, max_step_tokens=T.MAX_STEP_TOKENS):
    """the StepModel of a finalized context: a matrix [N, K] has a packed copy in bf16 when N % 16 == 0 and K % 32 == 0 (make_packed)"""
    m = T.MODELS[name]
    H, I, q_w, qkv_w = m['H'], m['I'], m['nh'] * m['d'], (m['nh'] + 2 * m['nkv']) * m['d']
    bf16 = m['dtype'] == 'bf16'
    packed = lambda N, K: bf16 and N % 16 == 0 and K % 32 == 0
    return dict(dtype=BF16 if bf16 else F32, H=H, I=I, nh=m['nh'], nkv=m['nkv'], d=m['d'], qkv_w=qkv_w, layers=2, qkv_p=packed(qkv_w, H), o_p=packed(H, q_w),
                gu_p=packed(2 * I, H), down_p=packed(H, I), fp8=m['fp8'], attn_ws=1, ws_bytes=(192 if max_step_tokens > 2048 else 64) << 20)


def switch_args(env):
    """mmd_create's reading of the environment: five switches act at '1' (MMDUET_NO_FUSE=2: the piece-major intermediates alone), three when set at all"""
    assert set(env) <= set(T.SWITCHES), env
    one = lambda k: env.get(k, '')[:1] == '1'
    return dict(no_fuse=one('MMDUET_NO_FUSE'), no_pm=env.get('MMDUET_NO_FUSE', '')[:1] in ('1', '2'), no_chain=one('MMDUET_NO_CHAIN'),
                no_slab_norm=one('MMDUET_NO_SLAB_NORM'), full_last_layer=one('MMDUET_FULL_LAST_LAYER'), no_rope_fuse=one('MMDUET_NO_ROPE_FUSE'),
                no_multi_fuse='MMDUET_NO_MULTI_FUSE' in env, no_multi_attn='MMDUET_NO_MULTI_ATTN' in env, no_chunk_rope='MMDUET_NO_CHUNK_ROPE' in env)


def row_args(row):
    return dict(model_args(row.model), n_need=row.need, hidden_out=row.hidden_out, dyn=row.dyn, **switch_args(row.env))


def test_the_table_covers_every_switch_and_schedule():
    assert len({r.name for r in T.ROWS}) == len(T.ROWS)
    assert {k for r in T.ROWS for k in r.env} == set(T.SWITCHES)
    assert {r.plan[0] for r in T.ROWS} == {T.TILE, T.FUSED, T.CHAIN}
    for i in range(1, len(T.FIELDS)):
        assert len({r.plan[i] for r in T.ROWS}) > 1, T.FIELDS[i]          # every field takes more than one value
    for r in T.ROWS:
        assert sum(r.segs) <= T.MAX_STEP_TOKENS and not (r.need and r.hidden_out) and (len(r.segs) == 1 or r.need == len(r.segs)), r.name


@pytest.mark.parametrize('row', T.ROWS, ids=[r.name for r in T.ROWS])
def test_plan_of_every_row(plan, row):
    rc, p, err = plan(row.segs, **row_args(row))
    assert (rc, err) == (MMD_OK, ''), (row.name, rc, err)
    assert p == row.plan, (row.name, dict(zip(T.FIELDS, p)))
    if row.need > 64:          # what reaches the step when more than 64 rows are read: no list
        assert plan(row.segs, **dict(row_args(row), n_need=0))[1] == row.plan, row.name


def test_refusals(plan):
    one, two = T.rows_by_name()['graph_1'], T.rows_by_name()['talk_1x2']
    assert plan(two.segs, **dict(row_args(two), dyn=1))[::2] == (MMD_EINVAL, 'graph decode is single-stream')
    for change in (dict(model_args('fp32')), switch_args({'MMDUET_NO_FUSE': '1'}), dict(qkv_p=0), dict(ws_bytes=0)):
        assert plan(one.segs, **dict(row_args(one), **change))[::2] == (MMD_EINVAL, 'graph decode needs the fused bf16 schedule'), change
    assert plan((257,), **dict(row_args(one)))[::2] == (MMD_EINVAL, 'graph decode needs the fused bf16 schedule')
    assert plan(one.segs, **dict(row_args(one), **switch_args({'MMDUET_NO_CHAIN': '1'})))[:2] == (MMD_OK, (T.FUSED, 0, 0, 0, 0, 0, 0, 0, 0))


def test_contexts_that_lack_a_buffer_or_a_packed_matrix(plan):
    R = T.rows_by_name()
    talk, chunk, dec = R['talk_1x2'], R['frame_700'], R['fwd_1']
    assert plan(talk.segs, **dict(row_args(talk), attn_ws=0))[1] == (T.CHAIN, 1, 0, 0, 0, 0, 0, 0, 0)          # no batched attention without its workspace
    for missing in ('qkv_p', 'o_p', 'down_p'):          # every slab GEMM of the layer must have its kernel
        assert plan(dec.segs, **dict(row_args(dec), **{missing: 0}))[1][0] == T.TILE, missing
    assert plan(dec.segs, **dict(row_args(dec), gu_p=0))[1] == dec.plan
    assert plan(chunk.segs, **dict(row_args(chunk), o_p=0))[1] == (T.TILE, 0, 1, 0, 0, 0, 0, 1, 1)             # the sparse last layer needs o_proj's and down_proj's slabs
    assert plan(chunk.segs, **dict(row_args(chunk), gu_p=0))[1] == (T.TILE, 0, 1, 1, 0, 0, 0, 1, 0)            # piece-major needs both GEMMs on the ring
    assert plan(chunk.segs, **dict(row_args(chunk), down_p=0))[1] == (T.TILE, 0, 1, 0, 0, 0, 0, 0, 0)
    assert plan(chunk.segs, **dict(row_args(chunk), ws_bytes=0))[1] == (T.TILE, 0, 1, 0, 0, 0, 0, 0, 0)        # no split K without a workspace: no slabs anywhere, down_proj off the ring
    big = dict(row_args(chunk), **dict(model_args('bf16', max_step_tokens=4096)))                             # the 192 MB workspace changes split counts, not the schedule
    assert plan(chunk.segs, **big)[1] == chunk.plan
    for k in (0, 1, 2, 3, 4, 9):          # the GEMV's short-K split is clamped to 1..4 slabs: always within what the attention kernel sums
        assert plan(dec.segs, **dict(row_args(dec), ksplit_short=k))[1] == dec.plan, k


@pytest.mark.parametrize('switch,field', [('MMDUET_NO_CHAIN', 'schedule'), ('MMDUET_NO_SLAB_NORM', 'down_slab_norm'), ('MMDUET_FULL_LAST_LAYER', 'sparse_last'),
                                          ('MMDUET_NO_ROPE_FUSE', 'rope_fused'), ('MMDUET_NO_CHUNK_ROPE', 'chunk_rope')])
def test_a_switch_acts_on_its_field_alone(plan, switch, field):
    """over every default bf16 row: the switch changes its own field in at least one row and no other field in any (MMDUET_NO_CHAIN also ends the
    chain's rope_fused: the attention kernel's own q / k / v preparation outside a round of talkers exists for the chain's steps)"""
    also = {'MMDUET_NO_CHAIN': ('rope_fused',)}.get(switch, ())
    acted = False
    for r in T.ROWS:
        if r.model != 'bf16' or r.env:
            continue
        a, b = plan(r.segs, **row_args(r))[1], plan(r.segs, **row_args(r._replace(env={switch: '1'})))[1]
        diff = {f for f, x, y in zip(T.FIELDS, a, b) if x != y}
        assert diff <= {field, *also}, (r.name, diff)
        acted |= field in diff
    assert acted
