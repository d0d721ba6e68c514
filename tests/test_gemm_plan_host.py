"""The GEMM regime table (tests/gemm_regimes.py) against the dispatch decision itself, without a GPU: gemm_plan() of mmduet_amd/csrc/gemm_plan.h is a
pure host function, so tests/gemm_plan_shim.cpp is compiled with the host C++ compiler into a temporary directory, loaded with ctypes, and asked about
the GemmArgs that mmd_op_gemm / mmd_op_gemm_w8 / mmd_op_gemm_slabs build for every row.  Checked per row: the plan (kernel, tiles, splits, blocks) that
tests/test_gpu_gemm_regimes.py reads back on the device, and the instantiation (MT, NT, WN) that it cannot see.  Then the rejections of the dispatcher,
the one tunable, and the profiler class of the kernel that runs."""
import ctypes as C
import os
import shutil
import subprocess
import pytest

import gemm_regimes as T

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler')

F32, BF16, F16 = 0, 1, 2                                  # mmd_dtype, and the launcher's internal IEEE-half code
EPI = dict(none=0, gelu_tanh=1, gelu_erf=2, resid=3, swiglu=4)
AUTO, SKINNY_V, BIG_V, STREAM_V = 0, 2, 4, 8               # GEMM_* variants
INVALID = -1
K_SKINNY_CLASS, K_TILE_CLASS = 0, 1                        # MMD_K_GEMM_SKINNY, MMD_K_GEMM_TILE
FIELDS = ('dtype M N K epi out_f32 variant ldx ldw ldr ldy X W Wp Wp8 wscale bias R Y ws ws_bytes slabs_out ring_slabs_out chain x_pm y_pm no_gemv ring_flags '
          'ring_max_blocks ksplit_short').split()
OUT = 'kernel tiles splits blocks mt nt wn prof_class reduce slabs ring_slabs ring_auto w_from chain gx gy kt_per_block bn bm'.split()
# 16-byte-aligned fake addresses: the planner looks at null / non-null / alignment only
X_, W_, WP_, WP8_, SC_, B_, R_, Y_, WS_ = (0x10000000 * (i + 1) for i in range(9))


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('gemm_plan') / 'gemm_plan_shim.so')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', os.path.join(HERE, 'gemm_plan_shim.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    assert lib.gemm_plan_shim_fields() == len(FIELDS)

    def ask(**kw):
        a = dict.fromkeys(FIELDS, 0)
        a.update(dtype=BF16, ring_flags=16, ksplit_short=2)
        assert set(kw) <= set(FIELDS), set(kw) - set(FIELDS)
        a.update(kw)
        out = (C.c_int * len(OUT))()
        lib.gemm_plan_shim((C.c_longlong * len(FIELDS))(*[a[f] for f in FIELDS]), out)
        return dict(zip(OUT, out))
    return ask


def row_args(row):
    """the GemmArgs mmd_op_gemm / mmd_op_gemm_w8 / mmd_op_gemm_slabs hand to the dispatcher for a row of the table"""
    N, K, epi = T.shape(row)
    M = row.M
    if row.mode == 'slabs':
        return dict(M=M, N=N, K=K, epi=EPI['none'], variant=SKINNY_V, X=X_, ldx=K, Wp=WP_, ws=WS_, ws_bytes=T.SLAB_MAX_SPLITS * M * N * 4, slabs_out=1)
    NO = N // 2 if epi == 'swiglu' else N
    a = dict(M=M, N=N, K=K, epi=EPI.get(epi, EPI['none']), out_f32=int(epi == 'out_f32'), variant=AUTO, X=X_, ldx=K, W=W_, ldw=K, Wp=WP_, Y=Y_, ldy=NO, ldr=NO,
             bias=B_ if epi in ('bias', 'gelu_tanh', 'gelu_erf') else 0, R=R_ if epi == 'resid' else 0,
             ws=WS_, ws_bytes=(192 if row.max_step_tokens > 2048 else 64) << 20)
    if row.mode == 'w8':
        a.update(Wp8=WP8_, wscale=SC_)
    return a


@pytest.mark.parametrize('row', T.ROWS, ids=[r.name for r in T.ROWS])
def test_plan_and_instantiation_of_every_row(plan, row):
    p = plan(**row_args(row))
    assert (p['kernel'], p['tiles'], p['splits'], p['blocks']) == row.plan, (row.name, p)
    assert {k: p[k.lower()] for k in row.inst} == row.inst, (row.name, p)
    assert p['blocks'] == p['gx'] * p['gy'] * p['splits'], (row.name, p)
    streaming = row.plan[0] in (T.GEMV16, T.SKINNY, T.STREAM)
    assert p['prof_class'] == (K_SKINNY_CLASS if streaming or (row.plan[0] == T.TILE64 and row.M <= 64) else K_TILE_CLASS), (row.name, p)
    # the weights a kernel reads: fp8 bytes in the GEMV / skinny kernels of an fp8 row, the packed copy in every other packed kernel, row-major in the generic ones
    assert p['w_from'] == (0 if row.plan[0] in (T.TILE64, T.TILE128) else 2 if row.mode == 'w8' and row.plan[0] in (T.GEMV16, T.SKINNY) else 1), (row.name, p)
    if row.mode == 'slabs':
        assert p['slabs'] == row.plan[2] and not p['reduce'], (row.name, p)          # the slabs are the caller's
    else:
        assert p['reduce'] == int(row.plan[2] > 1), (row.name, p)                    # nobody asked for the slabs: the reduce launch applies the epilogue


def _row(name):
    return row_args(T.rows_by_name()[name])


def test_piece_major_operands_need_the_automatic_ring(plan):
    up = _row('gemm_gate_up_513')                                     # plain 8-wave ring
    assert plan(**up)['ring_auto'] == 1
    assert plan(**up, y_pm=1)['kernel'] == T.RING256 and plan(**up, x_pm=1)['kernel'] == T.RING256
    down = _row('gemm_down_512')                                      # split-K ring: 9 splits
    assert plan(**down)['ring_auto'] == 2
    assert plan(**down, x_pm=1)['kernel'] == T.RING256
    assert plan(**down, y_pm=1)['kernel'] == INVALID                 # a piece-major output with a split-K producer: splitk_reduce writes row-major
    assert plan(**_row('gemm_qkv_512'), x_pm=1)['kernel'] == INVALID  # big tiles
    assert plan(**_row('gemm_qkv_1281'), x_pm=1)['kernel'] == INVALID  # the 4-wave ring of the mid-M cost model is not offered either
    assert plan(**_row('w8_gate_up_513'), y_pm=1)['kernel'] == INVALID  # no piece-major form with a weight scale
    forced = dict(up, variant=6)
    assert plan(**forced)['kernel'] == T.RING256 and plan(**forced)['ring_auto'] == 0 and plan(**forced, y_pm=1)['kernel'] == INVALID


def test_rejections(plan):
    qkv16, qkv17 = _row('gemm_qkv_16'), _row('gemm_qkv_17')
    assert plan(**dict(qkv16, variant=STREAM_V))['kernel'] == INVALID            # GEMM_STREAM on a shape stream_ok refuses (M <= 32)
    assert plan(**dict(_row('gemm_lm_head_65'), variant=STREAM_V))['kernel'] == INVALID          # ... (fp32 output)
    qkv2, o2 = _row('gemm_qkv_2'), _row('gemm_o_2')
    assert plan(**qkv2, chain=1)['kernel'] == T.GEMV16 and plan(**qkv2, chain=1)['chain'] == 1
    assert plan(**o2, chain=2)['chain'] == 2 and plan(**o2, chain=2)['blocks'] == 224
    assert plan(**qkv17, chain=1)['kernel'] == INVALID                           # the decode chain exists in the GEMV kernel only
    assert plan(**qkv2, chain=1, no_gemv=1)['kernel'] == INVALID
    assert plan(**qkv16, chain=1)['kernel'] == INVALID and plan(**qkv16, chain=2)['kernel'] == INVALID          # ... and there within its LDS rows / ssq entries (below)
    slab = _row('slabs_qkv_256')
    assert plan(**dict(slab, M=257, ws_bytes=16 * 257 * 4608 * 4))['kernel'] == INVALID          # slabs_out on a shape no slab kernel takes
    assert plan(**dict(slab, K=3600))['kernel'] == INVALID                       # ... K is not a whole number of steps
    assert plan(**dict(slab, ws_bytes=256 * 4608 * 4 - 1))['kernel'] == INVALID  # ... not even one slab fits
    assert plan(**dict(_row('slabs_qkv_16'), ws=0))['kernel'] == INVALID         # ... nowhere to leave them
    assert plan(**dict(qkv16, dtype=F16))['kernel'] == INVALID                   # IEEE-half operands on a skinny shape: ring / big kernels only
    assert plan(**dict(qkv17, dtype=F16))['kernel'] == INVALID
    assert plan(**dict(_row('gemm_qkv_257'), dtype=F16))['kernel'] == T.BIG64
    assert plan(**dict(_row('gemm_gate_up_513'), dtype=F16))['kernel'] == INVALID  # ... and no SwiGLU epilogue in the IEEE-half ring
    assert plan(**dict(qkv16, W=0, X=X_ + 2))['kernel'] == INVALID               # only the packed copy exists but the shape needs the generic path
    assert plan(**dict(_row('gemm_lm_head_65'), variant=BIG_V))['kernel'] == INVALID
    assert plan(**dict(_row('gemm_gate_up_513'), ring_flags=24))['kernel'] == INVALID            # a ring instantiation that is not in the library
    assert plan(**dict(qkv16, M=0))['kernel'] == -2                              # nothing to launch


def test_chain_forms_are_refused_outside_the_kernels_limits(plan):
    """A consumer keeps GEMV_CHAIN_ROWS = 4 rows x 1024 k per wave in LDS, a producer's ssq has GEMV_SSQ_STRIDE = 256 n-tile entries per row: both sides of each bound.  The
    plain GEMV at the same shapes is untouched."""
    def consumer(M, N, K, room, **kw):          # layer_qkv's form: fp32 slabs into a workspace with room for `room` of them
        return plan(M=M, N=N, K=K, epi=EPI['none'], variant=SKINNY_V, X=X_, ldx=K, Wp=WP_, ws=WS_, ws_bytes=room * M * N * 4, slabs_out=1, chain=1, **kw)

    def gate_up(M, N, K, **kw):                 # layer_tail_chain's form: SwiGLU in place, never split
        return plan(M=M, N=N, K=K, epi=EPI['swiglu'], variant=AUTO, X=X_, ldx=K, W=W_, ldw=K, Wp=WP_, Y=Y_, ldy=N // 2, ws=WS_, ws_bytes=64 << 20, chain=1, **kw)

    def producer(M, N, K, **kw):
        return plan(M=M, N=N, K=K, epi=EPI['none'], variant=SKINNY_V, X=X_, ldx=K, Wp=WP_, ws=WS_, ws_bytes=64 << 20, slabs_out=1, chain=2, **kw)
    # rows: 4 | 5
    p = consumer(4, 4608, 3584, 4)
    assert (p['kernel'], p['chain'], p['splits'], p['blocks']) == (T.GEMV16, 1, 2, 576), p
    assert consumer(5, 4608, 3584, 4)['kernel'] == INVALID and gate_up(5, 37888, 3584)['kernel'] == INVALID
    assert gate_up(4, 37888, 3584)['chain'] == 1
    # K per wave at one split: 4096 / 4 = 1024 | 4128 -> 33 k-tiles = 1056
    p = consumer(1, 512, 4096, 1)
    assert (p['kernel'], p['chain'], p['splits']) == (T.GEMV16, 1, 1), p
    assert consumer(1, 512, 4128, 1)['kernel'] == INVALID
    assert gate_up(1, 64, 4096)['splits'] == 1 and gate_up(1, 64, 4096)['chain'] == 1 and gate_up(1, 64, 4128)['kernel'] == INVALID
    # ... the bound is on the wave's range, not on K: two splits halve it (4128 -> 17 k-tiles per wave = 544; 8192 -> 1024; 8224 -> 1056)
    assert consumer(1, 512, 4128, 4)['splits'] == 2 and consumer(1, 512, 4128, 4)['kernel'] == T.GEMV16
    assert consumer(1, 512, 8192, 1)['kernel'] == INVALID
    # ... fp8 weights: ranges in pairs of k-tiles (4096 -> 16 pairs = 1024 | 4160 -> 17 pairs = 1088)
    assert consumer(1, 512, 4096, 1, Wp8=WP8_, wscale=SC_)['kernel'] == T.GEMV16 and consumer(1, 512, 4160, 1, Wp8=WP8_, wscale=SC_)['kernel'] == INVALID
    # producer: N = 16 x 256 | one tile more
    p = producer(4, 4096, 3584)
    assert (p['kernel'], p['chain'], p['splits'], p['blocks']) == (T.GEMV16, 2, 1, 256), p
    assert producer(4, 4112, 3584)['kernel'] == INVALID
    assert producer(16, 4096, 18944)['chain'] == 2          # (a producer keeps nothing per row: any M of the GEMV)
    # the plain GEMV has no such limits
    for M, N, K in ((5, 4608, 3584), (1, 512, 4128), (1, 4112, 3584), (16, 512, 8192)):
        assert plan(M=M, N=N, K=K, epi=EPI['none'], variant=SKINNY_V, X=X_, ldx=K, Wp=WP_, ws=WS_, ws_bytes=M * N * 4, slabs_out=1)['kernel'] == T.GEMV16


def test_fp32_contexts_take_the_generic_kernels(plan):
    for name in ('gemm_qkv_16', 'gemm_qkv_65', 'gemm_gate_up_513'):
        p = plan(**dict(_row(name), dtype=F32))
        assert p['kernel'] == (T.TILE128 if T.rows_by_name()[name].M >= 256 else T.TILE64) and p['w_from'] == 0, (name, p)
    assert plan(**dict(_row('gemm_qkv_16'), dtype=F32))['prof_class'] == K_SKINNY_CLASS
    assert plan(**dict(_row('gemm_qkv_65'), dtype=F32))['prof_class'] == K_TILE_CLASS


def test_the_short_k_split_of_the_gemv_is_tunable(plan):
    a = _row('slabs_qkv_1')
    assert [plan(**a, ksplit_short=k)['splits'] for k in (0, 1, 2, 3, 4, 9)] == [1, 1, 2, 3, 4, 4]
    assert plan(**_row('slabs_down_1'), ksplit_short=1)['splits'] == 4          # long K has its own rule
    assert plan(**_row('gemm_qkv_1'), ksplit_short=4)['splits'] == 1            # no slab consumer, no split


def test_split_k_slabs_go_to_the_caller_who_asks(plan):
    for name in ('gemm_down_512', 'gemm_down_511'):                              # split-K ring, big tiles with a 3-way split
        a = _row(name)
        n = T.rows_by_name()[name].plan[2]
        p, q = plan(**a), plan(**a, ring_slabs_out=1)
        assert (p['reduce'], p['ring_slabs']) == (1, 0) and (q['reduce'], q['ring_slabs']) == (0, n), (name, p, q)
        assert all(p[k] == q[k] for k in ('kernel', 'tiles', 'splits', 'blocks'))
    assert plan(**_row('gemm_qkv_512'), ring_slabs_out=1)['ring_slabs'] == 0     # unsplit: the GEMM applied its epilogue itself
