"""The GEMM regime table (tests/gemm_regimes.py) against the header and against itself, without a GPU: every kernel id of GEMM_K_* has a row, every
M threshold has its rows on both sides at every swept width, every named edge really switches the plan, and every row meets the shape conditions of
the kernel and instantiation it claims (tests/test_gemm_plan_host.py then asks the dispatch decision itself, on the host, and tests/test_gpu_gemm_regimes.py checks on the
device that every row's kernel really runs and computes the right thing)."""
import os
import re
import pytest

import gemm_regimes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cdiv(a, b):
    return -(-a // b)


def _header_kernel_ids():
    src = open(os.path.join(ROOT, 'mmduet_amd', 'csrc', 'gemm_plan.h')).read()
    m = re.search(r'enum\s*\{\s*(GEMM_K_[^}]*)\}', src)
    assert m, 'GEMM_K_* enum not found in gemm_plan.h'
    ids = dict((k, int(v)) for k, v in re.findall(r'GEMM_K_(\w+)\s*=\s*(\d+)', m.group(1)))
    assert ids
    return ids


def test_kernel_ids_match_the_header():
    ids = _header_kernel_ids()
    assert ids == {name: k for k, name in T.KERNEL_NAMES.items()}


def test_every_kernel_id_has_a_row():
    have = {r.plan[0] for r in T.ROWS}
    missing = [name for name, k in _header_kernel_ids().items() if k not in have]
    assert not missing, f'no table row runs GEMM_K_{missing}'


def test_row_names_are_unique_and_say_what_the_row_is():
    names = [r.name for r in T.ROWS]
    assert len(names) == len(set(names))
    for r in T.ROWS:
        assert r.name == f'{r.mode}_{r.width}_{r.M}' + ('' if r.max_step_tokens == 1024 else f'_ws{r.max_step_tokens}'), r


@pytest.mark.parametrize('mode,width', T.SWEEPS)
def test_every_threshold_has_both_sides(mode, width):
    have = {r.M for r in T.ROWS if r.mode == mode and r.width == width and r.max_step_tokens == 1024}
    want = [M for M in T.THRESHOLD_MS if mode != 'slabs' or M <= T.SLAB_MAX_M]
    missing = [M for M in want if M not in have]
    assert not missing, f'{mode} {width}: no row at M = {missing}'


@pytest.mark.parametrize('what,below,above', T.EDGES, ids=[e[1] + '->' + e[2] for e in T.EDGES])
def test_every_edge_has_both_sides_and_switches(what, below, above):
    rows = T.rows_by_name()
    assert below in rows and above in rows, (what, below, above)
    a, b = rows[below], rows[above]
    assert (a.plan, a.inst) != (b.plan, b.inst), f'{what}: {below} and {above} claim the same plan'
    assert a.mode == b.mode and T.WIDTHS[a.width][0] == T.WIDTHS[b.width][0]


def test_every_row_is_required():
    """A row is there for a threshold sweep, an edge or a stated coverage reason -- so that deleting any row fails a test above."""
    need = set(T.COVERAGE)
    for mode, width in T.SWEEPS:
        need |= {f'{mode}_{width}_{M}' for M in T.THRESHOLD_MS if mode != 'slabs' or M <= T.SLAB_MAX_M}
    for _, below, above in T.EDGES:
        need |= {below, above}
    have = set(T.rows_by_name())
    assert have == need, dict(unrequired=sorted(have - need), missing=sorted(need - have))


def test_every_tile_regime_has_an_m_that_is_not_a_multiple_of_16():
    for k in (T.SKINNY, T.STREAM, T.BIG64, T.BIG128, T.RING256, T.RING128X2, T.TILE64, T.TILE128):
        Ms = [r.M for r in T.ROWS if r.plan[0] == k]
        assert any(M % 16 for M in Ms), (T.KERNEL_NAMES[k], Ms)


@pytest.mark.parametrize('row', T.ROWS, ids=[r.name for r in T.ROWS])
def test_row_meets_the_conditions_of_its_kernel(row):
    N, K, epi = T.shape(row)
    M, (kernel, tiles, splits, blocks), inst = row.M, row.plan, row.inst
    assert row.mode in ('gemm', 'slabs', 'w8') and row.max_step_tokens in (1024, 4096)
    assert epi in ('bias', 'resid', 'swiglu', 'gelu_tanh', 'gelu_erf', 'out_f32', 'slab')
    assert M >= 1 and splits >= 1 and blocks >= 1 and tiles >= 1
    if row.mode == 'slabs':
        assert M <= T.SLAB_MAX_M and kernel in (T.GEMV16, T.SKINNY, T.STREAM) and splits <= T.SLAB_MAX_SPLITS
        assert row.max_step_tokens == 1024                                   # the workspace is the caller's slab buffer
    if row.mode == 'w8':
        assert N % 16 == 0 and K % 64 == 0 and epi != 'out_f32'              # mmd_op_gemm_w8's own conditions
    if epi == 'swiglu':
        assert N % 32 == 0 and splits == 1                                    # no kernel splits K under the SwiGLU epilogue
    nt = N // 16
    if kernel == T.GEMV16:
        assert M <= 16 and N % 16 == 0 and K % 32 == 0 and tiles == nt
        two = epi == 'swiglu' or (nt % 2 == 0 and nt >= 2048)
        assert inst == dict(NT=2 if two else 1) and blocks == (nt // 2 if two else nt) * splits
        assert splits == 1 or row.mode == 'slabs'                             # the GEMV splits K only for slab consumers
    elif kernel == T.SKINNY:
        assert M <= 64 and N % 16 == 0 and K % 32 == 0 and tiles == nt
        assert inst['MT'] == (1 if M <= 16 else 2 if M <= 32 else 4) and 16 * inst['MT'] >= M
        assert inst['NT'] == (2 if epi == 'swiglu' or nt >= 4096 else 1)
        assert blocks == cdiv(nt, 4 * inst['NT']) * splits and splits <= 8
        assert M <= 32 or row.mode == 'w8' or epi == 'out_f32'                # 33..64 rows: the stream kernel, unless fp8 or fp32 output
    elif kernel == T.STREAM:
        assert 32 < M <= 256 and N % 16 == 0 and epi != 'out_f32' and tiles == nt
        ksb = 4 if M <= 128 else 2
        assert K % (ksb * 32) == 0
        assert inst['MT'] == (4 if M <= 64 else 8 if M <= 128 else 16) and 4 <= inst['WN'] <= 8
        assert inst['NT'] == (2 if epi == 'swiglu' or nt >= 4096 else 1)
        assert blocks == cdiv(nt, inst['WN'] * inst['NT']) * splits and splits <= 16
        assert row.mode != 'w8' or M > 64
    elif kernel in (T.BIG64, T.BIG128):
        bn = 64 if kernel == T.BIG64 else 128
        assert M > 64 and N % bn == 0 and K % 64 == 0 and epi not in ('out_f32', 'slab') and inst == {}
        assert tiles in ((N // bn) * cdiv(M, 128), (N // 64) * cdiv(M, 160)) and blocks == tiles * splits
        assert splits == 1 or K >= 2048
    elif kernel in (T.RING256, T.RING128X2):
        bn = 256 if kernel == T.RING256 else 128
        assert M >= 512 and N % (32 if kernel == T.RING256 else 128) == 0 and K % 64 == 0 and epi not in ('out_f32', 'slab') and inst == {}
        assert tiles == cdiv(N, bn) * cdiv(M, 256)
        slots = 256 if kernel == T.RING256 else 512
        assert blocks == (tiles * splits if splits > 1 else min(tiles, slots))
        assert splits == 1 or K >= 8192                                        # the automatic split ring is for long K
        ws = (192 if row.max_step_tokens > 2048 else 64) << 20
        assert splits == 1 or splits * M * N * 4 <= ws                          # the slabs fit the context's workspace
    elif kernel in (T.TILE64, T.TILE128):
        assert row.mode == 'gemm' and epi == 'out_f32' and inst == {}          # the generic kernels serve what the packed kernels exclude
        bm = 64 if kernel == T.TILE64 else 128
        assert (kernel == T.TILE128) == (M >= 256)
        assert tiles == cdiv(N, bm) * cdiv(M, bm) and blocks == tiles * splits
    else:
        pytest.fail(f'unknown kernel {kernel}')
