"""CPU checks of mmd_kv_drop_spans: the case table (tests/kv_spans_cases.py) covers every class the kernels distinguish; kv_plan_spans() (through
tests/kv_spans_plan_shim.cpp, built the way tests/test_kv_plan_host.py builds its shim) refuses, normalises, cuts into segments, groups and books what the issue
states, and plans for one span what KV_DROP plans; and a host simulation of the owner walk -- tile by tile "all loads, then all stores", K in both forms and V through
its 64-token block layout, the planned launches in their order -- leaves exactly the host statement.  The simulation's tile sizes are the kernels' own
(KVD_THREADS * KVD_U = 1024 16-byte groups per tile: 1024 / ku tokens of K, 512 / kp tokens of shifted K, nb = 1024 / (ep * 64 / VEC) blocks of V), for the two
head shapes the GPU tests run: bf16 d 128 and fp32 d 16."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import kv_drop_cases as D
import kv_layout as L
import kv_spans_cases as S

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason='no host C++ compiler')
B7 = (28, 4, 128, 2)            # layers, kv heads, head_dim, element bytes
TINY32 = (2, 2, 16, 4)
CAP = 1 << 20
CASE_IDS = [f'{len(sp)}spans-of-{n}-{i}' for i, (sp, n) in enumerate(S.CASES)]


def test_case_list_covers_every_class():
    seen = set().union(*(S.classes(c) for c in S.CASES))
    assert seen == S.ALL_CLASSES, S.ALL_CLASSES ^ seen
    assert [c for c in S.CASES if len(c[0]) == 1][:len(D.REQUIRED)] == [([(f, t)], n) for f, t, n in D.REQUIRED]
    assert ([(8, 9), (10, 11), (12, 13), (14, 20)], 200) in S.CASES
    assert {len(S.normalise(sp)) for sp, _ in S.CASES} >= {1, 2, 20, 64, 65, 70}
    for sp, n in S.CASES:
        assert all(0 <= a <= b <= n for a, b in sp) and all(p[1] <= q[0] for p, q in zip(sp, sp[1:]))
    # fp32 groups hold 4 tokens: a group from three segments, and every residue of delta mod 4, are among the above
    segs = [s for c in S.CASES for s in S.segments(*c)]
    assert {s[3] % 4 for s in segs} == set(range(4))
    kinds = {code for _, code in S.REFUSED}
    assert kinds == {S.MMD_EINVAL, S.MMD_ERANGE}


def test_host_statement_deletes_token_rows():
    import torch
    nkv, d, m = 2, 8, 256
    K = (torch.arange(nkv)[:, None, None] * 1_000_000 + torch.arange(m)[None, :, None] * 100 + torch.arange(d)[None, None, :]).contiguous()
    V_raw = L.v_raw(K + 50)
    for spans, n in [([(5, 6), (20, 21)], 200), ([(0, 5), (9, 12)], 100), ([(5, 5), (10, 20), (20, 30)], 120), ([(0, 128)], 128), ([], 50)]:
        k, v = S.expected_arena(K, V_raw, spans, n)
        keep = S.kept(spans, n)
        assert k.shape == v.shape == (nkv, len(keep), d) and len(keep) == n - sum(b - a for a, b in spans)
        assert k[1, :, 0].tolist() == [1_000_000 + 100 * t for t in keep]
        assert torch.equal(v, k + 50)
    # the segments of the Python plan are the kept tokens, and every launch list composes to them
    for spans, n in S.CASES:
        keep = S.kept(spans, n)
        segs = S.segments(spans, n)
        first = S.normalise(spans)[0][0] if S.normalise(spans) else n
        assert [t for src, count, _, _ in segs for t in range(src, src + count)] == keep[first:]
        assert all(d1 > d0 >= 1 for (_, _, _, d0), (_, _, _, d1) in zip(segs, segs[1:])) and all(s[3] >= 1 for s in segs)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('kv_spans_plan') / 'kv_spans_plan_shim.so')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', os.path.join(HERE, 'kv_spans_plan_shim.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.kvsp_constant_name.restype = C.c_char_p
    lib.kvsp_constant.restype = C.c_longlong
    lib.kvsp_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    lib.kvsp_drop.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    consts = {lib.kvsp_constant_name(i).decode(): lib.kvsp_constant(i) for i in range(lib.kvsp_constants())}
    HW, LW, MAXL = lib.kvsp_head_words(), lib.kvsp_launch_words(), 8
    head_names = ('rc', 'nothing', 'launch', 'pitch_bytes', 'spans', 'dropped', 'launches', 'after_len', 'after_pos_off', 'after_cap', 'after_mapped', 'after_stash_from', 'after_stash_to')
    assert HW == len(head_names)

    class Ask:
        K = consts

        @staticmethod
        def spans(geom, state, spans, flags, n=None, null=False):
            """-> ({head field: value}, [(dst0, len_in, len_end, [(src, count)])], message)"""
            flat = [x for sp in spans for x in sp]
            arr = (C.c_longlong * max(1, len(flat)))(*flat)
            head, out, err = (C.c_longlong * HW)(), (C.c_longlong * (LW * MAXL))(), C.create_string_buffer(320)
            got = lib.kvsp_plan((C.c_longlong * 4)(*geom), (C.c_longlong * 6)(*state), None if null else arr, len(spans) if n is None else n, flags, head, out, MAXL, err, len(err))
            assert got <= MAXL
            ls = []
            for i in range(got):
                o = out[i * LW:(i + 1) * LW]
                assert all(x == 0 for x in o[4 + 2 * o[3]:])
                ls.append((o[0], o[1], o[2], [(o[4 + 2 * j], o[5 + 2 * j]) for j in range(o[3])]))
            return dict(zip(head_names, head)), ls, err.value.decode()

        @staticmethod
        def drop(geom, state, a, b, flags):
            out, err = (C.c_longlong * 8)(), C.create_string_buffer(320)
            lib.kvsp_drop((C.c_longlong * 4)(*geom), (C.c_longlong * 6)(*state), a, b, flags, out, err, len(err))
            return dict(zip(('rc', 'nothing', 'launch', 't0', 't1', 'pitch_bytes', 'after_len', 'after_pos_off'), out)), err.value.decode()
    return Ask


def state(n, pos_off=0, stash=(-1, -1)):
    return (n, pos_off, CAP, max(256, -(-n // 64) * 64), stash[0], stash[1])


@needs_cxx
def test_constants(shim):
    k = shim.K
    assert k['KV_OPS'] == 11 and k['KV_DROP'] == 4 and k['KV_DROP_SPANS'] > k['KV_OPS']          # kv_plan()'s operations did not move
    assert k['KV_SPANS_PER_LAUNCH'] == S.PER_LAUNCH == 64
    assert len({k['KV_LAUNCH_NONE'], k['KV_LAUNCH_DROP'], k['KV_LAUNCH_DROP_SHIFT'], k['KV_LAUNCH_COMPACT'], k['KV_LAUNCH_COMPACT_SHIFT']}) == 5
    assert (k['MMD_OK'], k['MMD_EINVAL'], k['MMD_ERANGE']) == (S.MMD_OK, S.MMD_EINVAL, S.MMD_ERANGE)


@needs_cxx
@pytest.mark.parametrize('geom', [B7, TINY32], ids=['bf16-d128', 'fp32-d16'])
@pytest.mark.parametrize('pos_off', [0, 777])
def test_plan_over_the_case_table(shim, geom, pos_off):
    k = shim.K
    pitch = CAP * geom[2] * geom[3]
    for spans, n in S.CASES:
        st = state(n, pos_off)
        for flags in (0, k['KV_F_SHIFT']):
            h, ls, err = shim.spans(geom, st, spans, flags)
            assert (h['rc'], err) == (S.MMD_OK, ''), (spans, n)
            ns = S.normalise(spans)
            total = sum(b - a for a, b in ns)
            if not ns:
                assert h['nothing'] == 1 and ls == [] and h['launch'] == k['KV_LAUNCH_NONE'] and (h['after_len'], h['after_pos_off']) == (n, pos_off)
                continue
            want = S.launches(spans, n)
            assert ls == want, (spans, n)
            assert h['nothing'] == 0 and h['spans'] == len(ns) and h['dropped'] == total and h['launches'] == len(want)
            assert h['launch'] == (k['KV_LAUNCH_NONE'] if not want else k['KV_LAUNCH_COMPACT_SHIFT'] if flags else k['KV_LAUNCH_COMPACT'])
            assert h['pitch_bytes'] == (pitch if want else 0)
            # the bookkeeping afterwards
            assert h['after_len'] == n - total and h['after_pos_off'] == (pos_off if flags else pos_off + total)
            assert (h['after_cap'], h['after_mapped'], h['after_stash_from'], h['after_stash_to']) == (st[2], st[3], -1, -1)
            # each launch: at most 64 segments, strictly growing delta >= 1, ending at the length it starts from; groups highest first, each a complete compaction
            cur = n
            for dst0, len_in, len_end, segs in ls:
                assert 1 <= len(segs) <= 64 and len_in == cur
                dst, deltas = dst0, []
                for src, count in segs:
                    assert count > 0
                    deltas.append(src - dst); dst += count
                assert deltas[0] >= 1 and all(b > a for a, b in zip(deltas, deltas[1:]))
                assert segs[-1][0] + segs[-1][1] in (len_in, ns[-1][0]) and dst == len_end          # (up to the length, or to a last span that ends there)
                cur = len_end
            assert [l[0] for l in ls] == sorted((l[0] for l in ls), reverse=True)
            assert (cur == n - total) or not want


@needs_cxx
def test_one_span_plans_what_kv_drop_plans(shim):
    k = shim.K
    for geom in (B7, TINY32):
        for frm, to, n in D.CASES:
            for flags in (0, k['KV_F_SHIFT']):
                st = state(n, 5)
                h, ls, err = shim.spans(geom, st, [(frm, to)], flags)
                d, derr = shim.drop(geom, st, frm, to, flags)
                assert h['rc'] == d['rc'] == S.MMD_OK and err == derr == ''
                assert (h['nothing'], h['after_len'], h['after_pos_off']) == (d['nothing'], d['after_len'], d['after_pos_off'])
                moves = d['launch'] != k['KV_LAUNCH_NONE']
                assert bool(ls) == moves and h['pitch_bytes'] == d['pitch_bytes']
                if moves:          # the same move: tokens [t1, len) down to t0
                    assert d['launch'] == (k['KV_LAUNCH_DROP_SHIFT'] if flags else k['KV_LAUNCH_DROP'])
                    assert ls == [(d['t0'], n, d['after_len'], [(d['t1'], n - d['t1'])])]


@needs_cxx
def test_plan_refusals(shim):
    k = shim.K
    n = S.REFUSAL_LEN
    for flags in (0, k['KV_F_SHIFT']):
        for spans, code in S.REFUSED:
            h, ls, err = shim.spans(B7, state(n, 5), spans, flags)
            assert h['rc'] == code and ls == [] and 'kv_drop_spans' in err, (spans, h, err)
            assert (h['after_len'], h['after_pos_off']) == (n, 5)
            if code == S.MMD_ERANGE:
                assert f'outside the context ({n} tokens)' in err
            else:
                assert 'ascend' in err
        # a stash is held: whatever the spans; the range is checked first
        for spans in ([(10, 20)], [(70, 80), (90, 95)], [(4, 4)], []):
            h, _, err = shim.spans(B7, state(n, 5, (60, 100)), spans, flags)
            assert h['rc'] == S.MMD_EINVAL and 'stashed' in err and '[60, 100)' in err
        assert shim.spans(B7, state(n, 0, (60, 100)), [(-1, 5)], flags)[0]['rc'] == S.MMD_ERANGE
        # no list
        assert shim.spans(B7, state(n), [], flags, n=-1)[0]['rc'] == S.MMD_EINVAL
        assert shim.spans(B7, state(n), [], flags, n=2, null=True)[0]['rc'] == S.MMD_EINVAL
        h, ls, _ = shim.spans(B7, state(n), [], flags, n=0, null=True)
        assert h['rc'] == S.MMD_OK and h['nothing'] == 1 and ls == []
    # the shifted form's head shapes: KV_DROP's refusal, word for word
    for geom in [(2, 2, 15, 2), (2, 2, 8, 2), (2, 2, 4, 4), (2, 2, 128, 1)]:
        h, _, err = shim.spans(geom, state(100, 3), [(10, 20), (30, 40)], k['KV_F_SHIFT'])
        d, derr = shim.drop(geom, state(100, 3), 10, 20, k['KV_F_SHIFT'])
        assert h['rc'] == d['rc'] == S.MMD_EINVAL and err == derr and 'not supported' in err
        assert shim.spans(geom, state(100, 3), [(10, 20), (30, 40)], 0)[0]['rc'] == S.MMD_OK


# ---- the walk, simulated -------------------------------------------------------------------------------------------------------------------------------------
# (VEC tokens per 16-byte group, K tile in tokens, shifted K tile in tokens, V blocks per tile) as launch_kv_compact derives them
SHAPES = {'bf16-d128': (8, 1024 // 8, 512 // 4, 1024 // (32 * 8)), 'fp32-d16': (4, 1024 // 4, 512 // 2, 1024 // (4 * 16))}


def seg_tables(dst0, segs):
    dst = [dst0]
    for _, count in segs:
        dst.append(dst[-1] + count)
    return dst, [src - d for (src, _), d in zip(segs, dst)]


def seg_of(dst, t):
    i = 0
    while i + 2 < len(dst) and t >= dst[i + 1]:
        i += 1
    return i


def walk_k_plain(A, launch, tile):
    dst0, _, _, segs = launch
    dst, delta = seg_tables(dst0, segs)
    for t0 in range(dst0, dst[-1], tile):
        ts = range(t0, min(t0 + tile, dst[-1]))
        loaded = [A[t + delta[seg_of(dst, t)]] for t in ts]          # all loads ...
        for t, v in zip(ts, loaded):                                 # ... then all stores
            A[t] = v


def walk_k_shifted(A, R, launch, tile):
    """A: the token in each slot, R: the positions it was turned back by so far.  A tile never crosses a segment."""
    dst0, _, _, segs = launch
    dst, delta = seg_tables(dst0, segs)
    for i, (src, count) in enumerate(segs):
        for t0 in range(0, count, tile):
            ts = range(t0, min(t0 + tile, count))
            loaded = [(A[src + t], R[src + t]) for t in ts]
            for t, (a, r) in zip(ts, loaded):
                A[dst[i] + t] = a; R[dst[i] + t] = r + delta[i]


def walk_v(F, launch, vec, nb, d, e):
    """F: one head's V row as stored (flat, transposed 64-token blocks); the owner of dim e walks its groups"""
    dst0, _, _, segs = launch
    dst, delta = seg_tables(dst0, segs)
    dend = dst[-1]
    at = lambda t: L.v_index(t, e, d)
    for b0 in range(dst0 >> 6, -(-dend // 64), nb):
        stores = []
        for t in range(b0 * 64, (b0 + nb) * 64, vec):          # the tile's destination groups
            if not (t + vec > dst0 and t < dend):
                continue
            i = seg_of(dst, t)
            if t >= dst0 and t + vec <= dst[i + 1]:          # two aligned loads and a funnel
                s0 = (t + delta[i]) // vec * vec
                sh = delta[i] % vec
                two = [F[at(s0 + k)] for k in range(vec)] + ([F[at(s0 + vec + k)] for k in range(vec)] if sh else [None] * vec)
                stores += [(t + k, two[sh + k]) for k in range(vec)]
            else:                                            # element by element, inside [dst0, dend) only
                for tk in range(max(t, dst0), min(t + vec, dend)):
                    stores.append((tk, F[at(tk + delta[seg_of(dst, tk)])]))
        for t, v in stores:
            assert v is not None
            F[at(t)] = v


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('case', S.CASES, ids=CASE_IDS)
def test_simulated_walk_leaves_the_statement(case, shape):
    spans, n = case
    vec, ktile, stile, nb = SHAPES[shape]
    slots = -(-n // 64) * 64 + 64
    keep = S.kept(spans, n)
    first = S.normalise(spans)[0][0] if S.normalise(spans) else n
    gone_below = np.cumsum(np.isin(np.arange(n), keep, invert=True))          # tokens dropped at or below each old slot
    # K, plain and shifted
    A = list(range(slots)); B = list(range(slots)); R = [0] * slots
    d, e = 2, 1
    F = [None] * (slots * d)
    for t in range(slots):
        F[L.v_index(t, e, d)] = t; F[L.v_index(t, 0, d)] = -1 - t
    newlen = n
    for launch in S.launches(spans, n):
        assert launch[1] == newlen
        walk_k_plain(A, launch, ktile)
        walk_k_shifted(B, R, launch, stile)
        walk_v(F, launch, vec, nb, d, e)
        newlen = launch[2]
    newlen = len(keep)
    assert A[:newlen] == keep and B[:newlen] == keep
    assert R[:newlen] == [int(gone_below[t]) for t in keep]          # every key turned back by exactly the tokens dropped in front of it
    assert R[:first] == [0] * first
    got_v = [F[L.v_index(t, e, d)] for t in range(slots)]
    assert got_v[:newlen] == keep
    assert [F[L.v_index(t, 0, d)] for t in range(slots)] == [-1 - t for t in range(slots)]          # another owner's dim is not touched
    assert all(v is not None and 0 <= v < slots for v in got_v)                                      # whatever lies behind the new length is a copy of an arena slot
    assert A[n:] == list(range(n, slots)) and got_v[n:] == list(range(n, slots))                      # nothing at or above the old length is written


def test_simulation_catches_a_wrong_order():
    """the same walk with the launches of a grouped plan issued lowest group first does NOT give the statement: the simulation can tell"""
    spans, n = S.every(5, 2, 3, 70), 420
    A = list(range(512))
    ls = S.launches(spans, n)
    assert len(ls) == 2
    for launch in reversed(ls):
        walk_k_plain(A, launch, 128)
    assert A[:len(S.kept(spans, n))] != S.kept(spans, n)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_in_the_header_and_bound():
    from mmduet_amd import _lib
    hdr = open(os.path.join(HERE, '..', 'include', 'mmduet.h')).read()
    assert 'int mmd_kv_drop_spans(mmd_stream* s, const int64_t* spans_host /* [n][2] */, int n, int shift);' in hdr
    assert 'mmd_kv_drop_spans' in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGS['mmd_kv_drop_spans'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int])
    lib = _lib.lib()          # dlopen + symbol check: raises when the library does not export it
    one = (C.c_int64 * 2)(0, 1)
    assert lib.mmd_kv_drop_spans(None, C.cast(one, C.c_void_p), 1, 0) == S.MMD_EINVAL          # the null stream, without a GPU
    import inspect
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM as M
    assert inspect.signature(M.kv_drop_many).parameters['shift'].default is False
