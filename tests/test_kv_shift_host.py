"""CPU checks of the shifted sliding window (mmd_kv_drop_shift): turning a key back composes with the rotation it was written with (the group property, which is what
makes the feature correct), the host statement (tests/kv_shift_oracle.py) is what it claims to be, kv_plan() with KV_F_SHIFT plans what DESIGN.md says over the span table
of tests/kv_drop_cases.py (through tests/kv_shift_plan_shim.cpp, built the way tests/test_kv_plan_host.py builds its shim) and plans what it always did without the flag,
the drop policy rounds to its quantum, and the new symbol is in the header and bound."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import kv_drop_cases as D
import kv_shift_oracle as S

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason='no host C++ compiler')

PI = Fraction('3.14159265358979323846264338327950288419716939937510582097494459')


def reduced(p, f):
    """the angle p * f (p an integer, f a float64, the product taken exactly) reduced into [-pi, pi] -> float64.  A float64 product p * f at p = 10^5 is already off by
    1e-11, more than the property is held to, so the reduction is done in rationals."""
    a = Fraction(int(p)) * Fraction(float(f))
    return float(a - round(a / (2 * PI)) * 2 * PI)


def written_at(x, p, freq):
    """the key a writer produces from x [d] at position p, in float64: x1 cos - x2 sin, x2 cos + x1 sin over the pairs (e, e + d/2)"""
    half = x.shape[-1] // 2
    a = np.array([reduced(p, f) for f in freq])
    c, s = np.cos(a), np.sin(a)
    return np.concatenate([x[:half] * c - x[half:] * s, x[half:] * c + x[:half] * s])


def turned_back(k, delta, freq):
    half = k.shape[-1] // 2
    a = np.array([reduced(delta, f) for f in freq])
    c, s = np.cos(a), np.sin(a)
    return np.concatenate([k[:half] * c + k[half:] * s, k[half:] * c - k[:half] * s])


def test_group_property():
    """a key written at p and turned back by delta is the key written at p - delta"""
    d = 128
    freq = 1.0 / 1000000.0 ** (np.arange(0, d, 2, dtype=np.float64) / d)          # Qwen2's table
    rng = np.random.default_rng(0)
    worst = 0.0
    for p, delta in [(1, 1), (64, 63), (4096, 49), (4145, 1024), (32768, 4096), (65537, 65000), (100000, 1), (100000, 31337), (100000, 99999), (100000, 100000)]:
        x = rng.standard_normal(d)
        err = np.abs(turned_back(written_at(x, p, freq), delta, freq) - written_at(x, p - delta, freq)).max()
        worst = max(worst, err)
        assert err <= 1e-12, (p, delta, err)
    print(f'group property: worst error {worst:.3g}')


def test_oracle_is_the_statement():
    """drop_shift deletes rows, leaves [0, from) and V alone, turns the rest back pair by pair with the fp32 angle, and keeps every pair's norm"""
    rng = np.random.default_rng(1)
    d, n = 16, 40
    inv = (1.0 / 10000.0 ** (np.arange(0, d, 2, dtype=np.float64) / d)).astype(np.float32)
    K, V = rng.standard_normal((2, 3, n, d)), rng.standard_normal((2, 3, n, d)).astype(np.float32)
    for frm, to in [(0, 7), (5, 6), (3, 40), (9, 9), (0, 40)]:
        Kn, Vn = S.drop_shift(K, V, frm, to, inv)
        keep = list(range(frm)) + list(range(to, n))
        assert Kn.shape == Vn.shape == (2, 3, len(keep), d) and Kn.dtype == np.float64 and Vn.dtype == np.float32
        assert np.array_equal(Vn, V[..., keep, :]) and np.array_equal(Kn[..., :frm, :], K[..., :frm, :])
        if frm == to:
            assert np.array_equal(Kn, K)
            continue
        for e in (0, 3, 7):          # the scalar formula
            a = float(np.float32(to - frm) * inv[e])
            x1, x2 = K[1, 2, to:, e], K[1, 2, to:, e + d // 2]
            assert np.allclose(Kn[1, 2, frm:, e], x1 * np.cos(a) + x2 * np.sin(a), rtol=0, atol=1e-15)
            assert np.allclose(Kn[1, 2, frm:, e + d // 2], x2 * np.cos(a) - x1 * np.sin(a), rtol=0, atol=1e-15)
        assert np.allclose(S.pair_norm(Kn[..., frm:, :]), S.pair_norm(K[..., to:, :]), rtol=1e-14, atol=0)
    # the angle is the fp32 product, not the float64 one
    assert S.angles(1000003, inv)[3] == float(np.float32(1000003) * inv[3]) != 1000003 * float(inv[3])
    # the bound's two terms
    assert S.U == {'bf16': 2.0 ** -8, 'fp32': 2.0 ** -23} and S.EVAL == 8 * 2.0 ** -24
    assert S.bound(np.array([2.0]), np.array([3.0]), 'bf16')[0] == 2.0 * 2.0 ** -8 + 3.0 * 8 * 2.0 ** -24


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------------------------
FIELDS_OF_A_DROP = ('nothing', 'launch', 't0', 't1', 'pitch_bytes', 'after_len', 'after_pos_off')
B7 = (28, 4, 128, 2)            # layers, kv heads, head_dim, element bytes
TINY32 = (2, 2, 16, 4)
CAP = 1 << 20


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('kv_shift_plan') / 'kv_shift_plan_shim.so')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', os.path.join(HERE, 'kv_shift_plan_shim.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.kvs_field_name.restype = lib.kvs_constant_name.restype = C.c_char_p
    lib.kvs_constant.restype = C.c_longlong
    lib.kvs_plan.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    fields = tuple(lib.kvs_field_name(i).decode() for i in range(lib.kvs_fields()))
    consts = {lib.kvs_constant_name(i).decode(): lib.kvs_constant(i) for i in range(lib.kvs_constants())}

    class Ask:
        K = consts

        @staticmethod
        def drop(geom, state, a, b, flags):
            """kv_plan(KV_DROP, ...); flags None: without the trailing argument -> (rc, {field: value}, message)"""
            out, err = (C.c_longlong * (1 + len(fields)))(), C.create_string_buffer(320)
            lib.kvs_plan(consts['KV_DROP'], (C.c_longlong * 4)(*geom), (C.c_longlong * 6)(*state), a, b, -1 if flags is None else flags, out, err, len(err))
            return out[0], dict(zip(fields, out[1:])), err.value.decode()
    return Ask


def state(n, pos_off=0, stash=(-1, -1)):
    return (n, pos_off, CAP, max(256, -(-n // 64) * 64), stash[0], stash[1])


@needs_cxx
def test_enums_did_not_move(shim):
    k = shim.K
    assert k['KV_OPS'] == 11 and k['KV_DROP'] == 4 and k['KV_LAUNCH_DROP'] == 3 and k['KV_CANON_SCATTER'] == 5
    assert k['KV_LAUNCH_DROP_SHIFT'] == k['KV_CANON_SCATTER'] + 1 and k['KV_F_SHIFT'] == 1
    assert (k['MMD_OK'], k['MMD_EINVAL'], k['MMD_ERANGE']) == (D.MMD_OK, D.MMD_EINVAL, D.MMD_ERANGE)


@needs_cxx
@pytest.mark.parametrize('geom', [B7, TINY32], ids=['bf16-d128', 'fp32-d16'])
@pytest.mark.parametrize('pos_off', [0, 777])
def test_plan_over_the_span_table(shim, geom, pos_off):
    k = shim.K
    pitch = CAP * geom[2] * geom[3]
    for frm, to, n in D.CASES:
        st = state(n, pos_off)
        rc0, p0, e0 = shim.drop(geom, st, frm, to, None)
        rc1, p1, e1 = shim.drop(geom, st, frm, to, 0)
        rcs, ps, es = shim.drop(geom, st, frm, to, k['KV_F_SHIFT'])
        assert (rc0, e0) == (rc1, e1) == (rcs, es) == (D.MMD_OK, ''), (frm, to, n)
        # without the flag: every field as before
        moves = frm != to and to != n
        want = dict(nothing=int(frm == to), launch=k['KV_LAUNCH_DROP'] if moves else k['KV_LAUNCH_NONE'], t0=frm if moves else 0, t1=to if moves else 0,
                    pitch_bytes=pitch if moves else 0, after_len=n - (to - frm), after_pos_off=pos_off + (to - frm))
        assert p0 == p1, (frm, to, n)
        assert {f: p0[f] for f in FIELDS_OF_A_DROP} == want, (frm, to, n)
        # with it: the new launch kind over the same span, the same length, the offset unchanged; nothing else differs
        want_s = dict(want, launch=k['KV_LAUNCH_DROP_SHIFT'] if moves else k['KV_LAUNCH_NONE'], after_pos_off=pos_off)
        assert {f: ps[f] for f in FIELDS_OF_A_DROP} == want_s, (frm, to, n)
        assert {f: v for f, v in ps.items() if f not in FIELDS_OF_A_DROP} == {f: v for f, v in p0.items() if f not in FIELDS_OF_A_DROP}
        assert ps['after_cap'] == st[2] and ps['after_mapped'] == st[3] and ps['after_stash_from'] == -1 and ps['reserve'] == 0 and ps['stash_bytes'] == 0


@needs_cxx
def test_plan_refuses_what_the_plain_drop_refuses(shim):
    k = shim.K
    cases = [(state(D.REFUSAL_LEN, 5), f, t, code) for (f, t), code in D.REFUSED_RANGES]
    cases += [(state(D.REFUSAL_LEN, 5, (60, 100)), f, t, D.MMD_EINVAL) for f, t in ((10, 20), (70, 80), (4, 4))]          # while a stash is held: whatever the span
    cases += [(state(D.REFUSAL_LEN, 0, (60, 100)), -1, 5, D.MMD_ERANGE)]          # the range is checked first
    for st, f, t, code in cases:
        plain, shifted = shim.drop(B7, st, f, t, 0), shim.drop(B7, st, f, t, k['KV_F_SHIFT'])
        assert plain[0] == shifted[0] == code and plain[2] == shifted[2] != '', (f, t, plain, shifted)          # the same code, the same message
        assert 'kv_drop' in plain[2]


@needs_cxx
def test_plan_refuses_an_unsupported_head_shape(shim):
    k = shim.K
    for geom in [(2, 2, 15, 2), (2, 2, 8, 2), (2, 2, 4, 4), (2, 2, 6, 4), (2, 2, 128, 1), (2, 2, 24, 2)]:          # odd; half a head below / not a multiple of 16 bytes; 1-byte elements
        st = state(100, 3)
        rc, _, err = shim.drop(geom, st, 10, 20, k['KV_F_SHIFT'])
        assert rc == D.MMD_EINVAL and 'kv_drop_shift' in err and 'not supported' in err, (geom, rc, err)
        assert shim.drop(geom, st, 200, 300, k['KV_F_SHIFT'])[0] == D.MMD_ERANGE          # behind the plain drop's own checks
    for geom in [(2, 2, 16, 2), (2, 2, 8, 4), (2, 2, 16, 4), (28, 4, 128, 2), (2, 2, 48, 2), (2, 2, 256, 4)]:
        assert shim.drop(geom, state(100, 3), 10, 20, k['KV_F_SHIFT'])[0] == D.MMD_OK, geom


# ---- the drop policy -----------------------------------------------------------------------------------------------------------------------------------------
def test_drop_amount_with_a_quantum():
    from mmduet_amd.inference import context_drop_amount
    for window, sink, rows in itertools.product((0, 64, 200, 1000), (0, 20, 63), (1, 49, 130)):
        for length in list(range(0, 300, 7)) + [window - rows, window - rows + 1, window, window + 5, 5000]:
            if length < sink or length < 0:
                continue
            m0 = context_drop_amount(length, rows, window, sink)
            assert context_drop_amount(length, rows, window, sink, 0) == m0 == context_drop_amount(length, rows, window, sink, quantum=0)
            for q in (1, 7, 49, 64, 1024):
                m = context_drop_amount(length, rows, window, sink, q)
                assert m0 <= m <= max(0, length - sink), (length, rows, window, sink, q, m)
                assert (m == 0) == (m0 == 0)          # a drop is never invented, and never rounded away
                if m0 > 0:
                    up = -(-m0 // q) * q
                    assert m == min(up, length - sink), (length, rows, window, sink, q, m)
                    assert m % q == 0 or m == length - sink          # a multiple, or the cap
    assert context_drop_amount(4145, 49, 4096, 20, 1024) == 1024 and context_drop_amount(4145, 49, 4096, 20) == 98
    assert context_drop_amount(500, 49, 400, 20, 1024) == 480          # capped at length - sink


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_in_the_header_and_bound():
    from mmduet_amd import _lib
    hdr = open(os.path.join(HERE, '..', 'include', 'mmduet.h')).read()
    assert 'int mmd_kv_drop_shift(mmd_stream* s, int64_t from, int64_t to);' in hdr
    assert 'int mmd_kv_drop(mmd_stream* s, int64_t from, int64_t to);' in hdr
    assert 'mmd_kv_drop_shift' in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGS['mmd_kv_drop_shift'] == _lib._SIGS['mmd_kv_drop'] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int64])
    lib = _lib.lib()          # dlopen + symbol check: raises when the library does not export it
    assert lib.mmd_kv_drop_shift(None, 0, 0) == D.MMD_EINVAL          # the null stream, without a GPU
    import inspect
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM as M
    assert inspect.signature(M.kv_drop).parameters['shift'].default is False


def test_cli_flags_and_driver_attributes():
    """--context_positions / --context_drop_quantum are parsed by the CLI's own parser, and the names it produces are the ones the driver reads"""
    from mmduet_amd.__main__ import cli_extra_args
    ns = cli_extra_args(['--llm_pretrained', 'x', '--context_window', '4096', '--context_positions', 'shifted', '--context_drop_quantum', '1024'])
    assert (ns.context_window, ns.context_positions, ns.context_drop_quantum) == (4096, 'shifted', 1024)
    ns = cli_extra_args(['--context_window', '4096'])
    assert (ns.context_positions, ns.context_drop_quantum) == ('kept', 0)
    with pytest.raises(SystemExit):
        cli_extra_args(['--context_positions', 'rotated'])
    src = open(os.path.join(HERE, '..', 'mmduet_amd', 'inference.py')).read()
    assert re.search(r"getattr\(args, 'context_positions'", src) and re.search(r"getattr\(args, 'context_drop_quantum'", src)
