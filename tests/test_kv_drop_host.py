"""CPU checks of the sliding context window: the host statement of mmd_kv_drop (tests/kv_drop_cases.py) is what it claims to be, its case list covers every class
the kernel distinguishes, the refusals are listed, the two symbols are bound, and the drivers' drop policy never leaves a forward past the window."""
import itertools
import torch
import kv_layout as L
import kv_drop_cases as D


def test_host_statement_deletes_token_rows_through_the_layout():
    """expected_arena on an arena whose every element names its (head, token, dim): what is left is tokens [0, from) + [to, len) in order, and V went through the
    64-token-block layout and back"""
    nkv, d, m = 2, 8, 256
    K = (torch.arange(nkv)[:, None, None] * 1_000_000 + torch.arange(m)[None, :, None] * 100 + torch.arange(d)[None, None, :]).contiguous()
    V_raw = L.v_raw(K + 50)
    for frm, to, n in [(0, 1, 2), (5, 6, 200), (63, 65, 250), (64, 128, 256), (1, 130, 131), (60, 63, 64), (17, 17, 100), (10, 50, 50)]:
        k, v = D.expected_arena(K, V_raw, frm, to, n)
        keep = list(range(0, frm)) + list(range(to, n))
        assert k.shape == v.shape == (nkv, n - (to - frm), d)
        assert k[1, :, 0].tolist() == [1_000_000 + 100 * t for t in keep]
        assert torch.equal(v, k + 50)
        flat = V_raw.reshape(nkv, -1)
        for t in keep[:3] + keep[-3:]:          # the same rows through the scalar formula
            assert v[0, keep.index(t), 5] == flat[0, L.v_index(t, 5, d)], t


def test_case_list_covers_every_class():
    seen = set().union(*(D.classes(c) for c in D.CASES))
    assert seen == D.ALL_CLASSES, D.ALL_CLASSES - seen
    assert all(c in D.CASES for c in D.REQUIRED + D.OVERLAPPING)
    assert D.REQUIRED == [(0, 1, 2), (5, 6, 200), (63, 65, 257), (64, 128, 300), (1, 130, 131), (60, 63, 64), (7, 71, 500)]
    assert D.OVERLAPPING == [(3, 4, 4099), (100, 149, 70000)]
    assert all(0 <= f <= t <= n for f, t, n in D.CASES)
    moving = [c for c in D.CASES if D.delta(c) and D.behind(c)]
    # `from`, `to` and delta on every residue mod 8 (a 16-byte group of a V line holds 8 bf16 tokens: delta % 8 is the funnel's shift, from % 8 the partly kept group)
    assert {c[0] % 8 for c in moving} == set(range(8))
    assert {c[1] % 8 for c in moving} == set(range(8))
    assert {D.delta(c) % 8 for c in moving} == set(range(8))
    assert {D.delta(c) % 4 for c in moving} == set(range(4))          # ... 4 fp32 tokens
    # `from` and `to` just below, on and just above a block edge
    assert {c[0] % 64 for c in moving} >= {0, 1, 63} and {c[1] % 64 for c in moving} >= {0, 1, 63}
    # overlapping moves that run over themselves many times, and one whose source starts inside the destination's first block
    assert any(D.behind(c) > 1000 * D.delta(c) for c in moving)
    assert any(D.delta(c) < 64 and c[0] // 64 == c[1] // 64 and D.behind(c) > 64 for c in moving)
    # more tokens behind the span than one block's walk covers in a tile (4 blocks of 64), and fewer than one 16-byte group
    assert any(D.behind(c) > 256 for c in moving) and any(D.behind(c) < 4 for c in moving)
    assert sum(c[2] >= D.BIG_LEN for c in D.CASES) == 1


def test_composition_of_two_drops_is_one_deletion_of_both_spans():
    x = torch.arange(300)[None, :, None].expand(1, 300, 2)
    once = D.drop_rows(D.drop_rows(x, 63, 65, 257), 10, 100)
    assert once[0, :, 0].tolist() == [t for t in range(257) if not (63 <= t < 65) and not (10 <= (t if t < 63 else t - 2) < 100)]


def test_refusal_list():
    for (f, t), code in D.REFUSED_RANGES:
        assert code == D.MMD_ERANGE and not (0 <= f <= t <= D.REFUSAL_LEN), (f, t)
    kinds = {('from<0' if f < 0 else 'to<from' if t < f else 'to>len') for (f, t), _ in D.REFUSED_RANGES}
    assert kinds == {'from<0', 'to<from', 'to>len'}
    import re, os
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'mmduet.h')).read()
    assert int(re.search(r'#define MMD_EINVAL \((-?\d+)\)', hdr).group(1)) == D.MMD_EINVAL
    assert int(re.search(r'#define MMD_ERANGE \((-?\d+)\)', hdr).group(1)) == D.MMD_ERANGE
    assert 'int mmd_kv_drop(mmd_stream* s, int64_t from, int64_t to);' in hdr and 'int64_t mmd_kv_position(const mmd_stream* s);' in hdr


def test_symbols_are_bound():
    import ctypes as C
    from mmduet_amd import _lib
    assert 'mmd_kv_drop' in _lib.EXPORTED_SYMBOLS and 'mmd_kv_position' in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGS['mmd_kv_drop'] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int64])
    assert _lib._SIGS['mmd_kv_position'] == (C.c_int64, [C.c_void_p])
    lib = _lib.lib()          # dlopen + symbol check: raises when the library does not export one of them
    assert lib.mmd_kv_drop(None, 0, 0) == D.MMD_EINVAL and lib.mmd_kv_position(None) == -1          # the null stream, without a GPU
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM as M
    assert callable(M.kv_drop) and callable(M.kv_position)


def test_drop_policy_never_leaves_a_forward_past_the_window():
    from mmduet_amd.inference import context_drop_amount
    for window, sink, rows in itertools.product((0, 1, 64, 200, 1000), (0, 1, 20, 63), (1, 7, 49, 130)):
        for length in list(range(0, 300, 7)) + [window - rows, window - rows + 1, window, window + 5, 5000]:
            if length < sink or length < 0:
                continue
            m = context_drop_amount(length, rows, window, sink)
            assert m == D.drop_amount_reference(length, rows, window, sink), (length, rows, window, sink, m)
            assert 0 <= m <= length - sink
            if window <= 0:
                assert m == 0          # off
            elif window >= sink + rows:
                assert length - m + rows <= window, (length, rows, window, sink, m)
            if m > 0:
                assert length - (m - 1) + rows > window          # the smallest amount
