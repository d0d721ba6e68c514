"""CPU checks of stream snapshots: the host statement of the canonical form (tests/kv_snapshot_cases.py) is kv_layout's, a KVSnapshot round-trips through state_dict
and torch.save bit for bit, mismatches are named, the chunking arithmetic covers [0, n) exactly once, and the four symbols are bound."""
import ctypes as C
import os
import re
import pytest
import torch
import kv_layout as L
import kv_snapshot_cases as S
from mmduet_amd.modeling_live import KVSnapshot, snapshot_chunks, VideoHeadLiveLlavaQwenForCausalLM as M

BF = torch.bfloat16


def test_canonical_form_is_the_layouts_logical_view():
    """on an arena image whose every element names its (head, token, dim): the canonical tensors of the case table's spans are v_logical of the raw image, sliced --
    and, element by element, the scalar formula v_index"""
    nkv, d, m = 2, 8, S.up64(S.CTX_LEN)
    K, V_raw = S.labelled_arena(nkv, m, d)
    flat = V_raw.reshape(nkv, -1)
    for frm, to in S.EXPORT_SPANS:
        k, v = S.canonical(K, V_raw, frm, to)
        assert k.shape == v.shape == (nkv, to - frm, d)
        assert torch.equal(v, L.v_logical(V_raw)[:, frm:to]) and torch.equal(k, K[:, frm:to])
        assert torch.equal(v, k + 50)
        assert k[1, :, 3].tolist() == [1_000_000 + 100 * t + 3 for t in range(frm, to)]
        for t in sorted({frm, (frm + to) // 2, to - 1} & set(range(frm, to))):
            for e in (0, 5, d - 1):
                assert v[1, t - frm, e] == flat[1, L.v_index(t, e, d)], (frm, to, t, e)


def test_import_statement_changes_the_span_only():
    """imported(): slots [at, at + n) take the canonical rows, every other element of the raw image -- the older tokens of a shared V block included -- is as it was;
    two pieces equal one piece"""
    nkv, d, m = 2, 8, 256
    K, V_raw = S.labelled_arena(nkv, m, d)
    Kc, Vc = -K[:, :S.CTX_LEN] - 7, -K[:, :S.CTX_LEN] - 9
    whole = S.imported(K, V_raw, 0, Kc, Vc)
    assert torch.equal(whole[0][:, :S.CTX_LEN], Kc) and torch.equal(L.v_logical(whole[1])[:, :S.CTX_LEN], Vc)
    assert torch.equal(whole[0][:, S.CTX_LEN:], K[:, S.CTX_LEN:]) and torch.equal(L.v_logical(whole[1])[:, S.CTX_LEN:], L.v_logical(V_raw)[:, S.CTX_LEN:])
    for s in S.IMPORT_SPLITS:
        first = S.imported(K, V_raw, 0, Kc[:, :s], Vc[:, :s])
        changed = (first[1] != V_raw).reshape(nkv, -1)
        want = torch.zeros_like(changed)
        for t in range(s):
            for e in range(d):
                want[:, L.v_index(t, e, d)] = True
        assert torch.equal(changed, want), s
        both = S.imported(*first, s, Kc[:, s:], Vc[:, s:])
        assert torch.equal(both[0], whole[0]) and torch.equal(both[1], whole[1]), s


def test_case_table():
    assert S.EXPORT_SPANS == [(0, 200), (0, 1), (63, 65), (64, 128), (1, 199), (130, 131), (199, 200), (70, 70)]
    assert S.IMPORT_SPLITS == [1, 63, 64, 65, 130] and S.FORK_LENGTHS == [1, 64, 65, 200] and S.CTX_LEN == 200
    assert all(0 <= f <= t <= S.CTX_LEN for f, t in S.EXPORT_SPANS)
    for (f, t), code in S.REFUSED_EXPORTS:
        assert code == S.MMD_ERANGE and not (0 <= f <= t <= S.CTX_LEN)
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'mmduet.h')).read()
    assert int(re.search(r'#define MMD_EINVAL \((-?\d+)\)', hdr).group(1)) == S.MMD_EINVAL
    assert int(re.search(r'#define MMD_ERANGE \((-?\d+)\)', hdr).group(1)) == S.MMD_ERANGE
    for decl in ('int mmd_kv_export(mmd_stream* s, int64_t from, int64_t to, void* K_out, void* V_out);',
                 'int mmd_kv_import(mmd_stream* s, const void* K_in, const void* V_in, int64_t n);',
                 'int mmd_kv_set_position(mmd_stream* s, int64_t position);',
                 'int mmd_kv_fork(mmd_stream* dst, const mmd_stream* src, int64_t n);'):
        assert decl in hdr, decl


def test_symbols_are_bound():
    from mmduet_amd import _lib
    I, I64, VP = C.c_int, C.c_int64, C.c_void_p
    assert _lib._SIGS['mmd_kv_export'] == (I, [VP, I64, I64, VP, VP])
    assert _lib._SIGS['mmd_kv_import'] == (I, [VP, VP, VP, I64])
    assert _lib._SIGS['mmd_kv_set_position'] == (I, [VP, I64])
    assert _lib._SIGS['mmd_kv_fork'] == (I, [VP, VP, I64])
    lib = _lib.lib()          # dlopen + symbol check: raises when the library does not export one of them
    # the null stream, without a GPU
    assert lib.mmd_kv_export(None, 0, 0, None, None) == S.MMD_EINVAL and lib.mmd_kv_import(None, None, None, 0) == S.MMD_EINVAL
    assert lib.mmd_kv_set_position(None, 0) == S.MMD_EINVAL and lib.mmd_kv_fork(None, None, 0) == S.MMD_EINVAL
    assert callable(M.kv_save) and callable(M.kv_load) and callable(M.kv_fork)


def make_snapshot(dtype, n=70, layers=2, nkv=3, d=16, position=None):
    g = torch.Generator().manual_seed(n + d)
    K = torch.randn(layers, nkv, n, d, generator=g).to(dtype)
    V = torch.randn(layers, nkv, n, d, generator=g).to(dtype)
    return KVSnapshot(K, V, n + 41 if position is None else position, dtype, layers, nkv, d, L.inv_freq(d))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_snapshot(a, b):
    return (a.dtype == b.dtype and a.position == b.position and (a.layers, a.kv_heads, a.head_dim) == (b.layers, b.kv_heads, b.head_dim) and a.length == b.length
            and torch.equal(bits(a.K), bits(b.K)) and torch.equal(bits(a.V), bits(b.V)) and torch.equal(bits(a.inv_freq), bits(b.inv_freq)))


@pytest.mark.parametrize('dtype', [BF, torch.float32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('n', [70, 0])
def test_snapshot_round_trips_bit_for_bit(tmp_path, dtype, n):
    s = make_snapshot(dtype, n)
    assert len(s) == s.length == n and s.position == n + 41
    sd = s.state_dict()
    assert all(isinstance(v, (torch.Tensor, int)) for v in sd.values()), {k: type(v) for k, v in sd.items()}          # plain tensors and ints
    assert same_snapshot(KVSnapshot.from_state_dict(sd), s)
    p = str(tmp_path / 'ctx.pt')
    torch.save(sd, p)
    assert same_snapshot(KVSnapshot.from_state_dict(torch.load(p)), s)
    s.save(p)
    assert same_snapshot(KVSnapshot.load(p), s)


def test_mismatches_raise_naming_the_field():
    s = make_snapshot(BF)
    inv = L.inv_freq(16)
    s.check_against(BF, 2, 3, 16, inv)                                   # its own geometry: accepted
    for field, args in [('dtype', (torch.float32, 2, 3, 16, inv)), ('layers', (BF, 4, 3, 16, inv)), ('kv_heads', (BF, 2, 4, 16, inv)),
                        ('head_dim', (BF, 2, 3, 32, L.inv_freq(32))), ('inv_freq', (BF, 2, 3, 16, L.inv_freq(16, theta=1e4)))]:
        with pytest.raises(ValueError, match=field):
            s.check_against(*args)
    one_ulp = inv.clone(); one_ulp.view(torch.int32)[3] += 1               # the table is compared bit for bit
    with pytest.raises(ValueError, match='inv_freq'):
        s.check_against(BF, 2, 3, 16, one_ulp)
    # a snapshot that contradicts itself is refused where it is built
    with pytest.raises(ValueError, match='shape'):
        KVSnapshot(s.K, s.V[:, :, :5], 100, BF, 2, 3, 16, inv)
    with pytest.raises(ValueError, match='shape'):
        KVSnapshot(s.K.float(), s.V, 100, BF, 2, 3, 16, inv)
    with pytest.raises(ValueError, match='position'):
        KVSnapshot(s.K, s.V, s.length - 1, BF, 2, 3, 16, inv)
    sd = s.state_dict(); sd['format'] = 99
    with pytest.raises(ValueError, match='format'):
        KVSnapshot.from_state_dict(sd)


@pytest.mark.parametrize('n', [0, 1, 63, 200, 16384])
def test_chunks_cover_the_context_exactly_once(n):
    token_bytes = 2 * 28 * 4 * 128 * 2          # K and V of one token of the 7B shape in bf16
    counts = {}
    for name, frac in S.CHUNK_BUDGETS:
        budget = int(max(n, 1) * token_bytes * frac)
        chunks = snapshot_chunks(n, token_bytes, budget)
        counts[name] = len(chunks)
        covered = [t for a, b in chunks for t in range(a, b)]
        assert covered == list(range(n)), (n, name)                       # in order, no gap, nothing twice
        assert all(a < b for a, b in chunks)
        per = max(1, budget // token_bytes)
        assert all(b - a <= per for a, b in chunks) and all((b - a) * token_bytes <= budget for a, b in chunks if per > 1 or budget >= token_bytes)
    if n >= 200:
        assert counts['one'] == 1 and counts['two'] == 2 and counts['many'] >= 3 and counts['below one token'] == n, counts
    if n == 1:
        assert counts == {k: 1 for k in counts}
    if n == 0:
        assert counts == {k: 0 for k in counts}
    assert snapshot_chunks(5, token_bytes, 0) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
