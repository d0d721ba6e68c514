"""Stream snapshots stated on the host, for tests/test_kv_snapshot_host.py (CPU) and tests/test_gpu_kv_snapshot.py.

The canonical form of tokens [from, to) of one layer is K [nkv, to - from, d] = the arena's K rows, and V [nkv, to - from, d] = kv_layout.v_logical of the arena's
V image, sliced: token-major for both.  An import of n canonical tokens at slot `at` is the same statement read backwards: the logical rows [at, at + n) of K and V
become the canonical ones and no other logical row changes.  The statement never speaks of 64-token blocks; the layout is kv_layout's."""
import torch
import kv_layout as L

MMD_OK, MMD_EINVAL, MMD_ERANGE = 0, -22, -34

CTX_LEN = 200                                                   # tokens the GPU tests fill by real steps
# (from, to) exported from a context of CTX_LEN tokens: everything, one token at either end, a span over a block edge, a whole block, all but the ends, one token
# inside the last (partly filled) block, nothing
EXPORT_SPANS = [(0, 200), (0, 1), (63, 65), (64, 128), (1, 199), (130, 131), (199, 200), (70, 70)]
IMPORT_SPLITS = [1, 63, 64, 65, 130]                            # an import of CTX_LEN tokens in two pieces: [0, s) then [s, CTX_LEN)
FORK_LENGTHS = [1, 64, 65, 200]
REFUSED_EXPORTS = [((0, CTX_LEN + 1), MMD_ERANGE), ((-1, 5), MMD_ERANGE), ((5, 4), MMD_ERANGE), ((CTX_LEN + 1, CTX_LEN + 1), MMD_ERANGE)]
# staging budgets for the chunking arithmetic, in tokens' worth of bytes: one chunk, two, many, and less than one token (one token per chunk)
CHUNK_BUDGETS = [('one', 1.0), ('two', 0.5), ('many', 0.07), ('below one token', 0.0001)]


def up64(n):
    return -(-n // L.BLK) * L.BLK


def canonical(K, V_raw, frm, to):
    """one layer as the arena stores it, K [nkv, m, d] and V_raw [nkv, m / 64, d, 64] -> canonical (K, V) [nkv, to - frm, d] of tokens [frm, to)"""
    return K[:, frm:to].contiguous(), L.v_logical(V_raw)[:, frm:to].contiguous()


def imported(K, V_raw, at, Kc, Vc):
    """the arena image of one layer after canonical tokens Kc, Vc [nkv, n, d] went into slots [at, at + n): -> (K, V_raw) of the same shapes as given"""
    n = Kc.shape[1]
    K2, V2 = K.clone(), L.v_logical(V_raw)
    K2[:, at:at + n] = Kc
    V2[:, at:at + n] = Vc
    return K2, L.v_raw(V2)


def labelled_arena(nkv, m, d, dtype=torch.int32):
    """an arena image whose every element names its (head, token, dim): K [nkv, m, d], V_raw as stored with V(h, t, e) = K(h, t, e) + 50"""
    K = (torch.arange(nkv)[:, None, None] * 1_000_000 + torch.arange(m)[None, :, None] * 100 + torch.arange(d)[None, None, :]).to(dtype).contiguous()
    return K, L.v_raw(K + 50)
