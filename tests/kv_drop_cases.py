"""mmd_kv_drop stated on the host, for tests/test_kv_drop_host.py (CPU), tests/test_gpu_kv_drop.py and tests/test_gpu_kv_drop_trueshape.py.

The arena after a drop of [from, to): the logical token rows of K and V with those rows deleted, nothing else touched (V goes through kv_layout.v_logical /
v_raw, so the statement never speaks of 64-token blocks).  The model after a drop: the oracle's own layer loop over the KV handle with the span sliced out, the
new rows rotated at the positions the stream has reached (n0 + arange(S)), NOT at the slots they are written to."""
import torch
import kv_layout as L
from oracle import duet_oracle as O

MMD_OK, MMD_EINVAL, MMD_ERANGE = 0, -22, -34

# (from, to, len).  The first seven are the ones the layout asks for: `from` / `to` on every side of a 64-token block edge and on residues mod 8
REQUIRED = [(0, 1, 2), (5, 6, 200), (63, 65, 257), (64, 128, 300), (1, 130, 131), (60, 63, 64), (7, 71, 500)]
OVERLAPPING = [(3, 4, 4099), (100, 149, 70000)]          # delta far below the tokens behind the span: the move runs over itself thousands of times
CASES = REQUIRED + OVERLAPPING + [
    (8, 200, 260),          # disjoint (delta 192 > 60 tokens behind), delta a multiple of 64
    (10, 50, 50),           # to == len: a truncate that keeps the position
    (0, 128, 128),          # ... of everything
    (17, 17, 100),          # from == to: nothing
    (0, 64, 130),           # from == 0, whole first block
    (2, 13, 140), (59, 62, 190), (4, 68, 133), (62, 127, 129), (125, 131, 322), (2, 14, 141), (59, 64, 197), (126, 133, 330),          # remaining residues mod 8 of from / to / delta
]
BIG_LEN = 70000             # 72 MB per arena in bf16 at nkv = 4: run with nkv = 4 only


def delta(c):
    return c[1] - c[0]


def behind(c):
    return c[2] - c[1]


def classes(c):
    """the names of every class a case belongs to"""
    f, t, n = c
    out = set()
    if f == t:
        return {'empty'}
    out.add('delta%64==0' if delta(c) % 64 == 0 else 'delta%64!=0')
    out.add('from%64==0' if f % 64 == 0 else 'from%64!=0')
    out.add('to%64==0' if t % 64 == 0 else 'to%64!=0')
    if t == n:
        out.add('to==len')
    elif delta(c) > behind(c):
        out.add('disjoint')
    elif delta(c) < behind(c):
        out.add('overlapping')
    if f == 0:
        out.add('from==0')
    if f // 64 != (t - 1) // 64:
        out.add('span crosses a block edge')
    return out


ALL_CLASSES = {'empty', 'delta%64==0', 'delta%64!=0', 'from%64==0', 'from%64!=0', 'to%64==0', 'to%64!=0', 'to==len', 'disjoint', 'overlapping', 'from==0',
               'span crosses a block edge'}

# (from, to) refused on a context of REFUSAL_LEN tokens, and the code; then the stash rule (any span while a stash is held: MMD_EINVAL) and the null stream (MMD_EINVAL)
REFUSAL_LEN = 100
REFUSED_RANGES = [((-1, 5), MMD_ERANGE), ((5, 4), MMD_ERANGE), ((0, 101), MMD_ERANGE), ((101, 101), MMD_ERANGE), ((50, 1 << 40), MMD_ERANGE), ((-3, -2), MMD_ERANGE)]


def drop_rows(x, frm, to, n=None):
    """[..., tokens, d] with token rows [frm, to) deleted (and cut to the first n tokens beforehand)"""
    if n is not None:
        x = x[..., :n, :]
    return torch.cat([x[..., :frm, :], x[..., to:, :]], -2)


def expected_arena(K, V_raw, frm, to, n):
    """K [nkv, m, d], V_raw [nkv, m / 64, d, 64] as stored before the drop (m >= n) -> (K [nkv, n - delta, d], V logical [nkv, n - delta, d]) of the live tokens after it"""
    return drop_rows(K, frm, to, n), drop_rows(L.v_logical(V_raw), frm, to, n)


def drop_handle(kv, a, b):
    """the oracle's KV handle with tokens [a, b) sliced out of every layer"""
    return O.KVHandle([torch.cat([k[:, :a], k[:, b:]], 1) for k in kv.k], [torch.cat([v[:, :a], v[:, b:]], 1) for v in kv.v])


def oracle_step_at(w, cfg, x, past, pos0):
    """O.llm_forward with the new rows' positions given (pos0 + arange(S)) instead of taken from the handle's length: x [S, H] -> (hidden [S, H], handle)"""
    S = x.shape[0]
    n = len(past) if past else 0
    cos, sin = O.rope_tables(cfg, pos0 + torch.arange(S), x.dtype)
    h, ks, vs = x, [], []
    for i in range(cfg.num_hidden_layers):
        h, k, v = O.llm_layer(w, cfg, i, h, cos, sin, past.k[i] if n else None, past.v[i] if n else None)
        ks.append(k); vs.append(v)
    return O.rms_norm(h, w['model.norm.weight'], cfg.rms_norm_eps), O.KVHandle(ks, vs)


def oracle_greedy_at(w, cfg, x, past, pos0, n_new):
    """greedy ids of the oracle from a context whose next position is pos0 (no penalty, no EOS) -> (ids, smallest gap between the two best logits, handle)"""
    ids, gap = [], float('inf')
    for _ in range(n_new):
        h, past = oracle_step_at(w, cfg, x, past, pos0)
        pos0 += x.shape[0]
        top = O.linear(h[-1:], w['lm_head.weight']).float()[0].topk(2)
        gap = min(gap, float(top.values[0] - top.values[1]))
        ids.append(int(top.indices[0]))
        x = w['model.embed_tokens.weight'][ids[-1]][None]
    return ids, gap, past


def drop_amount_reference(length, rows, window, sink):
    """the policy's m by search: the smallest m in [0, length - sink] with length - m + rows <= window, or length - sink if there is none"""
    if window <= 0:
        return 0
    for m in range(0, max(0, length - sink) + 1):
        if length - m + rows <= window:
            return m
    return max(0, length - sink)
