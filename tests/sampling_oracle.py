"""CPU restatement of the sampling contract (DESIGN.md "Sampling"), float64 and literal: no sort decides anything -- tie classes are grouped by VALUE and every
"strictly above" quantity is a sum over the classes with a larger value.  `analyse_literal` is the O(V^2) word-for-word form (small V); `analyse` computes the same
numbers per class and is what the tests use at vocabulary size.

  scores   z_i = pen(l_i) / T, pen(l) = l / p if l > 0 else l * p, once per id however often the id is listed
  top-k    keep i iff #{j: z_j > z_i} < k               (k = 0 or k >= V: off)
  top-p    over the top-k survivors: P_j = exp(z_j - max) / sum_kept exp(z - max); keep i iff sum{P_j: z_j > z_i} < p     (p = 1: off)
  draw     u = r / 2^64; the first kept index, in index order, whose inclusive prefix mass exceeds u * Z_kept
  r        Philox4x32-10, key (seed_lo, seed_hi), counter (offset_lo, offset_hi, lane, 0): r = x0 * 2^32 + x1
"""
import numpy as np

M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def philox_word(seed, offset, lane=0):
    x = philox4x32_10((offset & M32, (offset >> 32) & M32, lane & M32, 0), (seed & M32, (seed >> 32) & M32))
    return (x[0] << 32) | x[1]


def scores(logits, prev_ids=None, penalty=None, temperature=1.0):
    z = np.asarray(logits, dtype=np.float64).copy()
    if penalty and prev_ids is not None and len(prev_ids):
        ids = np.unique(np.asarray(prev_ids, dtype=np.int64))
        z[ids] = np.where(z[ids] > 0, z[ids] / penalty, z[ids] * penalty)
    return z / temperature


def _weights(z):
    with np.errstate(invalid='ignore'):
        return np.where(np.isneginf(z), 0.0, np.exp(z - z.max())) if np.isfinite(z.max()) else (z == z.max()).astype(np.float64)


def analyse_literal(z, top_k=0, top_p=1.0):
    """Word for word, O(V^2): -> (rank[i] = #{z_j > z_i}, mass_above[i] = share of the top-k survivors' mass strictly above z_i, keep[i])."""
    z = np.asarray(z, dtype=np.float64)
    V = len(z)
    w = _weights(z)
    rank = np.array([int((z > z[i]).sum()) for i in range(V)])
    keep_k = rank < top_k if 0 < top_k < V else np.ones(V, bool)
    Zk = (w * keep_k).sum()
    above = np.array([(w * keep_k * (z > z[i])).sum() for i in range(V)]) / Zk
    keep = keep_k & (above < top_p) if top_p < 1.0 else keep_k
    return rank, above, keep


def analyse(z, top_k=0, top_p=1.0):
    """The same three arrays through the tie classes (np.unique groups equal values; the cumulative sums run over classes, largest value first)."""
    z = np.asarray(z, dtype=np.float64)
    V = len(z)
    w = _weights(z)
    vals, inv, cnt = np.unique(z, return_inverse=True, return_counts=True)          # ascending class values
    above_cnt = cnt.sum() - np.cumsum(cnt)                                          # members of the classes with a larger value
    rank = above_cnt[inv]
    keep_k = rank < top_k if 0 < top_k < V else np.ones(V, bool)
    cm = np.bincount(inv, weights=w * keep_k, minlength=len(vals))
    rev = np.cumsum(cm[::-1])[::-1]                                                  # mass of this class and every larger one
    above = ((rev - cm) / rev[0])[inv]
    keep = keep_k & (above < top_p) if top_p < 1.0 else keep_k
    return rank, above, keep


def draw_interval(z, keep, token):
    """[lo, hi) of `token` in the index-order CDF over `keep`, as shares of the kept mass, and the token's own mass."""
    w = _weights(np.asarray(z, dtype=np.float64)) * keep
    c = np.cumsum(w)
    return (c[token] - w[token]) / c[-1], c[token] / c[-1], w[token]


def draw(z, keep, r):
    """The token the contract assigns to the 64-bit word r, and the distance of u from the nearest CDF boundary."""
    w = _weights(np.asarray(z, dtype=np.float64)) * keep
    c = np.cumsum(w) / w.sum()
    u = r / 2.0 ** 64
    t = int(np.searchsorted(c, u, side='right'))          # first index with c > u
    while w[t] == 0:                                       # (a boundary hit exactly: the next token with mass)
        t += 1
    return t, float(np.abs(c - u).min())


def sample(logits, prev_ids=None, penalty=None, temperature=1.0, top_k=0, top_p=1.0, r=0):
    z = scores(logits, prev_ids, penalty, temperature)
    if np.isnan(z).any():
        return -1
    return draw(z, analyse(z, top_k, top_p)[2], r)[0]
