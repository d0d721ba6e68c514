"""CPU restatement of the plain greedy token loop's device side (ops.hip: argmax_penalty_kernel / argmax_penalty_multi_kernel with their final kernels, advance_state_kernel)
and the rows the tests put through it.

The oracle works in float32 ON PURPOSE.  The kernels apply the repetition penalty as one fp32 multiplication or division per listed id (ops.hip is compiled with
-ffp-contract=off and without -ffast-math, so that is an IEEE operation), and the arg-max then decides ties between those rounded values.  An fp32 oracle rounds the same way
and therefore ties where the kernel ties; a float64 oracle would see 2.0 / 1.3 and a neighbouring logit as different numbers where the device sees equal ones, and would call
another winner.  There is no tolerance anywhere: a token is an integer.

Contract (include/mmduet.h, mmd_greedy_generate / mmd_op_argmax):
  * ids of the list outside [0, V) match no column; an id listed several times is penalised once;
  * pen(l) = l * p if l < 0 else l / p on listed ids, l elsewhere; penalty None or <= 0: no penalty at all;
  * a NaN among the RAW logits -> -1, wherever it sits; otherwise the first maximal index of pen(l) (all -inf: 0; +inf: the first +inf; -0.0 == +0.0).
tests/test_greedy_oracle_host.py pins this to transformers' RepetitionPenaltyLogitsProcessor followed by torch.argmax."""
import numpy as np
import torch

SLICES = 64          # ARGMAX_BLOCKS: a row is cut into 64 slices of per(V) columns, 256 threads stride through a slice
VS = (1, 2, 63, 64, 65, 255, 4097, 151936, 152064)
INT_MAX = 0x7fffffff


def per(V):
    return -(-V // SLICES)


def scores(logits, prev_ids=(), penalty=None):
    """pen(l) in float32."""
    l = np.asarray(logits, dtype=np.float32)
    z = l.copy()
    if penalty is not None and penalty > 0 and len(prev_ids):
        V = l.shape[0]
        ids = np.array(sorted({int(t) for t in prev_ids if 0 <= int(t) < V}), dtype=np.int64)
        if len(ids):
            p = np.float32(penalty)
            with np.errstate(invalid='ignore'):
                z[ids] = np.where(l[ids] < 0, l[ids] * p, l[ids] / p).astype(np.float32)
    return z


def pick(logits, prev_ids=(), penalty=None):
    l = np.asarray(logits, dtype=np.float32)
    if np.isnan(l).any():
        return -1
    return int(np.argmax(scores(l, prev_ids, penalty)))


def advance(state, tok, eos, use_penalty, prev_cap):
    """advance_state_kernel without constraints.  state: dict(prev=list of prev_cap (or more) slots, n_prev, n_ctx, step) -> a new one."""
    s = dict(prev=list(state['prev']), n_prev=state['n_prev'], n_ctx=state['n_ctx'], step=state['step'])
    if use_penalty and tok != eos and s['n_prev'] < prev_cap:
        s['prev'][s['n_prev']] = tok
        s['n_prev'] += 1
    s['n_ctx'] += 1
    s['step'] += 1
    return s


# ---- the two comparison rules, folded over a row in index order (small rows only: a Python loop) ------------------------------------------------------------------
def better_new(v, i, bv, bi):
    return v > bv or (v == bv and i < bi) or (v != v and bv == bv)


def better_before(v, i, bv, bi):
    """`better` as it was before a NaN failed the arg-max: a NaN loses every comparison"""
    return v > bv or (v == bv and i < bi)


def fold(z, better, final_nan_check):
    """The kernels' reduction with the candidates taken in index order: -> what the final kernel writes."""
    best, bi = np.float32(-np.inf), INT_MAX
    for i, v in enumerate(np.asarray(z, dtype=np.float32)):
        if better(v, i, best, bi):
            best, bi = v, i
    return -1 if final_nan_check and best != best else bi


# ---- the rows -------------------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    __slots__ = ('name', 'row', 'prev', 'penalty', 'want')

    def __init__(self, name, row, prev=(), penalty=None, want=None):
        self.name, self.row, self.prev, self.penalty, self.want = name, row.to(torch.float32).contiguous(), list(prev), penalty, want

    @property
    def has_nan(self):
        return bool(torch.isnan(self.row).any())

    @property
    def hf_expressible(self):
        """no NaN and every listed id in range: what RepetitionPenaltyLogitsProcessor can be asked"""
        V = self.row.numel()
        return not self.has_nan and all(0 <= t < V for t in self.prev)


def tie_pairs(V):
    """Index pairs (i < j) a planted tie is written at: both ends of the row, neighbours in a wave, one lane on two strides, a wave boundary inside a slice, slice
    boundaries, and the first slice against the last."""
    p = per(V)
    c = [(0, V - 1)]
    if p >= 3:
        c.append((1, 2))                                   # (i, i + 1) in one wave of one slice
    if p > 260:
        c.append((2 * p + 3, 2 * p + 3 + 256))             # the same lane on its next stride
    if p >= 65:
        c += [(63, 64), (p + 63, p + 64)]                  # lanes 63 / 0 of neighbouring waves, in slice 0 and in slice 1
    c += [(k * p - 1, k * p) for k in (1, 31, 63)]         # slice boundaries
    c.append((p - 1, 63 * p))                              # the last column of slice 0 against the first column of slice 63
    out = []
    for i, j in c:
        if 0 <= i < j < V and (i, j) not in out:
            out.append((i, j))
    return out


def nan_columns(V):
    return sorted({0, V - 1, min(V - 1, per(V)), max(0, per(V) - 1), V // 2})


_cases = {}


def cases(V):
    """Every row of one vocabulary size, built once (the tests never write to them).  `want` is set where the expected token follows from how the row was made; the
    oracle must agree with it (tests/test_greedy_oracle_host.py), the kernels are compared with the oracle."""
    if V in _cases:
        return _cases[V]
    g = torch.Generator().manual_seed(1100 + VS.index(V) if V in VS else V)
    out = []
    std_prev = [0, V - 1, 3 % V, 3 % V, 0]

    def randn(scale=1.0):
        return torch.randn(V, generator=g) * scale

    # families, each without and with a penalty
    fam = [('randn4_%d' % k, randn(4.0), None) for k in range(4)]
    fam.append(('equal', torch.full((V,), 0.7), 0))
    fam.append(('neginf', torch.full((V,), -float('inf')), 0))
    r = randn()
    a, b = (V // 3, V - 1) if V > 1 else (0, 0)
    r[a] = r[b] = float('inf')
    fam.append(('posinf2', r, a))
    r = -randn().abs() - 0.5
    r[a], r[b] = -0.0, 0.0
    fam.append(('zeros', r, a))
    for name, row, want in fam:
        out.append(Case(name, row, (), None, want))
        out.append(Case(name + '+pen', row, std_prev, 1.3, None))
    # planted ties: the row maximum at (i, j), once on a row and once on its mirror image (what surrounds the pair differs), written in both orders
    for i, j in tie_pairs(V):
        base = randn()
        top = float(base.max()) + 1.0
        r1 = base.clone(); r1[i] = top; r1[j] = top
        r2 = base.flip(0).clone(); r2[j] = top; r2[i] = top
        out.append(Case('tie_%d_%d' % (i, j), r1, (), None, i))
        clear = i > 3 and j < V - 1          # the pair is not on the standard list: penalising the others moves them away from the maximum, never onto it
        out.append(Case('tie_%d_%d_mirror' % (i, j), r2, std_prev if clear else (), 1.3, i))
    # ties the penalty makes: the penalised id before and after the other index
    pairs = tie_pairs(V)
    for i, j in (pairs[:1] + pairs[-2:-1] if len(pairs) > 1 else pairs):
        for pen_at, other in ((i, j), (j, i)):
            first = min(i, j)
            for p, pos, neg in ((2.0, 2.0, -1.0), (0.5, 0.5, -4.0), (1.0, 1.0, -2.0)):
                r = -randn().abs()                       # everything else <= 0 < 1
                r[other] = 1.0; r[pen_at] = pos          # pos / p == 1
                out.append(Case('pentie_pos_p%s_%d_%d' % (p, pen_at, other), r, [pen_at], p, first))
                r = -randn().abs() - 2.5                 # everything else < -2
                r[other] = -2.0; r[pen_at] = neg         # neg * p == -2
                out.append(Case('pentie_neg_p%s_%d_%d' % (p, pen_at, other), r, [pen_at], p, first))
    # lists
    r = randn(4.0)
    out.append(Case('list_empty', r, [], 1.3, int(r.argmax())))
    if V >= 2:          # an id listed seven times is penalised once: 4 / 2 = 2 beats the runner-up's 1.5, a second division (1) would lose to it
        r = -randn().abs() - 1.0
        w, u = (V * 2) // 3, V // 3
        r[w], r[u] = 4.0, 1.5
        out.append(Case('list_dup_winner', r, [w] * 7, 2.0, w))
    r2 = randn(); r2[0] = float(r2.max()) + 1.0
    out.append(Case('list_out_of_range', r2, [V, -1, 1 << 40, 1 << 32, -(1 << 40), V + (1 << 33)], 100.0, 0))          # (an id cut to 32 bits would hit column 0 and dethrone it)
    out.append(Case('list_out_of_range_mixed', r2, [V, 0, -1, 1 << 40], 100.0, None))
    if V == 255:
        out.append(Case('list_all', randn(4.0), list(range(V)), 1.7, None))
        out.append(Case('list_all_shuffled', randn(4.0), torch.randperm(V, generator=g).tolist() + [5, 5], 0.6, None))
    if V == 152064:
        ids = torch.randperm(V, generator=g)[:2048]
        r = randn(4.0)
        top = torch.topk(r, 40).indices          # the 40 largest are on the list (among 2008 others): the winner comes from below them
        ids[:40] = top
        out.append(Case('list_2048', r, sorted(set(ids.tolist())), 3.0, None))
    # NaN: -1 wherever it sits
    for c in nan_columns(V):
        r = randn(4.0); r[c] = float('nan')
        out.append(Case('nan_%d' % c, r, (), None, -1))
        out.append(Case('nan_%d_listed' % c, r, [c, 0], 1.3, -1))
        out.append(Case('nan_%d_other_listed' % c, r, [(c + 1) % V], 1.3, -1))
    if V > 1:
        r = randn(); r[V // 2] = float('nan'); r[V // 2 - 1] = float('inf')
        out.append(Case('nan_beside_posinf', r, (), None, -1))
        r = randn(); r[0] = float('inf'); r[V - 1] = float('nan')
        out.append(Case('nan_after_posinf', r, [0], 1.3, -1))
    out.append(Case('nan_all', torch.full((V,), float('nan')), (), None, -1))
    out.append(Case('nan_all_listed', torch.full((V,), float('nan')), std_prev, 1.3, -1))
    _cases[V] = out
    return out
