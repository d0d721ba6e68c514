"""mmd_kv_drop_spans stated on the host, for tests/test_kv_spans_host.py (CPU) and tests/test_gpu_kv_spans.py.

The arena after a drop of the spans [(from_i, to_i)]: the logical token rows of K and V with those rows deleted, nothing else touched (V goes through
kv_layout.v_logical, so the statement never speaks of 64-token blocks).  The plan is stated here a second time, in Python and independently of kv_plan.h: normalised
spans, retained segments, groups of 64 issued highest first."""
import torch
import kv_layout as L
import kv_drop_cases as D

MMD_OK, MMD_EINVAL, MMD_ERANGE = D.MMD_OK, D.MMD_EINVAL, D.MMD_ERANGE
PER_LAUNCH = 64


def every(first, width, gap, count):
    """`count` spans of `width` tokens, `gap` retained tokens between them, the first at `first`"""
    return [(first + i * (width + gap), first + i * (width + gap) + width) for i in range(count)]


# (spans, len)
ONE_SPAN = [([(f, t)], n) for f, t, n in D.REQUIRED]
CASES = ONE_SPAN + [
    ([(10, 20), (21, 30)], 200), ([(10, 20), (23, 30)], 200), ([(10, 20), (29, 40)], 200),          # the segment between two spans: 1, 3, 9 tokens
    ([(8, 9), (10, 11), (12, 13), (14, 20)], 200),                                                   # one destination group of 8 draws from four segments
    ([(5, 6), (20, 21), (40, 41), (70, 71), (90, 91), (130, 131), (150, 151), (200, 201)], 300),     # delta_i = 1 .. 8: every residue mod 8
    ([(3, 40), (100, 127)], 260),                                                                    # delta 37, then 64
    ([(60, 63), (64, 70), (127, 129), (190, 192)], 300),                                             # spans and segments below, on and across a block edge
    ([(0, 5), (9, 12)], 100),                                                                        # first span at 0
    ([(5, 9), (90, 100)], 100),                                                                      # last span ends at len
    ([(5, 5), (10, 20), (20, 30), (40, 40), (50, 55), (55, 55)], 120),                               # touching and empty spans
    ([(7, 7)], 50), ([], 50),                                                                        # nothing
    (every(10, 1, 2, 20), 10 + 60 + 4000),                                                           # an overlapping move: 20 tokens dropped, 4 000 behind
    (every(5, 2, 3, 70), 420), (every(5, 2, 3, 64), 400), (every(5, 2, 3, 65), 400),                 # across the 64-segment grouping
    (every(1, 2, 3, 64), 320),                                                                       # 64 spans, the last one ends at len: 63 segments
    (every(0, 1, 1, 130), 300),                                                                      # three groups of one-token segments
    ([(0, 128)], 128),                                                                               # all of the context
]

REFUSAL_LEN = 100
REFUSED = [([(30, 40), (10, 20)], MMD_EINVAL), ([(10, 30), (20, 40)], MMD_EINVAL), ([(10, 20), (15, 15)], MMD_EINVAL),          # unsorted, overlapping
           ([(10, 20), (90, 101)], MMD_ERANGE), ([(-1, 5)], MMD_ERANGE), ([(10, 20), (50, 40)], MMD_ERANGE), ([(30, 40), (10, 101)], MMD_ERANGE)]          # (the range is checked first)


def normalise(spans):
    """empty spans ignored, touching spans merged"""
    out = []
    for a, b in spans:
        if a == b:
            continue
        if out and out[-1][1] == a:
            out[-1] = (out[-1][0], b)
        else:
            out.append((a, b))
    return out


def kept(spans, n):
    """the old slots of the tokens that stay, in order"""
    gone = set()
    for a, b in spans:
        gone.update(range(a, b))
    return [t for t in range(n) if t not in gone]


def launches(spans, n):
    """-> [(dst0, len_in, len_end, [(src, count), ...]), ...] in the order they are issued"""
    ns, out, cur = normalise(spans), [], n
    for j in reversed(range(0, len(ns), PER_LAUNCH)):
        grp = ns[j:j + PER_LAUNCH]
        segs = [(b, (grp[i + 1][0] if i + 1 < len(grp) else cur) - b) for i, (a, b) in enumerate(grp)]
        segs = [s for s in segs if s[1] > 0]
        gone = sum(b - a for a, b in grp)
        if segs:
            out.append((grp[0][0], cur, cur - gone, segs))
        cur -= gone
    return out


def segments(spans, n):
    """the retained segments behind the first span as one pass would move them: [(src, count, dst, delta)]"""
    ns, out, dst = normalise(spans), [], None
    for i, (a, b) in enumerate(ns):
        dst = a if dst is None else dst
        end = ns[i + 1][0] if i + 1 < len(ns) else n
        if end > b:
            out.append((b, end - b, dst, b - dst))
            dst += end - b
    return out


def classes(case):
    """the names of every class a case belongs to"""
    spans, n = case
    ns, out = normalise(spans), set()
    if not ns:
        return {'nothing'}
    segs = segments(spans, n)
    if len(ns) == 1:
        out.add('one span')
    if any(a == b for a, b in spans):
        out.add('empty span in the list')
    if any(p[1] == q[0] and p[0] < p[1] and q[0] < q[1] for p, q in zip(spans, spans[1:])):
        out.add('touching spans')
    for (_, b), (a2, _) in zip(ns, ns[1:]):
        if a2 - b in (1, 3, 9):
            out.add(f'segment of {a2 - b} between two spans')
    for src, count, dst, delta in segs:
        out.add(f'delta%8=={delta % 8}')
        if delta % 64 == 0:
            out.add('delta%64==0')
        if src // 64 != (src + count - 1) // 64:
            out.add('segment crosses a block edge')
        if (src + count) % 64 == 0:
            out.add('segment ends on a block edge')
    for a, b in ns:
        if a // 64 != (b - 1) // 64:
            out.add('span crosses a block edge')
        if a % 64 == 0:
            out.add('span starts on a block edge')
        if b % 64 == 0:
            out.add('span ends on a block edge')
    for g0 in range(0, n, 8):          # a destination group of 8 tokens (bf16; fp32 groups hold 4) and the segments it draws from
        if sum(1 for _, count, dst, _ in segs if dst < g0 + 8 and dst + count > g0) >= 3:
            out.add('group from three segments')
    if ns[0][0] == 0:
        out.add('first span at 0')
    if ns[-1][1] == n:
        out.add('last span ends at len')
    if ns == [(0, n)]:
        out.add('all of the context')
    if len(ns) >= 20 and n - ns[-1][1] >= 4000 and all(b - a == 1 for a, b in ns):
        out.add('overlapping move')
    if len(ns) == PER_LAUNCH:
        out.add('64 spans')
    if len(ns) == PER_LAUNCH + 1:
        out.add('65 spans')
    if len(ns) >= 70:
        out.add('70 spans or more')
    if len(ns) > 2 * PER_LAUNCH:
        out.add('three groups')
    return out


ALL_CLASSES = ({'nothing', 'one span', 'empty span in the list', 'touching spans', 'segment of 1 between two spans', 'segment of 3 between two spans',
                'segment of 9 between two spans', 'delta%64==0', 'segment crosses a block edge', 'segment ends on a block edge', 'span crosses a block edge',
                'span starts on a block edge', 'span ends on a block edge', 'group from three segments', 'first span at 0', 'last span ends at len', 'all of the context',
                'overlapping move', '64 spans', '65 spans', '70 spans or more', 'three groups'} | {f'delta%8=={r}' for r in range(8)})


def drop_rows(x, spans, n=None):
    """[..., tokens, d] with the token rows of every span deleted (and cut to the first n tokens beforehand)"""
    if n is not None:
        x = x[..., :n, :]
    keep = torch.tensor(kept(spans, x.shape[-2]), dtype=torch.long, device=x.device)
    return x.index_select(-2, keep)


def expected_arena(K, V_raw, spans, n):
    """K [nkv, m, d], V_raw [nkv, m / 64, d, 64] as stored before the drop (m >= n) -> (K, V logical) [nkv, n - total, d] of the live tokens after it"""
    return drop_rows(K, spans, n), drop_rows(L.v_logical(V_raw), spans, n)


def drop_handle(kv, spans):
    """the oracle's KV handle with every span sliced out of every layer (kv_drop_cases.drop_handle per span, last span first)"""
    for a, b in reversed(normalise(spans)):
        kv = D.drop_handle(kv, a, b)
    return kv
