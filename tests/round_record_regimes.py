"""The recording rows of a scheduler round (round_blocks of mmduet_amd/csrc/select_plan.h with RoundSeg.record / lp_top), one row per case.  Plain data (imports without a
GPU): tests/test_round_record_plan_host.py asks round_blocks about every row on the host.

RECORD rows (name, segs, V, order, plan, rec0, record, kinds, refusal): segs are select_regimes.seg's eight fields followed by (record, lp_top); order lists the sampling
segments in the order of their logits rows -- plain arg-max | constrained arg-max | sampled, inside a block the rows that record nothing first and the recording ones last,
each group in segment order; plan is select_regimes.ROUND_FIELDS; rec0 the first row of each block's recording tail (the block's end when nothing in it records); record is
what mmd_op_round_last_record reports, (recording rows plain, constrained, sampled, largest top_n or -1); kinds names, per block, the select_regimes.SELECT_ROWS row whose
plan the block's launches follow (the sampled block: before its any_k / any_p are set from the round's)."""
from collections import namedtuple

import select_regimes as T

RecordRow = namedtuple('RecordRow', 'name segs V order plan rec0 record kinds refusal')
RECORD_FIELDS = ('plain', 'constrained', 'sampled', 'top_n')


def rseg(kind, sampler, record=0, lp_top=-1, **kw):
    return T.seg(**dict(dict(sampler=sampler), **dict(kind, **kw))) + (record, lp_top)


def _row(name, segs, order, plan, rec0, record, kinds, refusal=None, V=T.V):
    return RecordRow(name, tuple(segs), V, tuple(order) if order is not None else None, tuple(plan) if plan is not None else None, tuple(rec0) if rec0 is not None else None,
                     tuple(record) if record is not None else None, kinds, refusal)


P, Cn, S, FEED = T.PLAIN, T.CONS, T.SAMPLED, T.FEED_ONLY
OFF = ('block_argmax', 'block_argmax_cons', 'block_draw')
ON = ('block_argmax_lp', 'block_argmax_cons_lp', 'block_draw_lp')


def _rec(kind, i, top, **kw):
    return rseg(kind, i, 1, top, **kw)


RECORD_ROWS = [
    # one block at a time: every row records | none does
    _row('plain_all', [_rec(P, 0, 3), _rec(P, 1, 0)], (0, 1), (2, 2, 2, 0, 0, 0), (0, 2, 2), (2, 0, 0, 3), (ON[0], OFF[1], OFF[2])),
    _row('plain_none', [rseg(P, 0), rseg(P, 1)], (0, 1), (2, 2, 2, 0, 0, 0), (2, 2, 2), (0, 0, 0, -1), OFF),
    _row('cons_all', [_rec(Cn, 0, 8), _rec(Cn, 1, 2)], (0, 1), (0, 2, 2, 0, 0, 0), (0, 0, 2), (0, 2, 0, 8), (OFF[0], ON[1], OFF[2])),
    _row('cons_none', [rseg(Cn, 0), rseg(Cn, 1)], (0, 1), (0, 2, 2, 0, 0, 0), (0, 2, 2), (0, 0, 0, -1), OFF),
    _row('sampled_all', [_rec(S, 0, 0), _rec(S, 1, 0)], (0, 1), (0, 0, 2, 0, 0, 0), (0, 0, 0), (0, 0, 2, 0), (OFF[0], OFF[1], ON[2])),
    _row('sampled_none', [rseg(S, 0), rseg(S, 1)], (0, 1), (0, 0, 2, 0, 0, 0), (0, 0, 2), (0, 0, 0, -1), OFF),
    # interleaved inside a block: the recording rows move behind the others, both groups keep the segment order
    _row('plain_interleaved', [_rec(P, 0, 1), rseg(P, 1), _rec(P, 2, 4), rseg(P, 3)], (1, 3, 0, 2), (4, 4, 4, 0, 0, 0), (2, 4, 4), (2, 0, 0, 4), (ON[0], OFF[1], OFF[2])),
    _row('cons_interleaved', [_rec(Cn, 0, 1), rseg(Cn, 1), _rec(Cn, 2, 0)], (1, 0, 2), (0, 3, 3, 0, 0, 0), (0, 1, 3), (0, 2, 0, 1), (OFF[0], ON[1], OFF[2])),
    _row('sampled_interleaved', [rseg(S, 0, top_k=5), _rec(S, 1, 2), rseg(S, 2, top_p=0.5), _rec(S, 3, 6, constrained=1)], (0, 2, 1, 3), (0, 0, 4, 1, 1, 1), (0, 0, 2),
         (0, 0, 2, 6), (OFF[0], OFF[1], 'block_draw_cons_lp')),
    # all three blocks in one round, a feed-only segment between them (select_regimes.MIXED with recording rows)
    _row('mixed_all', [_rec(S, 0, 2), _rec(P, 1, 3), _rec(Cn, 2, 0), rseg(FEED, 3), _rec(P, 4, 8)], (1, 4, 2, 0), (2, 3, 4, 0, 0, 0), (0, 2, 3), (2, 1, 1, 8), ON),
    _row('mixed_none', [rseg(S, 0), rseg(P, 1), rseg(Cn, 2), rseg(FEED, 3), rseg(P, 4)], (1, 4, 2, 0), (2, 3, 4, 0, 0, 0), (2, 3, 4), (0, 0, 0, -1), OFF),
    _row('mixed_interleaved', [_rec(P, 0, 3), rseg(S, 1), rseg(P, 2), _rec(Cn, 3, 0), _rec(S, 4, 0), rseg(Cn, 5), _rec(P, 6, 1), rseg(S, 7)],
         (2, 0, 6, 5, 3, 1, 7, 4), (3, 5, 8, 0, 0, 0), (1, 4, 7), (2, 1, 1, 3), ON),
    # a recording sampler that only feeds is no recording row
    _row('feed_only_recording', [rseg(P, 0), rseg(FEED, 1, 1, 5)], (0,), (1, 1, 1, 0, 0, 0), (1, 1, 1), (0, 0, 0, -1), OFF),
    # the limit of a round: 32 recording plain rows
    _row('32_plain_recording', [_rec(P, i, 8) for i in range(32)], tuple(range(32)), (32, 32, 32, 0, 0, 0), (0, 32, 32), (32, 0, 0, 8), (ON[0], OFF[1], OFF[2])),
    # the refusals are the ones of the round without records
    _row('33_sampling', [_rec(P, i, 0) for i in range(33)], None, None, None, None, None, (T.MMD_ERANGE, 'more than 32 sampling segments')),
    _row('sampler_twice', [_rec(P, 0, 0), _rec(S, 1, 0), _rec(Cn, 0, 0)], None, None, None, None, None, (T.MMD_EINVAL, 'a sampler may appear once per round')),
    _row('feed_two_rows', [_rec(P, 0, 0), rseg(FEED, 1, rows=2)], None, None, None, None, None, (T.MMD_EINVAL, 'a feed segment is one row (segment 1 has 2)')),
]
