"""The stream KV arena's operations (kv_plan of mmduet_amd/csrc/kv_plan.h), one row per case: the plan an operation must get -- every field of it -- or the refusal, and the
capacities growth must try.  tests/test_kv_plan_host.py asks the header about every row on the host.

The expectations are stated here on their own, from the layout (kv_layout.BLK, kv_layout.v_index) and plain arithmetic in tokens and bytes; where a row pins which of two
refusals wins, or a limit, it cites the line of model.hip at commit 25fad5b (the last one whose entry points made these checks themselves) that decided it."""
from collections import namedtuple
from math import gcd

import kv_layout as L
import kv_snapshot_cases as S

MMD_OK, MMD_EINVAL, MMD_ERANGE = S.MMD_OK, S.MMD_EINVAL, S.MMD_ERANGE
# the header's enums (the test checks these numbers against the shim's list)
OPS = ('truncate', 'reset', 'stash', 'unstash', 'drop', 'export', 'import', 'set_position', 'fork', 'debug_set_len', 'debug_read')
TRUNCATE, RESET, STASH, UNSTASH, DROP, EXPORT, IMPORT, SET_POSITION, FORK, DEBUG_SET_LEN, DEBUG_READ = range(len(OPS))
BUF_OK, BUF_MISSING, BUF_MISALIGNED = range(3)
NONE, ROWS_OUT, ROWS_IN, LAUNCH_DROP, CANON_GATHER, CANON_SCATTER = range(6)
CONSTANTS = dict({'KV_' + n.upper(): i for i, n in enumerate(OPS)}, KV_OPS=len(OPS), KV_BUF_OK=BUF_OK, KV_BUF_MISSING=BUF_MISSING, KV_BUF_MISALIGNED=BUF_MISALIGNED,
                 KV_LAUNCH_NONE=NONE, KV_ROWS_OUT=ROWS_OUT, KV_ROWS_IN=ROWS_IN, KV_LAUNCH_DROP=LAUNCH_DROP, KV_CANON_GATHER=CANON_GATHER, KV_CANON_SCATTER=CANON_SCATTER,
                 KV_MAX_RESERVATIONS=64, KV_VIRTUAL_TOKENS_DEFAULT=4 << 20)

FIELDS = ('nothing', 'reserve', 'stash_bytes', 'launch', 'k_off', 'k_bytes', 'v_off', 'v_bytes', 'k_cols', 'v_cols', 'pitch4', 'k_other4', 'v_other4', 'copy_rows', 't0', 't1',
          'pitch_bytes', 'after_len', 'after_pos_off', 'after_cap', 'after_mapped', 'after_stash_from', 'after_stash_to')
Geom = namedtuple('Geom', 'layers kv_heads head_dim elem')
State = namedtuple('State', 'len pos_off cap mapped stash_from stash_to')
Row = namedtuple('Row', 'name op geom state a b src bufs refusal plan')          # refusal: (rc, a distinctive piece of the message) or None;  plan: {field: value} or None

TINY, B7 = Geom(2, 3, 16, 2), Geom(28, 4, 128, 2)          # 32 and 256 bytes per token
GEOMS = {'tiny': TINY, '7b': B7}
INT_MAX = 2 ** 31 - 1          # one copy launch takes a row's width as an int of 4-byte units (fork: model.hip:1283; debug_read, times the kv heads: model.hip:1312)


def tok(g):
    return g.head_dim * g.elem


def rows(g):
    return g.layers * g.kv_heads


def ctx(g, n=S.CTX_LEN, pos_off=0, stash=(-1, -1)):
    """a context of n tokens: the tiny model on a plain 256-token arena, the 7B one on a virtual row stride of 4 Mi tokens with one 8192-token chunk behind it"""
    cap, mapped = (256, 256) if g is TINY else (4 << 20, 8192)
    return State(n, pos_off, cap, mapped, *stash)


def plan(state, **kw):
    """every field of a plan that launches nothing and leaves the state as it is, then the row's own"""
    p = dict.fromkeys(FIELDS, 0)
    p.update({'after_' + k: v for k, v in state._asdict().items()})
    assert set(kw) <= set(FIELDS), set(kw) - set(FIELDS)
    p.update(kw)
    return p


def span(g, cap, frm, to, launch, n_rows=None, base=0, other4=None):
    """the strided copy of tokens [frm, to): K's bytes as they lie, V's in the whole 64-token blocks that hold them; widths and pitches also in 4-byte units; the other side
    packed (each row as wide as its span) unless it has a pitch of its own"""
    t = tok(g)
    first_blk, end_blk = frm // L.BLK, -(-to // L.BLK)
    k_bytes, v_bytes = (to - frm) * t, (end_blk - first_blk) * L.BLK * t
    return dict(launch=launch, copy_rows=rows(g) if n_rows is None else n_rows, k_off=base + frm * t, k_bytes=k_bytes, v_off=base + first_blk * L.BLK * t, v_bytes=v_bytes,
                k_cols=k_bytes // 4, v_cols=v_bytes // 4, pitch4=cap * t // 4, k_other4=k_bytes // 4 if other4 is None else other4, v_other4=v_bytes // 4 if other4 is None else other4)


def _rows():
    out = []

    def add(name, op, g, state, a=0, b=0, src=None, bufs=BUF_OK, refusal=None, plan=None):
        assert (refusal is None) != (plan is None), name
        out.append(Row(name, op, g, state, a, b, src, bufs, refusal, plan))

    for gn, g in GEOMS.items():
        c, t, r = ctx(g), tok(g), rows(g)
        # ---- spans of a 200-token context -------------------------------------------------------------------------------
        # (63, 65) straddles a block edge, (64, 128) is exactly one block, (130, 131) one token.  (70, 70) is empty for K; V's rule -- from the start of `from`'s block to the
        # end of the last block that reaches `to` -- still names the block around slot 70, and model.hip:1178-1187 copied it: the plan must say the same
        for frm, to in S.EXPORT_SPANS:
            sp = span(g, c.cap, frm, to, ROWS_OUT)
            add(f'{gn}_stash_{frm}_{to}', STASH, g, c, frm, to, plan=plan(c, stash_bytes=r * max(sp['k_bytes'], sp['v_bytes']), after_stash_from=frm, after_stash_to=to, **sp))
            held = ctx(g, frm, stash=(frm, to))
            add(f'{gn}_unstash_{frm}_{to}', UNSTASH, g, held, plan=plan(held, reserve=to, after_len=to, after_stash_from=-1, after_stash_to=-1, **span(g, c.cap, frm, to, ROWS_IN)))
            moved = dict(after_len=c.len - (to - frm), after_pos_off=to - frm)
            if frm == to:
                add(f'{gn}_drop_{frm}_{to}', DROP, g, c, frm, to, plan=plan(c, nothing=1))
                add(f'{gn}_export_{frm}_{to}', EXPORT, g, c, frm, to, plan=plan(c, nothing=1))
                continue
            if to == c.len:          # a dropped tail moves nothing: no launch
                add(f'{gn}_drop_{frm}_{to}', DROP, g, c, frm, to, plan=plan(c, **moved))
            else:
                add(f'{gn}_drop_{frm}_{to}', DROP, g, c, frm, to, plan=plan(c, launch=LAUNCH_DROP, t0=frm, t1=to, pitch_bytes=c.cap * t, **moved))
            add(f'{gn}_export_{frm}_{to}', EXPORT, g, c, frm, to, plan=plan(c, launch=CANON_GATHER, t0=frm, t1=to - frm, pitch_bytes=c.cap * t))
        for (frm, to), rc in S.REFUSED_EXPORTS:
            for op, word in ((STASH, 'kv_stash ['), (DROP, 'kv_drop ['), (EXPORT, 'kv_export [')):
                add(f'{gn}_{OPS[op]}_refused_{frm}_{to}', op, g, c, frm, to, refusal=(rc, f'{word}{frm}, {to}) outside the context (200 tokens)'))
        # ---- fork: the destination's own bookkeeping goes, the source's position comes; each side keeps its own pitch ------
        src = ctx(g, pos_off=11)
        dst = State(7, 3, 512 if g is TINY else 1 << 20, 512 if g is TINY else 8192, -1, -1)
        assert dst.cap != src.cap
        for n in [0] + S.FORK_LENGTHS:
            add(f'{gn}_fork_{n}', FORK, g, dst, n, src=src, plan=plan(dst, reserve=n, after_len=n, after_pos_off=src.pos_off, **span(g, dst.cap, 0, n, ROWS_IN, other4=src.cap * t // 4)))
        # ---- debug_read: one layer's kv-head rows, whole blocks, only where memory is --------------------------------------
        for layer, n in ((0, 0), (0, 64), (g.layers - 1, 128), (1, c.mapped)):
            sp = span(g, c.cap, 0, n, ROWS_OUT, n_rows=g.kv_heads, base=layer * g.kv_heads * c.cap * t)
            assert sp['v_bytes'] == sp['k_bytes']
            add(f'{gn}_debug_read_{layer}_{n}', DEBUG_READ, g, c, layer, n, plan=plan(c, **sp))
        for layer, n, bufs, word in ((0, 65, BUF_OK, 'n = 65 must be a multiple of 64'), (0, c.mapped + 64, BUF_OK, f'within the {c.mapped} tokens backed by memory'),
                                     (0, -64, BUF_OK, 'n = -64 must be'), (-1, 64, BUF_OK, f'layer -1 of {g.layers}'), (g.layers, 64, BUF_OK, f'layer {g.layers} of {g.layers}'),
                                     (0, 64, BUF_MISSING, 'or an output buffer missing')):
            add(f'{gn}_debug_read_refused_{layer}_{n}_{bufs}', DEBUG_READ, g, c, layer, n, bufs=bufs, refusal=(MMD_EINVAL, word))
        add(f'{gn}_debug_read_misaligned', DEBUG_READ, g, c, 0, 64, bufs=BUF_MISALIGNED,          # model.hip:1307 asked for the buffers' presence alone
            plan=plan(c, **span(g, c.cap, 0, 64, ROWS_OUT, n_rows=g.kv_heads)))
        # ---- bookkeeping ----------------------------------------------------------------------------------------------------
        held = ctx(g, 150, pos_off=9, stash=(120, 180))
        add(f'{gn}_truncate_below_stash', TRUNCATE, g, held, 119, plan=plan(held, after_len=119, after_stash_from=-1, after_stash_to=-1))
        add(f'{gn}_truncate_at_stash', TRUNCATE, g, held, 120, plan=plan(held, after_len=120))
        add(f'{gn}_truncate_above_stash', TRUNCATE, g, held, 149, plan=plan(held, after_len=149))
        add(f'{gn}_truncate_all', TRUNCATE, g, c, 0, plan=plan(c, after_len=0))
        add(f'{gn}_truncate_none', TRUNCATE, g, c, 200, plan=plan(c))
        add(f'{gn}_truncate_negative', TRUNCATE, g, c, -1, refusal=(MMD_ERANGE, 'kv_truncate(-1) outside [0, 200]'))
        add(f'{gn}_truncate_beyond', TRUNCATE, g, c, 201, refusal=(MMD_ERANGE, 'kv_truncate(201) outside [0, 200]'))
        add(f'{gn}_reset', RESET, g, held, plan=plan(held, after_len=0, after_pos_off=0, after_stash_from=-1, after_stash_to=-1))
        add(f'{gn}_set_position_same', SET_POSITION, g, held, 150, plan=plan(held, after_pos_off=0))
        add(f'{gn}_set_position', SET_POSITION, g, held, 1000, plan=plan(held, after_pos_off=850))
        add(f'{gn}_set_position_below', SET_POSITION, g, held, 149, refusal=(MMD_ERANGE, "kv_set_position(149) below the context's 150 tokens"))
        dropped = ctx(g, pos_off=40)
        add(f'{gn}_drop_keeps_counting', DROP, g, dropped, 10, 30, plan=plan(dropped, launch=LAUNCH_DROP, t0=10, t1=30, pitch_bytes=c.cap * t, after_len=180, after_pos_off=60))
        for n in (1, 5, 300, 9000):
            add(f'{gn}_import_{n}', IMPORT, g, dropped, n, plan=plan(dropped, reserve=200 + n, launch=CANON_SCATTER, t0=200, t1=n, pitch_bytes=c.cap * t, after_len=200 + n))
        add(f'{gn}_import_nothing', IMPORT, g, c, 0, plan=plan(c, nothing=1))
        add(f'{gn}_import_negative', IMPORT, g, c, -3, refusal=(MMD_ERANGE, 'kv_import of -3 tokens'))
        for n in (0, 300, 9000):
            add(f'{gn}_debug_set_len_{n}', DEBUG_SET_LEN, g, c, n, plan=plan(c, reserve=n, after_len=n))
        # ---- what a held stash refuses, what an unstash needs ------------------------------------------------------------------
        add(f'{gn}_drop_stashed', DROP, g, held, 10, 20, refusal=(MMD_EINVAL, 'kv_drop while tokens [120, 180) are stashed'))
        add(f'{gn}_import_stashed', IMPORT, g, held, 5, refusal=(MMD_EINVAL, 'kv_import while tokens [120, 180) are stashed'))
        add(f'{gn}_fork_stashed', FORK, g, held, 5, src=src, refusal=(MMD_EINVAL, 'kv_fork onto a stream whose tokens [120, 180) are stashed'))
        add(f'{gn}_fork_beyond', FORK, g, dst, 201, src=src, refusal=(MMD_ERANGE, 'kv_fork of 201 tokens from a context of 200'))
        add(f'{gn}_fork_negative', FORK, g, dst, -1, src=src, refusal=(MMD_ERANGE, 'kv_fork of -1 tokens'))
        # (a fork onto itself or across contexts is refused in model.hip, in front of the plan: those two checks compare pointers, which a plan of integers never sees)
        add(f'{gn}_unstash_none', UNSTASH, g, c, refusal=(MMD_EINVAL, 'kv_unstash without a (still valid) stash'))
        add(f'{gn}_unstash_elsewhere', UNSTASH, g, held, refusal=(MMD_EINVAL, 'the arena holds 150 tokens, the stash continues a context of 120'))
        # ---- the caller's buffers --------------------------------------------------------------------------------------------
        for op, a, b in ((EXPORT, 0, 5), (IMPORT, 5, 0)):
            add(f'{gn}_{OPS[op]}_missing', op, g, c, a, b, bufs=BUF_MISSING, refusal=(MMD_EINVAL, f'kv_{OPS[op]}: a canonical buffer is missing'))
            add(f'{gn}_{OPS[op]}_misaligned', op, g, c, a, b, bufs=BUF_MISALIGNED, refusal=(MMD_EINVAL, f'kv_{OPS[op]}: the canonical buffers must be 16-byte aligned'))

    # ---- the canonical form's limits (model.hip:1238): token bytes a multiple of 16 and at most 1 KiB, at most 65535 rows; both sides of each -----------------------
    for name, g, ok in (('tok_24', Geom(2, 3, 12, 2), False), ('tok_16', Geom(2, 3, 8, 2), True), ('tok_1024', Geom(2, 3, 256, 4), True), ('tok_1040', Geom(2, 3, 260, 4), False),
                        ('rows_65535', Geom(21845, 3, 16, 2), True), ('rows_65536', Geom(16384, 4, 16, 2), False)):
        c = State(200, 0, 256, 256, -1, -1)
        for op, a, b in ((EXPORT, 0, 5), (IMPORT, 5, 0)):
            if not ok:
                add(f'canon_{name}_{OPS[op]}', op, g, c, a, b, refusal=(MMD_EINVAL, f'kv_{OPS[op]}: head_dim {g.head_dim} x {g.elem} bytes (a multiple of 16, at most 1 KiB) or {g.layers} x {g.kv_heads} rows not supported'))
            elif op == EXPORT:
                add(f'canon_{name}_export', op, g, c, a, b, plan=plan(c, launch=CANON_GATHER, t0=0, t1=5, pitch_bytes=256 * tok(g)))
            else:
                add(f'canon_{name}_import', op, g, c, a, b, plan=plan(c, reserve=205, launch=CANON_SCATTER, t0=200, t1=5, pitch_bytes=256 * tok(g), after_len=205))

    # ---- the width guard: a row wider than 2^31 - 1 four-byte units is more than one copy launch takes.  Stated from a large state alone: a plan touches no memory ------
    for gn, g in GEOMS.items():
        t = tok(g)
        wide = (INT_MAX + 1) * 4 // t                      # the first token count whose bytes no longer fit: 2^25 at 256 bytes per token, 2^28 at 32; a multiple of 64
        assert wide % L.BLK == 0 and wide * t // 4 == INT_MAX + 1
        big = State(2 * wide, 0, 4 * wide, 2 * wide, -1, -1)
        msg = '{}: {} tokens are more than one copy launch takes'
        add(f'{gn}_wide_stash', STASH, g, big, 0, wide, refusal=(MMD_EINVAL, msg.format('kv_stash', wide)))
        add(f'{gn}_wide_stash_v_alone', STASH, g, big, 1, wide - 1, refusal=(MMD_EINVAL, msg.format('kv_stash', wide - 2)))          # K fits; V's blocks [0, wide) do not
        sp = span(g, big.cap, 64, wide, ROWS_OUT)
        add(f'{gn}_widest_stash', STASH, g, big, 64, wide, plan=plan(big, stash_bytes=rows(g) * sp['v_bytes'], after_stash_from=64, after_stash_to=wide, **sp))
        held = State(wide, 0, 4 * wide, 2 * wide, wide, 2 * wide)
        add(f'{gn}_wide_unstash', UNSTASH, g, held, refusal=(MMD_EINVAL, msg.format('kv_unstash', wide)))
        add(f'{gn}_wide_fork', FORK, g, State(0, 0, 2 * wide, 256, -1, -1), wide, src=big, refusal=(MMD_EINVAL, msg.format('kv_fork', wide)))
        add(f'{gn}_wide_fork_by_a_block', FORK, g, State(0, 0, 2 * wide, 256, -1, -1), wide - 63, src=big, refusal=(MMD_EINVAL, msg.format('kv_fork', wide - 63)))
        dst = State(0, 0, 2 * wide, 256, -1, -1)
        add(f'{gn}_widest_fork', FORK, g, dst, wide - 64, src=big,
            plan=plan(dst, reserve=wide - 64, after_len=wide - 64, **span(g, dst.cap, 0, wide - 64, ROWS_IN, other4=big.cap * t // 4)))
        # debug_read: the limit is on kv_heads x width
        per_head = -(-(INT_MAX // g.kv_heads + 1) * 4 // t // L.BLK) * L.BLK          # the first whole-block count whose width is beyond INT_MAX // kv_heads
        assert per_head * t // 4 > INT_MAX // g.kv_heads >= (per_head - L.BLK) * t // 4 and per_head <= big.mapped
        add(f'{gn}_wide_debug_read', DEBUG_READ, g, big, 0, per_head, refusal=(MMD_EINVAL, msg.format('kv_debug_read', per_head)))
        add(f'{gn}_widest_debug_read', DEBUG_READ, g, big, 0, per_head - L.BLK, plan=plan(big, **span(g, big.cap, 0, per_head - L.BLK, ROWS_OUT, n_rows=g.kv_heads)))

    # ---- the order of checks: two refusals apply, the earlier one of the entry point wins (lines of model.hip) ------------------------------------------------------
    g, c = B7, ctx(B7)
    held = ctx(B7, 150, stash=(120, 180))
    bad = Geom(2, 3, 12, 2)
    wide = (INT_MAX + 1) * 4 // tok(g)
    big = State(2 * wide, 0, 4 * wide, 2 * wide, -1, -1)
    add('order_stash_outside_before_wide', STASH, g, big, -1, wide, refusal=(MMD_ERANGE, 'outside the context'))          # :1175, then the copy's arithmetic (:1178-1187)
    add('order_unstash_none_before_elsewhere', UNSTASH, g, ctx(B7, 5), refusal=(MMD_EINVAL, 'without a (still valid) stash'))          # :1194 before :1197 (5 != -1 as well)
    add('order_unstash_elsewhere_before_wide', UNSTASH, g, State(5, 0, 4 * wide, 2 * wide, wide, 2 * wide), refusal=(MMD_EINVAL, 'the stash continues a context of'))   # :1197, then :1201-1205
    add('order_drop_outside_before_stashed', DROP, g, held, 10, 151, refusal=(MMD_ERANGE, 'outside the context'))          # :1218 before :1219
    add('order_drop_stashed_before_empty', DROP, g, held, 10, 10, refusal=(MMD_EINVAL, 'are stashed'))          # :1219 before :1220
    add('order_export_outside_before_buffers', EXPORT, g, c, 5, 201, bufs=BUF_MISSING, refusal=(MMD_ERANGE, 'outside the context'))          # :1244 before :1246
    add('order_export_empty_before_buffers', EXPORT, bad, c, 5, 5, bufs=BUF_MISSING, plan=plan(c, nothing=1))          # :1245 before :1246
    add('order_export_missing_before_misfit', EXPORT, bad, c, 0, 5, bufs=BUF_MISSING, refusal=(MMD_EINVAL, 'a canonical buffer is missing'))          # :1236 before :1238
    add('order_export_misaligned_before_misfit', EXPORT, bad, c, 0, 5, bufs=BUF_MISALIGNED, refusal=(MMD_EINVAL, '16-byte aligned'))          # :1237 before :1238
    add('order_import_negative_before_stashed', IMPORT, g, held, -1, refusal=(MMD_ERANGE, 'kv_import of -1 tokens'))          # :1255 before :1256
    add('order_import_stashed_before_empty', IMPORT, g, held, 0, refusal=(MMD_EINVAL, 'are stashed'))          # :1256 before :1257
    add('order_import_empty_before_buffers', IMPORT, bad, c, 0, bufs=BUF_MISSING, plan=plan(c, nothing=1))          # :1257 before :1258
    add('order_import_missing_before_misfit', IMPORT, bad, c, 5, bufs=BUF_MISSING, refusal=(MMD_EINVAL, 'a canonical buffer is missing'))          # :1236 before :1238
    add('order_fork_stashed_before_beyond', FORK, g, held, 201, src=c, refusal=(MMD_EINVAL, 'are stashed'))          # :1277 before :1278
    add('order_fork_beyond_before_wide', FORK, g, State(0, 0, 4 * wide, 256, -1, -1), wide, src=ctx(B7, wide - 1), refusal=(MMD_ERANGE, f'from a context of {wide - 1}'))   # :1278 before :1283
    add('order_debug_read_layer_before_n', DEBUG_READ, g, c, 28, 65, refusal=(MMD_EINVAL, 'layer 28 of 28'))          # :1307 before :1308
    add('order_debug_read_n_before_wide', DEBUG_READ, g, State(0, 0, 4 * wide, 64, -1, -1), 0, wide, refusal=(MMD_EINVAL, 'within the 64 tokens backed by memory'))   # :1308 before :1312
    return out


ROWS = _rows()

# ---- growth ------------------------------------------------------------------------------------------------------------------------------------
MiB = 1 << 20
CHUNK_CASES = [(256, 2 * MiB), (256, 4096), (32, 2 * MiB), (512, 2 * MiB)]          # (bytes per token, allocation granularity)
CHUNK_KNOWN = {(256, 2 * MiB): 8192, (256, 4096): 8192, (32, 2 * MiB): 65536}


def chunk_tokens(t, gran):
    """the smallest count of whole 64-token blocks whose bytes are whole pages, doubled until a row's chunk is at least 2 MiB"""
    block = L.BLK * t
    n = (block * gran // gcd(block, gran)) // t          # lcm(block bytes, page bytes), in tokens
    while n * t < 2 * MiB:
        n *= 2
    return n


RESERVATION_INITIALS = [256, 1024, 100000]
RESERVATION_CHUNK = 8192


def reservation_requests(initial):
    return [('default', 4 << 20), ('below_initial', initial // 2), ('one_chunk', RESERVATION_CHUNK)]


def up(n, m):
    return -(-n // m) * m


GROW_CASES = [(1024, 1025, 2048), (1024, 5000, 8192), (256, 257, 512), (256, 513, 1024), (4096, 8192, 8192), (320, 100000, 163840)]          # (cap, need, the doubling)
