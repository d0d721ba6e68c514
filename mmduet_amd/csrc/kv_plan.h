// kv_plan.h -- the stream KV arena's geometry, its span operations and its growth, and nothing else.  Pure host functions: no GPU header, no runtime call, no environment;
// they compile with the host C++17 compiler alone (tests/test_kv_plan_host.py runs the table of tests/kv_plan_cases.py through them without a GPU).
//   KvGeom       the only place the token <-> byte conversions and the V block size are written
//   kv_plan()    one operation on a stream's arena (KV_DROP in two forms: flags): refused (code and message), nothing to do, or what must have memory behind it, what is launched over which spans and the
//                bookkeeping the stream has afterwards.  kv_run (model.hip) does what it says, in that order.
//   kv_plan_spans()   mmd_kv_drop_spans: a LIST of spans in one owner walk per 64 of them -- the same contract, the launches as a list of retained segments
//   kv_vmm_*, kv_grow_*   the capacities growth tries: the chunk of the virtual-memory arena, the virtual reservations of mmd_stream_create, the fallback arena's reallocation
#pragma once
#include <stdio.h>
#include <vector>
#include "gemm_plan.h"          // round_up, the MMD_ codes

// ---- geometry ----------------------------------------------------------------------------------------------------------
// K and V are [layers][kv_heads][cap][head_dim]: `cap` is the row STRIDE in tokens (the reserved virtual capacity), a row is one (layer, kv head).  K holds rotated token
// rows; V holds transposed 64-token blocks, so whatever moves V moves whole blocks.
struct KvGeom {
    int layers = 0, kv_heads = 0, head_dim = 0, elem_bytes = 0;
    static constexpr int64_t BLK = 64;                                 // tokens per V block
    size_t tok_bytes() const { return (size_t)head_dim * elem_bytes; }
    size_t rows() const { return (size_t)layers * kv_heads; }
    size_t pitch_bytes(int64_t cap) const { return (size_t)cap * tok_bytes(); }
    size_t layer_bytes(int64_t cap) const { return (size_t)kv_heads * pitch_bytes(cap); }
    size_t arena_bytes(int64_t cap) const { return (size_t)layers * layer_bytes(cap); }          // of K, and of V
    static int64_t block_floor(int64_t t) { return t / BLK * BLK; }    // the first slot of t's block (t >= 0)
    static int64_t block_ceil(int64_t t) { return round_up(t, BLK); }  // the end of the last block that holds a slot below t
};
// a stream's bookkeeping
struct KvState {
    int64_t len = 0;                   // live tokens
    int64_t pos_off = 0;               // tokens dropped in front of the live ones: the RoPE position of slot t is t + pos_off
    int64_t cap = 0, mapped = 0;       // row stride; tokens with memory behind them
    int64_t stash_from = -1, stash_to = -1;          // the span set aside by a stash (-1: none)
};

// ---- one operation -----------------------------------------------------------------------------------------------------
enum { KV_TRUNCATE = 0,                // a = n: keep the first n tokens
       KV_RESET,
       KV_STASH,                       // a = from, b = to
       KV_UNSTASH,
       KV_DROP,                        // a = from, b = to
       KV_EXPORT,                      // a = from, b = to, the canonical buffers
       KV_IMPORT,                      // a = n, the canonical buffers
       KV_SET_POSITION,                // a = the RoPE position of the next token
       KV_FORK,                        // a = n; the state is the destination's, `src` the source's (that the two are distinct streams of one context is model.hip's check:
                                       // it compares pointers)
       KV_DEBUG_SET_LEN,               // a = n (n < 0 is the entry point's plain MMD_EINVAL, beside its null check)
       KV_DEBUG_READ,                  // a = layer, b = n, the output buffers
       KV_OPS };
enum { KV_BUF_OK = 0, KV_BUF_MISSING, KV_BUF_MISALIGNED };          // the caller's buffer pair: both there and 16-byte aligned, one missing, one misaligned
enum { KV_LAUNCH_NONE = 0,
       KV_ROWS_OUT,                    // launch_copy_rows for K, then for V: strided rows out of the arena ...
       KV_ROWS_IN,                     // ... into it
       KV_LAUNCH_DROP,                 // launch_kv_drop(t0, t1, len)
       KV_CANON_GATHER,                // launch_kv_canon: tokens [t0, t0 + t1) out of the arena into the canonical form ...
       KV_CANON_SCATTER,               // ... out of the canonical form into the arena
       KV_LAUNCH_DROP_SHIFT };         // launch_kv_drop_shift(t0, t1, len): KV_DROP with KV_F_SHIFT
enum { KV_F_SHIFT = 1 };               // kv_plan's flags.  KV_F_SHIFT (KV_DROP only): the keys behind the span are turned back by the span's length and the position shrinks with the length
constexpr int64_t KV_COPY_MAX_COLS = 0x7fffffff;          // launch_copy_rows takes a row's width as an int of 4-byte units
struct KvPlan {
    int rc = MMD_OK; char error[256] = {0};          // rc != MMD_OK: refused with this message
    bool nothing = false;              // an empty span: MMD_OK, and nothing else happens
    int64_t reserve = 0;               // tokens that must have memory behind them before anything is launched (0: none).  The fallback arena's growth changes `cap`: plan
                                       // again behind it
    size_t stash_bytes = 0;            // what each of the two stash buffers must hold
    int launch = KV_LAUNCH_NONE;
    // KV_ROWS_*: `copy_rows` rows; on the arena's side K's span starts k_off bytes into the arena and V's v_off, the pitch is `pitch4`; the other side's pitches are k_other4
    // and v_other4.  Widths (k_cols, v_cols) and pitches are in the 4-byte units launch_copy_rows takes.
    size_t k_off = 0, k_bytes = 0, v_off = 0, v_bytes = 0;
    int64_t k_cols = 0, v_cols = 0, pitch4 = 0, k_other4 = 0, v_other4 = 0; int copy_rows = 0;
    int64_t t0 = 0, t1 = 0;            // KV_LAUNCH_DROP, KV_LAUNCH_DROP_SHIFT: from, to.  KV_CANON_*: the first slot, the token count
    int64_t pitch_bytes = 0;           // KV_LAUNCH_DROP, KV_LAUNCH_DROP_SHIFT, KV_CANON_*: the arena's row pitch
    KvState after;                     // the stream's bookkeeping once the launches are queued (cap and mapped are kv_reserve's to change)
};
#define KV_REFUSE(code, ...) do { p.rc = (code); snprintf(p.error, sizeof(p.error), __VA_ARGS__); return p; } while (0)
// The strided copy of tokens [from, to) of every one of `rows` rows that start `base` bytes into the arena (launch_copy_rows: hipMemcpy2D rejects the GiB-scale row pitch of
// the virtual-memory arena).  K rows travel as they are.  V travels in whole blocks, which also carry -- unchanged -- the slots just below `from` and, up to the block's end,
// those at and above `to` (finite bytes: every byte of the arena was zero-filled before its first use).  other4 = 0: the other side is packed, each row as wide as its span.
// -> whether one launch takes the width (or the plan is refused, for every operation alike); `limit_rows` narrows that to limit_rows * cols (kv_debug_read's limit, as it
// always was)
static inline bool kv_plan_rows(KvPlan& p, const char* what, const KvGeom& g, int64_t cap, int launch, size_t base, int rows, int64_t from, int64_t to, int64_t other4, int limit_rows = 1) {
    const size_t tok = g.tok_bytes();
    const int64_t v_from = KvGeom::block_floor(from), v_to = KvGeom::block_ceil(to);
    p.launch = launch; p.copy_rows = rows;
    p.k_off = base + (size_t)from * tok; p.k_bytes = (size_t)(to - from) * tok;
    p.v_off = base + (size_t)v_from * tok; p.v_bytes = (size_t)(v_to - v_from) * tok;
    p.k_cols = (int64_t)(p.k_bytes / 4); p.v_cols = (int64_t)(p.v_bytes / 4); p.pitch4 = (int64_t)(g.pitch_bytes(cap) / 4);
    p.k_other4 = other4 ? other4 : p.k_cols; p.v_other4 = other4 ? other4 : p.v_cols;
    if ((p.k_cols > p.v_cols ? p.k_cols : p.v_cols) <= KV_COPY_MAX_COLS / limit_rows) return true;
    p.rc = MMD_EINVAL; snprintf(p.error, sizeof(p.error), "%s: %lld tokens are more than one copy launch takes", what, (long long)(to - from));
    return false;
}
// s: the stream's state (KV_FORK: the destination's, src the source's).  The checks of each operation stand in the order its entry point always made them.
static inline KvPlan kv_plan(int op, const KvGeom& g, const KvState& s, int64_t a = 0, int64_t b = 0, const KvState* src = nullptr, int bufs = KV_BUF_OK,
                             int flags = 0) {
    KvPlan p; p.after = s;
    const long long la = (long long)a, lb = (long long)b, len = (long long)s.len, sf = (long long)s.stash_from, st = (long long)s.stash_to;
    const bool outside = a < 0 || b < a || b > s.len, stashed = s.stash_from >= 0;          // a span [a, b) outside the context; a stash is held
    const int rows = (int)g.rows();
    const char* const names[KV_OPS] = {"kv_truncate", "stream_reset", "kv_stash", "kv_unstash", "kv_drop", "kv_export", "kv_import", "kv_set_position", "kv_fork", "kv_debug_set_len",
                                       "kv_debug_read"};
    const char* const what = op >= 0 && op < KV_OPS ? names[op] : "kv";
    auto clear_stash = [&p]() { p.after.stash_from = p.after.stash_to = -1; };
    switch (op) {
    case KV_TRUNCATE:
        if (a < 0 || a > s.len) KV_REFUSE(MMD_ERANGE, "kv_truncate(%lld) outside [0, %lld]", la, len);
        p.after.len = a;
        if (a < s.stash_from) clear_stash();          // the context a stash continued no longer exists
        break;
    case KV_RESET:
        p.after.len = 0; p.after.pos_off = 0; clear_stash();
        break;
    // Set the KV of tokens [from, to) aside and bring it back later: lets a caller roll the arena back to `from`, run something that overwrites those slots (a response whose
    // turn is NOT kept in the context) and then continue with the frames it had already encoded behind `from` instead of recomputing them.
    case KV_STASH:
        if (outside) KV_REFUSE(MMD_ERANGE, "kv_stash [%lld, %lld) outside the context (%lld tokens)", la, lb, len);
        if (!kv_plan_rows(p, what, g, s.cap, KV_ROWS_OUT, 0, rows, a, b, 0)) return p;
        p.stash_bytes = g.rows() * (p.k_bytes > p.v_bytes ? p.k_bytes : p.v_bytes);
        p.after.stash_from = a; p.after.stash_to = b;
        break;
    case KV_UNSTASH:
        if (!stashed) KV_REFUSE(MMD_EINVAL, "kv_unstash without a (still valid) stash");
        // the stash continues the context [0, from): the arena must stand exactly there (tokens >= from are overwritten, tokens of the V blocks just below `from` come back
        // with their stash-time values, so nothing below `from` may have changed either -- a truncate below `from` or a reset drops the stash)
        if (s.len != s.stash_from) KV_REFUSE(MMD_EINVAL, "kv_unstash: the arena holds %lld tokens, the stash continues a context of %lld (truncate to it first)", len, sf);
        if (!kv_plan_rows(p, what, g, s.cap, KV_ROWS_IN, 0, rows, s.stash_from, s.stash_to, 0)) return p;
        p.reserve = s.stash_to;
        p.after.len = s.stash_to; clear_stash();
        break;
    // Sliding context window: slots [from, to) leave every layer's arena, the tokens behind them move down bit for bit (keys keep the rotation they were written with) and
    // the stream goes on counting RoPE positions where it was: position = slot + pos_off.  One launch, no host synchronisation; pages stay mapped; slots at or above the
    // new length hold unspecified bits.
    case KV_DROP:
        if (outside) KV_REFUSE(MMD_ERANGE, "kv_drop [%lld, %lld) outside the context (%lld tokens)", la, lb, len);
        if (stashed) KV_REFUSE(MMD_EINVAL, "kv_drop while tokens [%lld, %lld) are stashed (unstash or drop the stash first)", sf, st);
        // KV_F_SHIFT (mmd_kv_drop_shift): the keys that move down are turned back by to - from positions on the way (launch_kv_drop_shift), so slot t holds position
        // t + pos_off again: the offset stays and the position shrinks with the length.  The rotation pairs dims (e, e + d/2) and moves 16-byte groups of both halves.
        if ((flags & KV_F_SHIFT) && (g.head_dim % 2 != 0 || (g.elem_bytes != 2 && g.elem_bytes != 4) || ((size_t)(g.head_dim / 2) * g.elem_bytes) % 16 != 0 || g.rows() > 65535))
            KV_REFUSE(MMD_EINVAL, "kv_drop_shift: head_dim %d x %d bytes (2- or 4-byte elements, half a head a multiple of 16 bytes) or %d x %d rows not supported", g.head_dim, g.elem_bytes,
                      g.layers, g.kv_heads);
        if (a == b) { p.nothing = true; break; }
        if (b < s.len) { p.launch = (flags & KV_F_SHIFT) ? KV_LAUNCH_DROP_SHIFT : KV_LAUNCH_DROP; p.t0 = a; p.t1 = b; p.pitch_bytes = (int64_t)g.pitch_bytes(s.cap); }          // (a dropped tail moves nothing)
        p.after.len = s.len - (b - a);
        if (!(flags & KV_F_SHIFT)) p.after.pos_off = s.pos_off + (b - a);
        break;
    // Snapshots.  The canonical form K, V [layers][kv heads][n][d] is token-major for both and has the context's dtype: nothing in it depends on the arena's capacity, pitch
    // or V blocking.  launch_kv_canon converts; a fork stays in arena form (the stash's strided copy between two pitches).
    case KV_EXPORT: case KV_IMPORT:
        if (op == KV_EXPORT) {
            if (outside) KV_REFUSE(MMD_ERANGE, "kv_export [%lld, %lld) outside the context (%lld tokens)", la, lb, len);
            if (a == b) { p.nothing = true; break; }
        } else {
            if (a < 0) KV_REFUSE(MMD_ERANGE, "kv_import of %lld tokens", la);
            if (stashed) KV_REFUSE(MMD_EINVAL, "kv_import while tokens [%lld, %lld) are stashed (unstash or drop the stash first)", sf, st);
            if (a == 0) { p.nothing = true; break; }
        }
        if (bufs == KV_BUF_MISSING) KV_REFUSE(MMD_EINVAL, "%s: a canonical buffer is missing", what);
        if (bufs == KV_BUF_MISALIGNED) KV_REFUSE(MMD_EINVAL, "%s: the canonical buffers must be 16-byte aligned", what);
        if (g.tok_bytes() % 16 != 0 || g.tok_bytes() > 1024 || g.rows() > 65535)
            KV_REFUSE(MMD_EINVAL, "%s: head_dim %d x %zu bytes (a multiple of 16, at most 1 KiB) or %d x %d rows not supported", what, g.head_dim, (size_t)g.elem_bytes, g.layers, g.kv_heads);
        if (op == KV_EXPORT) { p.launch = KV_CANON_GATHER; p.t0 = a; p.t1 = b - a; }
        else { p.launch = KV_CANON_SCATTER; p.t0 = s.len; p.t1 = a; p.reserve = s.len + a; p.after.len = s.len + a; }
        p.pitch_bytes = (int64_t)g.pitch_bytes(s.cap);
        break;
    case KV_SET_POSITION:
        if (a < s.len) KV_REFUSE(MMD_ERANGE, "kv_set_position(%lld) below the context's %lld tokens", la, len);
        p.after.pos_off = a - s.len;
        break;
    case KV_FORK:
        if (stashed) KV_REFUSE(MMD_EINVAL, "kv_fork onto a stream whose tokens [%lld, %lld) are stashed", sf, st);
        if (a < 0 || a > src->len) KV_REFUSE(MMD_ERANGE, "kv_fork of %lld tokens from a context of %lld", la, (long long)src->len);
        // V in whole blocks, like the stash: slots [n, block end) of the destination get the source's (finite) bytes
        if (!kv_plan_rows(p, what, g, s.cap, KV_ROWS_IN, 0, rows, 0, a, (int64_t)(g.pitch_bytes(src->cap) / 4))) return p;
        p.reserve = a;
        p.after.len = a; p.after.pos_off = src->pos_off;
        break;
    // measurement aid (tools/kv_growth_sweep.py): declare the first n slots of the arena live without computing them, to time a step at a given context length (the slots
    // hold zeros / stale data -- numerically meaningless, same memory traffic)
    case KV_DEBUG_SET_LEN:
        p.reserve = a; p.after.len = a;
        break;
    // test aid (tests/test_gpu_kv_arena.py): the first n tokens of one layer as the arena stores them -- K_out [nkv, n, d], V_out [nkv, n / 64, d, 64] (device, context
    // dtype).  Nothing is un-transposed and no address beyond token n of a row is touched (the row stride may be virtual).
    case KV_DEBUG_READ:
        if (bufs == KV_BUF_MISSING || a < 0 || a >= g.layers) KV_REFUSE(MMD_EINVAL, "kv_debug_read: layer %d of %d, or an output buffer missing", (int)a, g.layers);
        if (b < 0 || (b % KvGeom::BLK) != 0 || b > s.mapped) KV_REFUSE(MMD_EINVAL, "kv_debug_read: n = %lld must be a multiple of 64 within the %lld tokens backed by memory", lb, (long long)s.mapped);
        if (!kv_plan_rows(p, what, g, s.cap, KV_ROWS_OUT, (size_t)a * g.layer_bytes(s.cap), g.kv_heads, 0, b, 0, g.kv_heads)) return p;
        break;
    default:
        KV_REFUSE(MMD_EINVAL, "kv_plan: no operation %d", op);
    }
    return p;
}
#undef KV_REFUSE

// ---- many spans in one walk --------------------------------------------------------------------------------------------
// KV_DROP_SPANS (mmd_kv_drop_spans): the spans (from_i, to_i), i < n, ascending and disjoint, leave the context in ONE owner walk per launch (launch_kv_compact): every
// retained byte moves once, and with KV_F_SHIFT every retained key is turned back once, by the tokens dropped in front of it.  The operation has a span LIST for its
// argument, so it has a planning function of its own beside kv_plan() (whose operations 0 .. KV_OPS - 1 and signature stay as they are); kv_run_spans (model.hip) does
// what the plan says, launch by launch.
//   Normalised: empty spans are ignored, touching spans are merged.  A launch carries at most KV_SPANS_PER_LAUNCH retained SEGMENTS (src, count): the tokens between one
//   span and the next (or the end of the context); the destination is implied -- dst_0 is given, dst_{i+1} = dst_i + count_i -- and delta_i = src_i - dst_i, the tokens
//   dropped in front of segment i, grows strictly.  A final span that ends at `len` yields no segment.
//   More spans than one launch takes: the spans are cut into groups of KV_SPANS_PER_LAUNCH and each group is a complete compaction of its own -- of the whole context
//   behind the group's first span, tail included -- issued HIGHEST GROUP FIRST, so that the coordinates of a lower group are untouched by the launches before it.  The
//   tail behind a group moves once per group at or below it: more traffic than one pass, paid only beyond KV_SPANS_PER_LAUNCH spans.  (A device-resident table would
//   lift the limit; it is deliberately not built.)
constexpr int KV_SPANS_PER_LAUNCH = 64;
enum { KV_DROP_SPANS = KV_OPS + 1 };                                   // not an operation of kv_plan(): kv_plan_spans() plans it
enum { KV_LAUNCH_COMPACT = KV_LAUNCH_DROP_SHIFT + 1,                   // launch_kv_compact(segments, dst0, len_end), inv_freq null ...
       KV_LAUNCH_COMPACT_SHIFT };                                      // ... or the context's table: KV_F_SHIFT
struct KvSeg { int64_t src, count; };
struct KvCompact {
    int64_t dst0 = 0;                  // the first destination slot: the group's first span starts here
    int64_t len_in = 0, len_end = 0;   // the stream's length in front of this launch and behind it; no segment reaches beyond len_in, the last destination is len_end
    int nseg = 0; KvSeg seg[KV_SPANS_PER_LAUNCH];
};
struct KvSpansPlan {
    int rc = MMD_OK; char error[256] = {0};
    bool nothing = false;              // no span, or only empty ones: MMD_OK, and nothing else happens
    int launch = KV_LAUNCH_NONE;       // the kind of every launch in `launches` (NONE: the spans were a dropped tail, only the bookkeeping changes)
    int64_t pitch_bytes = 0;
    int64_t spans = 0, dropped = 0;    // normalised spans; tokens they hold
    std::vector<KvCompact> launches;   // in the order they are issued
    KvState after;
};
// spans: [n][2] in host memory (from, to); flags: KV_F_SHIFT or 0.  The checks stand in KV_DROP's order: the ranges, then the list's order, the stash, the head shape.
static inline KvSpansPlan kv_plan_spans(const KvGeom& g, const KvState& s, const int64_t* spans, int n, int flags = 0) {
    KvSpansPlan p; p.after = s;
#define KV_REFUSE(code, ...) do { p.rc = (code); snprintf(p.error, sizeof(p.error), __VA_ARGS__); return p; } while (0)
    if (n < 0 || (n > 0 && !spans)) KV_REFUSE(MMD_EINVAL, "kv_drop_spans: %d spans, or no span list", n);
    for (int i = 0; i < n; ++i) {
        const int64_t a = spans[2 * i], b = spans[2 * i + 1];
        if (a < 0 || b < a || b > s.len) KV_REFUSE(MMD_ERANGE, "kv_drop_spans: span %d [%lld, %lld) outside the context (%lld tokens)", i, (long long)a, (long long)b, (long long)s.len);
    }
    for (int i = 1; i < n; ++i)
        if (spans[2 * i] < spans[2 * i - 1])
            KV_REFUSE(MMD_EINVAL, "kv_drop_spans: span %d [%lld, %lld) %s span %d [%lld, %lld) (the spans must ascend and be disjoint)", i, (long long)spans[2 * i], (long long)spans[2 * i + 1],
                      spans[2 * i] < spans[2 * i - 2] ? "stands in front of" : "overlaps", i - 1, (long long)spans[2 * i - 2], (long long)spans[2 * i - 1]);
    if (s.stash_from >= 0) KV_REFUSE(MMD_EINVAL, "kv_drop_spans while tokens [%lld, %lld) are stashed (unstash or drop the stash first)", (long long)s.stash_from, (long long)s.stash_to);
    if ((flags & KV_F_SHIFT) && (g.head_dim % 2 != 0 || (g.elem_bytes != 2 && g.elem_bytes != 4) || ((size_t)(g.head_dim / 2) * g.elem_bytes) % 16 != 0 || g.rows() > 65535))
        KV_REFUSE(MMD_EINVAL, "kv_drop_shift: head_dim %d x %d bytes (2- or 4-byte elements, half a head a multiple of 16 bytes) or %d x %d rows not supported", g.head_dim, g.elem_bytes,
                  g.layers, g.kv_heads);
#undef KV_REFUSE
    std::vector<int64_t> norm(2 * (size_t)n);          // the normalised spans (norm[2 i], norm[2 i + 1]), i < m
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t a = spans[2 * i], b = spans[2 * i + 1];
        if (a == b) continue;
        if (m > 0 && norm[2 * m - 1] == a) norm[2 * m - 1] = b;
        else { norm[2 * m] = a; norm[2 * m + 1] = b; ++m; }
    }
    if (m == 0) { p.nothing = true; return p; }
    p.spans = m;
    const int groups = (m + KV_SPANS_PER_LAUNCH - 1) / KV_SPANS_PER_LAUNCH;
    int64_t cur = s.len;
    for (int gi = groups - 1; gi >= 0; --gi) {          // highest group first
        const int j = gi * KV_SPANS_PER_LAUNCH, k = j + KV_SPANS_PER_LAUNCH < m ? j + KV_SPANS_PER_LAUNCH : m;
        KvCompact c; c.dst0 = norm[2 * j]; c.len_in = cur;
        int64_t gone = 0;
        for (int i = j; i < k; ++i) {
            gone += norm[2 * i + 1] - norm[2 * i];
            const int64_t src = norm[2 * i + 1], end = i + 1 < k ? norm[2 * i + 2] : cur;          // the retained tokens behind span i: up to the next span of the group, or the whole tail
            if (end > src) { c.seg[c.nseg].src = src; c.seg[c.nseg].count = end - src; ++c.nseg; }
        }
        cur -= gone; c.len_end = cur; p.dropped += gone;
        if (c.nseg > 0) p.launches.push_back(c);          // (a dropped tail moves nothing)
    }
    if (!p.launches.empty()) { p.launch = (flags & KV_F_SHIFT) ? KV_LAUNCH_COMPACT_SHIFT : KV_LAUNCH_COMPACT; p.pitch_bytes = (int64_t)g.pitch_bytes(s.cap); }
    p.after.len = s.len - p.dropped;
    if (!(flags & KV_F_SHIFT)) p.after.pos_off = s.pos_off + p.dropped;
    return p;
}

// ---- growth ------------------------------------------------------------------------------------------------------------
// Every byte growth puts behind the arena is zero-filled before its first use: key tiles may cover slots beyond the live length (their P is masked to 0), so those slots
// must stay finite.
constexpr int64_t KV_MIN_TOKENS = 256;                                 // a stream's smallest first backing
constexpr int64_t KV_VIRTUAL_TOKENS_DEFAULT = (int64_t)4 << 20;        // the row stride reserved once: the HBM limit of the 7B model
constexpr int KV_MAX_RESERVATIONS = 64;
static inline int64_t kv_initial_tokens(int64_t asked) { return KvGeom::block_ceil(asked < KV_MIN_TOKENS ? KV_MIN_TOKENS : asked); }
// the virtual-memory arena's chunk: whole V blocks and whole pages, at least 2 MiB per row and step
static inline int64_t kv_vmm_chunk_tokens(size_t tok_bytes, size_t granularity) {
    int64_t ct = KvGeom::BLK; while (((size_t)ct * tok_bytes) % granularity != 0) ct += KvGeom::BLK;
    while ((size_t)ct * tok_bytes < ((size_t)2 << 20)) ct *= 2;
    return ct;
}
// the row strides mmd_stream_create tries to reserve, in order: the requested one, then halves down to what the first backing needs.  Each is rounded to whole chunks (the row
// stride must stay a multiple of the allocation granularity).  -> how many (at most KV_MAX_RESERVATIONS)
static inline int kv_vmm_reservations(int64_t initial_tokens, int64_t requested, int64_t chunk, int64_t* out) {
    const int64_t least = round_up(initial_tokens, chunk);
    int64_t vcap = round_up(requested < initial_tokens ? initial_tokens : requested, chunk);
    int n = 0;
    while (n < KV_MAX_RESERVATIONS) {
        out[n++] = vcap;
        if (vcap == least) break;
        const int64_t half = round_up(vcap / 2, chunk);
        vcap = half < least ? least : half;
    }
    return n;
}
// the fallback arena (plain allocation, growth by reallocation + copy) tries twice: doubling, then -- where that does not fit next to the old arena -- the need + 1/8 headroom
static inline int64_t kv_grow_doubled(int64_t cap, int64_t need) { int64_t ncap = cap * 2; while (ncap < need) ncap *= 2; return ncap; }
static inline int64_t kv_grow_exact(int64_t need) { return KvGeom::block_ceil(need + need / 8); }
// ... and carries a row's live bytes over: V is stored in whole blocks
static inline size_t kv_grow_copy_bytes(const KvGeom& g, int64_t len) { return (size_t)KvGeom::block_ceil(len) * g.tok_bytes(); }
