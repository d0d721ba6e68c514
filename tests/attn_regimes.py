"""The attention dispatch regimes of attn_plan / attn_plan_decode_multi (mmduet_amd/csrc/attn_plan.h), one row per regime: which form (the number
mmd_op_attention_last_form reports) and how many key splits the dispatch must choose, on both sides of every threshold.  Plain data (imports without a GPU):
tests/test_attn_plan_host.py asks the planner about every row on the host, tests/test_gpu_attn_regimes.py runs every row that mmd_op_attention can reach on the device.

A row is (name, reach, layout, dtype, S, nh, nkv, d, n_ctx, causal, variant, over, form, splits, geom):
  * reach -- 'op': mmd_op_attention builds exactly these AttnArgs (the GPU test runs the row);  'host': host-only.  mmd_op_attention hands the kernels row-major K / V
    and transposes V only for the forced variants 3, 5 and 6, so it reaches the GQA-128 forms through those variants alone: the AUTOMATIC choices over the arena (the
    w1 rule, the chunk rule), the graph-replayed and slab-fed decode forms, the tower's fused-qkv layout, other workspaces than 128 MB, form 9 and every rejection are
    host-only rows.  On the device those are covered by the model-level tests of tests/test_gpu_production.py (benign data) and of tests/test_gpu_llm_stress.py (a sink
    key, q / k biases of 50 .. 60, outlier channels and saturated gates over live contexts: forms 4, 5, 8 and 9, the graph-replayed and the slab-fed decode); the tower rows (tower_d72, tower_d72_pooled_queries,
    tower_d72_f16, tower_d72_f32: the fused [tokens, 3C] layout, batch strides, 196 gathered query rows over 729 keys) also by tests/test_gpu_tower_stress.py, on
    peaked scores (three register keys at +30 .. +80) and outlier channels, in the fp32, bf16 and both fp16 towers.
  * layout -- which caller's AttnArgs build_args() builds: 'op' mmd_op_attention (K / V [nkv, cap, d], cap = n_ctx + S rounded up to 64, 128 MB of workspace);  'arena' the
    LLM step (the same with the transposed V arena);  'tower' the vision tower (q / k / v inside the fused [tokens, 3C] qkv rows, a batch of 4);  'multi'
    launch_attention_decode_multi (form 9: `nseg` streams of S rows).  `over` overrides single fields (a smaller workspace, dyn, qkv_slabs, an A/B switch ...).
  * form, splits -- 1 one wave per row, 2 16-row MFMA, 3 / 4 attn_gqa128_kernel on 64- / 128- and 256-row blocks, 5 attn_gqa128_w1_kernel, 6 attn_rowmajor_kernel,
    7 attn_d72_ring_kernel, 8 attn_gqa128_chunk_kernel (splits = the most parts a unit may have), 9 several streams' decode rows;  INVALID: the launcher returns an
    invalid-value error.
  * geom -- what can be derived by hand besides: qblocks (grid.x) and inst = (RT, NSLOT, WAVES) of attn_gqa128_kernel, qblocks / block_rows of the w1 kernel, nb (blocks of
    the contiguous decomposition), dp of attn_mfma_kernel<DP>, inst = (NC, DVT, EXACT) of attn_rowmajor_kernel.

Where the values come from.  Every non-chunk row is what the dispatch code did BEFORE the planner existed -- the launchers of that commit were run row by row (their decision
is host arithmetic; form and splits were read back through its attn_last_form) -- and every 'op' row was confirmed on an MI355X through mmd_op_attention_last_form of that
commit's library.  The automatic chunk rows (form 8 at variant 0) were derived by hand from that code: blocks = 4 cdiv(7 S, 256) >= 40 from S = 330;  the linear tile count
W = 4 sum_b tiles(b), W / 256 >= 14 from 951 keys at S = 1274;  one split with >= 80 % of the last round filled (208 of 256 blocks) from S = 1866 at 15 000 keys;
parts_max = tmax / (W / 256) + 2 = 3 at S = 1274 over 15 000 keys, 3 x 35 672 rows x 520 B = 55 648 320 B of workspace."""
from collections import namedtuple

BF16, F32, F16 = 'bf16', 'f32', 'f16'
DTYPE_CODE = {F32: 0, BF16: 1, F16: 2}          # mmd_dtype, and the launcher's internal IEEE-half code
INVALID = -1                                     # ATTN_PLAN_INVALID
WS_BYTES = 128 << 20                             # what mmd_op_attention allocates
# 16-byte-aligned fake addresses: the planner looks at null / non-null / alignment only
Q, K, V, WS, DYN, SLABS, SEGS = (0x10000000 * (i + 1) for i in range(7))
Q7 = (28, 4, 128)

Row = namedtuple('Row', 'name reach layout dtype S nh nkv d n_ctx causal variant over form splits geom')


def build_args(row):
    """the AttnArgs (and AttnTuning) fields a caller of the row's layout hands to the dispatch; fields that are not named are 0 / null"""
    S, nh, d, n_ctx = row.S, row.nh, row.d, row.n_ctx
    cap = (n_ctx + S + 63) // 64 * 64
    a = dict(dtype=DTYPE_CODE[row.dtype], S=S, nh=nh, nkv=row.nkv, d=d, n_ctx=n_ctx, causal=int(row.causal), batch=1, variant=row.variant, ldq=nh * d, ldo=nh * d, q=Q, K=K, V=V,
             ws=WS, ws_bytes=WS_BYTES, decode_ring=1, vit_ring=1)
    if row.layout == 'op':
        a.update(k_hs=cap * d, k_ts=d, v_hs=cap * d, v_ts=d, v_transposed=int(row.variant in (3, 5, 6)))
    elif row.layout in ('arena', 'multi'):
        a.update(k_hs=cap * d, k_ts=d, v_hs=cap * d, v_ts=d, v_transposed=1)
        if row.layout == 'multi':
            a.update(multi=1, segs=SEGS, K=0, V=0)
    else:
        assert row.layout == 'tower', row.layout
        C = nh * d
        a.update(ldq=C, ldo=C, k_hs=d, k_ts=3 * C, v_hs=d, v_ts=3 * C, batch=4, q_bstride=S * C, kv_bstride=(n_ctx + S) * 3 * C, o_bstride=S * C, K=K + 2 * C, V=K + 4 * C)
    a.update(row.over)
    return a


ROWS = [
    Row('llm_S1_n0', 'host', 'arena', BF16, 1, 28, 4, 128, 0, True, 0, {}, 3, 1, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('llm_S1_n100', 'host', 'arena', BF16, 1, 28, 4, 128, 100, True, 0, {}, 3, 2, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('llm_S1_n15000', 'host', 'arena', BF16, 1, 28, 4, 128, 15000, True, 0, {}, 3, 59, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('llm_S2_n100', 'host', 'arena', BF16, 2, 28, 4, 128, 100, True, 0, {}, 3, 2, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('llm_S2_n15000', 'host', 'arena', BF16, 2, 28, 4, 128, 15000, True, 0, {}, 3, 59, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('llm_S3_n100', 'host', 'arena', BF16, 3, 28, 4, 128, 100, True, 0, {}, 3, 1, {'qblocks': 1, 'inst': (1, 2, 4)}),
    Row('llm_S3_n15000', 'host', 'arena', BF16, 3, 28, 4, 128, 15000, True, 0, {}, 5, 59, {'qblocks': 1, 'block_rows': 32}),
    Row('llm_S9_n1000', 'host', 'arena', BF16, 9, 28, 4, 128, 1000, True, 0, {}, 3, 8, {'qblocks': 1, 'inst': (1, 2, 4)}),
    Row('llm_S10_n1000', 'host', 'arena', BF16, 10, 28, 4, 128, 1000, True, 0, {}, 4, 8, {'qblocks': 1, 'inst': (2, 2, 4)}),
    Row('llm_S10_n4085', 'host', 'arena', BF16, 10, 28, 4, 128, 4085, True, 0, {}, 4, 32, {'qblocks': 1, 'inst': (2, 2, 4)}),
    Row('llm_S10_n4086', 'host', 'arena', BF16, 10, 28, 4, 128, 4086, True, 0, {}, 5, 32, {'qblocks': 1, 'block_rows': 80}),
    Row('llm_S49_n15000', 'host', 'arena', BF16, 49, 28, 4, 128, 15000, True, 0, {}, 5, 30, {'qblocks': 2, 'block_rows': 176}),
    Row('llm_S109_n15000', 'host', 'arena', BF16, 109, 28, 4, 128, 15000, True, 0, {}, 5, 20, {'qblocks': 3, 'block_rows': 256}),
    Row('llm_S110_n15000', 'host', 'arena', BF16, 110, 28, 4, 128, 15000, True, 0, {}, 4, 17, {'qblocks': 7, 'inst': (2, 2, 4)}),
    Row('llm_S146_n15000', 'host', 'arena', BF16, 146, 28, 4, 128, 15000, True, 0, {}, 4, 16, {'qblocks': 8, 'inst': (2, 2, 4)}),
    Row('llm_S147_n15000', 'host', 'arena', BF16, 147, 28, 4, 128, 15000, True, 0, {}, 4, 12, {'qblocks': 5, 'inst': (2, 4, 8)}),
    Row('llm_S329_n15000', 'host', 'arena', BF16, 329, 28, 4, 128, 15000, True, 0, {}, 4, 7, {'qblocks': 9, 'inst': (2, 4, 8)}),
    Row('llm_S330_n15000', 'host', 'arena', BF16, 330, 28, 4, 128, 15000, True, 0, {}, 8, 8, {'nb': 256}),
    Row('llm_S1274_n950', 'host', 'arena', BF16, 1274, 28, 4, 128, 950, True, 0, {}, 4, 3, {'qblocks': 35, 'inst': (2, 4, 8)}),
    Row('llm_S1274_n951', 'host', 'arena', BF16, 1274, 28, 4, 128, 951, True, 0, {}, 8, 4, {'nb': 256}),
    Row('llm_S1865_n15000', 'host', 'arena', BF16, 1865, 28, 4, 128, 15000, True, 0, {}, 8, 3, {'nb': 256}),
    Row('llm_S1866_n15000', 'host', 'arena', BF16, 1866, 28, 4, 128, 15000, True, 0, {}, 4, 1, {'qblocks': 52, 'inst': (2, 4, 8)}),
    Row('llm_S1274_n15000', 'host', 'arena', BF16, 1274, 28, 4, 128, 15000, True, 0, {}, 8, 3, {'nb': 256}),
    Row('llm_S1911_n15000', 'host', 'arena', BF16, 1911, 28, 4, 128, 15000, True, 0, {}, 4, 1, {'qblocks': 53, 'inst': (2, 4, 8)}),
    Row('llm_S1911_n0', 'host', 'arena', BF16, 1911, 28, 4, 128, 0, True, 0, {}, 4, 1, {'qblocks': 53, 'inst': (2, 4, 8)}),
    Row('llm_S1274_n15000_ws_3_parts', 'host', 'arena', BF16, 1274, 28, 4, 128, 15000, True, 0, {'ws_bytes': 55648320}, 8, 3, {'nb': 256}),
    Row('llm_S1274_n15000_ws_under_3_parts', 'host', 'arena', BF16, 1274, 28, 4, 128, 15000, True, 0, {'ws_bytes': 55648319}, 4, 1, {'qblocks': 35, 'inst': (2, 4, 8)}),
    Row('llm_S49_n15000_ws_2_splits', 'host', 'arena', BF16, 49, 28, 4, 128, 15000, True, 0, {'ws_bytes': 1426880}, 5, 2, {'qblocks': 2, 'block_rows': 176}),
    Row('llm_S49_n15000_ws_under_2_splits', 'host', 'arena', BF16, 49, 28, 4, 128, 15000, True, 0, {'ws_bytes': 1426879}, 5, 1, {'qblocks': 2, 'block_rows': 176}),
    Row('llm_S49_n1000_ws_under_2_splits', 'host', 'arena', BF16, 49, 28, 4, 128, 1000, True, 0, {'ws_bytes': 1426879}, 4, 1, {'qblocks': 3, 'inst': (2, 2, 4)}),
    Row('llm_S1_n15000_no_ws', 'host', 'arena', BF16, 1, 28, 4, 128, 15000, True, 0, {'ws': 0, 'ws_bytes': 0}, 3, 1, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('llm_S49_n15000_no_ws', 'host', 'arena', BF16, 49, 28, 4, 128, 15000, True, 0, {'ws': 0, 'ws_bytes': 0}, 4, 1, {'qblocks': 3, 'inst': (2, 2, 4)}),
    Row('llm_S1274_n15000_no_ws', 'host', 'arena', BF16, 1274, 28, 4, 128, 15000, True, 0, {'ws': 0, 'ws_bytes': 0}, 4, 1, {'qblocks': 35, 'inst': (2, 4, 8)}),
    Row('llm_S1_n15000_dyn', 'host', 'arena', BF16, 1, 28, 4, 128, 15000, True, 0, {'dyn': DYN, 'dyn_splits': 64}, 3, 64, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('llm_S1_n0_dyn', 'host', 'arena', BF16, 1, 28, 4, 128, 0, True, 0, {'dyn': DYN, 'dyn_splits': 64}, 3, 64, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('llm_S3_n15000_dyn', 'host', 'arena', BF16, 3, 28, 4, 128, 15000, True, 0, {'dyn': DYN, 'dyn_splits': 64}, 3, 64, {'qblocks': 1, 'inst': (1, 2, 4)}),
    Row('llm_S1_n15000_slabs', 'host', 'arena', BF16, 1, 28, 4, 128, 15000, True, 0, {'qkv_slabs': SLABS, 'n_slabs': 2}, 3, 59, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('llm_S9_n15000_slabs', 'host', 'arena', BF16, 9, 28, 4, 128, 15000, True, 0, {'qkv_slabs': SLABS, 'n_slabs': 4}, 3, 59, {'qblocks': 1, 'inst': (1, 2, 4)}),
    Row('llm_S1_n15000_two_slot', 'host', 'arena', BF16, 1, 28, 4, 128, 15000, True, 0, {'decode_ring': 0}, 3, 59, {'qblocks': 1, 'inst': (1, 2, 4)}),
    Row('llm_S49_n15000_v3', 'host', 'arena', BF16, 49, 28, 4, 128, 15000, True, 3, {}, 4, 40, {'qblocks': 3, 'inst': (2, 2, 4)}),
    Row('llm_S392_n15000_v3', 'host', 'arena', BF16, 392, 28, 4, 128, 15000, True, 3, {}, 4, 5, {'qblocks': 11, 'inst': (2, 4, 8)}),
    Row('llm_S1274_n15000_v3', 'host', 'arena', BF16, 1274, 28, 4, 128, 15000, True, 3, {}, 4, 5, {'qblocks': 35, 'inst': (2, 4, 8)}),
    Row('llm_S49_n15000_v5', 'host', 'arena', BF16, 49, 28, 4, 128, 15000, True, 5, {}, 5, 30, {'qblocks': 2, 'block_rows': 176}),
    Row('llm_S392_n15000_v5', 'host', 'arena', BF16, 392, 28, 4, 128, 15000, True, 5, {}, 5, 5, {'qblocks': 11, 'block_rows': 256}),
    Row('llm_S1274_n15000_v5', 'host', 'arena', BF16, 1274, 28, 4, 128, 15000, True, 5, {}, 5, 5, {'qblocks': 35, 'block_rows': 256}),
    Row('llm_S49_n15000_v6', 'host', 'arena', BF16, 49, 28, 4, 128, 15000, True, 6, {}, 8, 35, {'nb': 256}),
    Row('llm_S392_n15000_v6', 'host', 'arena', BF16, 392, 28, 4, 128, 15000, True, 6, {}, 8, 8, {'nb': 256}),
    Row('llm_S1274_n15000_v6', 'host', 'arena', BF16, 1274, 28, 4, 128, 15000, True, 6, {}, 8, 3, {'nb': 256}),
    Row('op_v3_S1_n0', 'op', 'op', BF16, 1, 28, 4, 128, 0, True, 3, {}, 3, 1, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('op_v3_S1_n100', 'op', 'op', BF16, 1, 28, 4, 128, 100, True, 3, {}, 3, 2, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('op_v3_S1_n15000', 'op', 'op', BF16, 1, 28, 4, 128, 15000, True, 3, {}, 3, 59, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('op_v3_S2_n15000', 'op', 'op', BF16, 2, 28, 4, 128, 15000, True, 3, {}, 3, 59, {'qblocks': 1, 'inst': (1, 4, 4)}),
    Row('op_v3_S3_n15000', 'op', 'op', BF16, 3, 28, 4, 128, 15000, True, 3, {}, 3, 59, {'qblocks': 1, 'inst': (1, 2, 4)}),
    Row('op_v3_S9_n1000', 'op', 'op', BF16, 9, 28, 4, 128, 1000, True, 3, {}, 3, 8, {'qblocks': 1, 'inst': (1, 2, 4)}),
    Row('op_v3_S10_n1000', 'op', 'op', BF16, 10, 28, 4, 128, 1000, True, 3, {}, 4, 8, {'qblocks': 1, 'inst': (2, 2, 4)}),
    Row('op_v3_S49_n15000', 'op', 'op', BF16, 49, 28, 4, 128, 15000, True, 3, {}, 4, 40, {'qblocks': 3, 'inst': (2, 2, 4)}),
    Row('op_v3_S146_n15000', 'op', 'op', BF16, 146, 28, 4, 128, 15000, True, 3, {}, 4, 16, {'qblocks': 8, 'inst': (2, 2, 4)}),
    Row('op_v3_S147_n15000', 'op', 'op', BF16, 147, 28, 4, 128, 15000, True, 3, {}, 4, 12, {'qblocks': 5, 'inst': (2, 4, 8)}),
    Row('op_v3_S392_n15000', 'op', 'op', BF16, 392, 28, 4, 128, 15000, True, 3, {}, 4, 5, {'qblocks': 11, 'inst': (2, 4, 8)}),
    Row('op_v3_S1274_n15000', 'op', 'op', BF16, 1274, 28, 4, 128, 15000, True, 3, {}, 4, 5, {'qblocks': 35, 'inst': (2, 4, 8)}),
    Row('op_v3_S1911_n15000', 'op', 'op', BF16, 1911, 28, 4, 128, 15000, True, 3, {}, 4, 1, {'qblocks': 53, 'inst': (2, 4, 8)}),
    Row('op_v3_S1911_n0', 'op', 'op', BF16, 1911, 28, 4, 128, 0, True, 3, {}, 4, 1, {'qblocks': 53, 'inst': (2, 4, 8)}),
    Row('op_v5_S10_n4086', 'op', 'op', BF16, 10, 28, 4, 128, 4086, True, 5, {}, 5, 32, {'qblocks': 1, 'block_rows': 80}),
    Row('op_v5_S49_n15000', 'op', 'op', BF16, 49, 28, 4, 128, 15000, True, 5, {}, 5, 30, {'qblocks': 2, 'block_rows': 176}),
    Row('op_v5_S109_n15000', 'op', 'op', BF16, 109, 28, 4, 128, 15000, True, 5, {}, 5, 20, {'qblocks': 3, 'block_rows': 256}),
    Row('op_v5_S392_n15000', 'op', 'op', BF16, 392, 28, 4, 128, 15000, True, 5, {}, 5, 5, {'qblocks': 11, 'block_rows': 256}),
    Row('op_v5_S1274_n15000', 'op', 'op', BF16, 1274, 28, 4, 128, 15000, True, 5, {}, 5, 5, {'qblocks': 35, 'block_rows': 256}),
    Row('op_v6_S37_n15000', 'op', 'op', BF16, 37, 28, 4, 128, 15000, True, 6, {}, 8, 35, {'nb': 256}),
    Row('op_v6_S49_n15000', 'op', 'op', BF16, 49, 28, 4, 128, 15000, True, 6, {}, 8, 35, {'nb': 256}),
    Row('op_v6_S392_n15000', 'op', 'op', BF16, 392, 28, 4, 128, 15000, True, 6, {}, 8, 8, {'nb': 256}),
    Row('op_v6_S1274_n15000', 'op', 'op', BF16, 1274, 28, 4, 128, 15000, True, 6, {}, 8, 3, {'nb': 256}),
    Row('op_v6_S1911_n15000', 'op', 'op', BF16, 1911, 28, 4, 128, 15000, True, 6, {}, 8, 3, {'nb': 256}),
    Row('op_auto_rowmajor_S63', 'op', 'op', BF16, 63, 28, 4, 128, 300, True, 0, {}, 2, 1, {'dp': 128}),
    Row('op_auto_rowmajor_S64', 'op', 'op', BF16, 64, 28, 4, 128, 300, True, 0, {}, 6, 1, {'inst': (4, 8, 0)}),
    Row('op_auto_rowmajor_S49_n15000', 'op', 'op', BF16, 49, 28, 4, 128, 15000, True, 0, {}, 2, 22, {'dp': 128}),
    Row('op_v2_d32', 'op', 'op', BF16, 49, 4, 1, 32, 300, True, 2, {}, 2, 1, {'dp': 32}),
    Row('op_v2_d16', 'op', 'op', BF16, 130, 4, 2, 16, 41, True, 2, {}, 2, 1, {'dp': 32}),
    Row('op_v2_d64_n3000', 'op', 'op', BF16, 7, 4, 2, 64, 3000, True, 2, {}, 2, 11, {'dp': 64}),
    Row('op_v2_d96', 'op', 'op', BF16, 33, 4, 4, 96, 100, True, 2, {}, 2, 1, {'dp': 96}),
    Row('op_auto_S20_d128_noncausal', 'op', 'op', BF16, 20, 8, 8, 128, 100, False, 0, {}, 2, 1, {'dp': 128}),
    Row('op_v1_bf16', 'op', 'op', BF16, 7, 4, 2, 16, 5, True, 1, {}, 1, 1, {}),
    Row('op_v1_f32', 'op', 'op', F32, 7, 4, 2, 16, 5, True, 1, {}, 1, 1, {}),
    Row('op_auto_f32', 'op', 'op', F32, 49, 4, 1, 32, 300, True, 0, {}, 1, 1, {}),
    Row('op_v4_d72_S729', 'op', 'op', BF16, 729, 16, 16, 72, 0, False, 4, {}, 7, 1, {}),
    Row('op_v4_d72_S70_n58', 'op', 'op', BF16, 70, 2, 2, 72, 58, False, 4, {}, 7, 1, {}),
    Row('op_v4_d72_causal', 'op', 'op', BF16, 70, 2, 2, 72, 58, True, 4, {}, 6, 1, {'inst': (3, 5, 1)}),
    Row('op_v4_d64', 'op', 'op', BF16, 577, 16, 16, 64, 0, False, 4, {}, 6, 1, {'inst': (2, 4, 0)}),
    Row('op_v4_d32', 'op', 'op', BF16, 130, 4, 4, 32, 0, False, 4, {}, 6, 1, {'inst': (1, 2, 0)}),
    Row('op_v4_d96', 'op', 'op', BF16, 130, 4, 4, 96, 0, False, 4, {}, 6, 1, {'inst': (3, 6, 0)}),
    Row('op_v4_d80', 'op', 'op', BF16, 130, 4, 4, 80, 0, False, 4, {}, 6, 1, {'inst': (3, 5, 1)}),
    Row('op_v4_d128', 'op', 'op', BF16, 130, 4, 4, 128, 0, False, 4, {}, 6, 1, {'inst': (4, 8, 0)}),
    Row('op_auto_d72_S64', 'op', 'op', BF16, 64, 3, 3, 72, 0, False, 0, {}, 7, 1, {}),
    Row('op_auto_d72_S63', 'op', 'op', BF16, 63, 3, 3, 72, 0, False, 0, {}, 2, 1, {'dp': 96}),
    Row('tower_d72', 'host', 'tower', BF16, 729, 16, 16, 72, 0, False, 0, {}, 7, 1, {}),
    Row('tower_d72_ring_off', 'host', 'tower', BF16, 729, 16, 16, 72, 0, False, 0, {'vit_ring': 0}, 6, 1, {'inst': (3, 5, 1)}),
    Row('tower_d72_pooled_queries', 'host', 'tower', BF16, 196, 16, 16, 72, 533, False, 0, {}, 7, 1, {}),
    Row('tower_d72_unaligned_K', 'host', 'tower', BF16, 729, 16, 16, 72, 0, False, 0, {'K': K + 8}, 6, 1, {'inst': (3, 5, 1)}),
    Row('tower_d64', 'host', 'tower', BF16, 577, 16, 16, 64, 0, False, 0, {}, 6, 1, {'inst': (2, 4, 0)}),
    Row('tower_d32', 'host', 'tower', BF16, 196, 8, 8, 32, 0, False, 0, {}, 6, 1, {'inst': (1, 2, 0)}),
    Row('tower_d96', 'host', 'tower', BF16, 196, 8, 8, 96, 0, False, 0, {}, 6, 1, {'inst': (3, 6, 0)}),
    Row('tower_d72_S63', 'host', 'tower', BF16, 63, 16, 16, 72, 0, False, 0, {}, 2, 1, {'dp': 96}),
    Row('tower_d72_f16', 'host', 'tower', F16, 729, 16, 16, 72, 0, False, 4, {}, 7, 1, {}),
    Row('tower_d64_f16', 'host', 'tower', F16, 577, 16, 16, 64, 0, False, 4, {}, 6, 1, {'inst': (2, 4, 0)}),
    Row('tower_f16_auto_S63', 'host', 'tower', F16, 63, 16, 16, 72, 0, False, 0, {}, INVALID, 1, {}),
    Row('tower_f16_v2', 'host', 'tower', F16, 729, 16, 16, 72, 0, False, 2, {}, INVALID, 1, {}),
    Row('tower_d72_f32', 'host', 'tower', F32, 729, 16, 16, 72, 0, False, 0, {}, 1, 1, {}),
    Row('multi_2_streams', 'host', 'multi', BF16, 1, 28, 4, 128, 0, True, 0, {'nseg': 2}, 9, 32, {'inst': (1, 4, 4)}),
    Row('multi_4_streams', 'host', 'multi', BF16, 1, 28, 4, 128, 0, True, 0, {'nseg': 4}, 9, 16, {'inst': (1, 4, 4)}),
    Row('multi_32_streams', 'host', 'multi', BF16, 1, 28, 4, 128, 0, True, 0, {'nseg': 32}, 9, 2, {'inst': (1, 4, 4)}),
    Row('multi_2_streams_S2', 'host', 'multi', BF16, 2, 28, 4, 128, 0, True, 0, {'nseg': 2}, 9, 32, {'inst': (1, 4, 4)}),
    Row('multi_4_streams_ws_for_5_splits', 'host', 'multi', BF16, 1, 28, 4, 128, 0, True, 0, {'nseg': 4, 'ws_bytes': 291200}, 9, 5, {'inst': (1, 4, 4)}),
    Row('multi_33_streams_8_kv', 'host', 'multi', BF16, 1, 56, 8, 128, 0, True, 0, {'nseg': 33}, INVALID, 1, {}),
    Row('multi_S3', 'host', 'multi', BF16, 3, 28, 4, 128, 0, True, 0, {'nseg': 2}, INVALID, 1, {}),
    Row('multi_no_ws', 'host', 'multi', BF16, 1, 28, 4, 128, 0, True, 0, {'nseg': 2, 'ws': 0, 'ws_bytes': 0}, INVALID, 1, {}),
    Row('multi_ws_under_2_splits', 'host', 'multi', BF16, 1, 28, 4, 128, 0, True, 0, {'nseg': 2, 'ws_bytes': 58239}, INVALID, 1, {}),
    Row('multi_65_streams', 'host', 'multi', BF16, 1, 28, 4, 128, 0, True, 0, {'nseg': 65}, INVALID, 1, {}),
    Row('multi_no_segs', 'host', 'multi', BF16, 1, 28, 4, 128, 0, True, 0, {'nseg': 2, 'segs': 0}, INVALID, 1, {}),
    Row('multi_5_slabs', 'host', 'multi', BF16, 1, 28, 4, 128, 0, True, 0, {'nseg': 2, 'qkv_slabs': SLABS, 'n_slabs': 5}, INVALID, 1, {}),
    Row('bad_slabs_not_gqa128', 'host', 'arena', BF16, 1, 28, 4, 128, 100, True, 2, {'qkv_slabs': SLABS, 'n_slabs': 2}, INVALID, 1, {}),
    Row('bad_slabs_65_rows', 'host', 'arena', BF16, 10, 28, 4, 128, 100, True, 3, {'qkv_slabs': SLABS, 'n_slabs': 2}, INVALID, 1, {}),
    Row('bad_slabs_5', 'host', 'arena', BF16, 1, 28, 4, 128, 100, True, 3, {'qkv_slabs': SLABS, 'n_slabs': 5}, INVALID, 1, {}),
    Row('bad_slabs_0', 'host', 'arena', BF16, 1, 28, 4, 128, 100, True, 3, {'qkv_slabs': SLABS, 'n_slabs': 0}, INVALID, 1, {}),
    Row('bad_f16_arena', 'host', 'arena', F16, 49, 28, 4, 128, 100, True, 0, {}, INVALID, 1, {}),
    Row('bad_v4_transposed', 'host', 'arena', BF16, 130, 28, 4, 128, 100, True, 4, {}, INVALID, 1, {}),
    Row('bad_v2_f32', 'host', 'op', F32, 49, 4, 1, 32, 300, True, 2, {}, INVALID, 1, {}),
    Row('bad_v2_d20', 'host', 'op', BF16, 49, 4, 1, 20, 300, True, 2, {}, INVALID, 1, {}),
    Row('bad_v3_d64', 'host', 'op', BF16, 49, 4, 1, 64, 300, True, 3, {}, INVALID, 1, {}),
    Row('bad_v3_row_major_V', 'host', 'op', BF16, 49, 28, 4, 128, 300, True, 3, {'v_transposed': 0}, INVALID, 1, {}),
    Row('bad_v5_d64', 'host', 'op', BF16, 49, 4, 1, 64, 300, True, 5, {}, INVALID, 1, {}),
    Row('bad_v5_dyn', 'host', 'arena', BF16, 49, 28, 4, 128, 15000, True, 5, {'dyn': DYN, 'dyn_splits': 64}, INVALID, 1, {}),
    Row('bad_v6_dyn', 'host', 'arena', BF16, 1274, 28, 4, 128, 15000, True, 6, {'dyn': DYN, 'dyn_splits': 64}, INVALID, 1, {}),
    Row('bad_v6_255_rows', 'host', 'arena', BF16, 36, 28, 4, 128, 15000, True, 6, {}, INVALID, 1, {}),
    Row('bad_v6_no_ws', 'host', 'arena', BF16, 1274, 28, 4, 128, 15000, True, 6, {'ws': 0, 'ws_bytes': 0}, INVALID, 1, {}),
    Row('bad_v6_129_row_blocks', 'host', 'arena', BF16, 4682, 28, 4, 128, 0, True, 6, {'ws_bytes': 1073741824}, INVALID, 1, {}),
    Row('llm_v6_128_row_blocks', 'host', 'arena', BF16, 4681, 28, 4, 128, 0, True, 6, {'ws_bytes': 1073741824}, 8, 3, {'nb': 256}),
    Row('bad_v6_ws_under_parts', 'host', 'arena', BF16, 1274, 28, 4, 128, 15000, True, 6, {'ws_bytes': 55648319}, INVALID, 1, {}),
    Row('bad_v1_d136', 'host', 'op', F32, 7, 2, 2, 136, 5, True, 1, {}, INVALID, 1, {}),
    Row('bad_v4_ldo_unaligned', 'host', 'tower', BF16, 729, 16, 16, 72, 0, False, 4, {'ldo': 1154}, INVALID, 1, {}),
]


def rows_by_name():
    return {r.name: r for r in ROWS}


OP_ROWS = [r for r in ROWS if r.reach == 'op']
