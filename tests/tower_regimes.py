"""The schedules of a vision-tower run (tower_plan of mmduet_amd/csrc/tower_plan.h), one row per regime: which plan it must take, on both sides of every term of
the sparse-last rule, in every residual and embed form, and on both sides of the row count at which fc1 and fc2 reach the ring.  Plain data (imports without a GPU):
tests/test_tower_plan_host.py asks tower_plan about every row on the host, tests/test_gpu_tower_regimes.py runs the rows a context reaches on the device and compares
`tower_last_plan()`.

A row is (name, mode, tower, B, for_pool, full_tower, env, ring, model, plan, refusal):
  * mode -- a key of MODES: model dtype and tower_f16 (0 the model dtype, 1 IEEE half with the fp32 residual stream, 2 IEEE half with the fp16 stream).
  * tower -- a key of TOWERS: the geometry.  'true' is SigLIP-so400m (C = 1152, 729 tokens, fc1 rows padded 4304 -> 4352) behind the 27 -> 7 bilinear pool;
    'small12' / 'small16' the 64-wide tower of test_fp16_tower_small_grids_fall_back_to_the_full_last_layer at grids 12 and 16, stride 4.
  * B, for_pool (the encode entry points; False: mmd_vision_tower), full_tower (mmd_vit_set_full_tower).
  * env -- MMDUET_NO_FUSE as the context was created under ('1' | '2': no piece-major intermediates).
  * ring -- None, or the argument of mmd_set_tower_share (a cap on the ring GEMMs' persistent grid: it changes their grid, never which kernel runs).
  * model -- TowerModel fields that differ from the tower's defaults (a class token, post-LayerNorm, another pool mode, ...).
  * plan -- what mmd_op_tower_last_plan must report, over FIELDS; None for a refused run, whose message is `refusal`.

Every plan was derived by hand from the rule as model.hip's comments and DESIGN.md state it:
  * the last layer runs on the U = 4 pout^2 rows of a frame the bilinear pool reads (pout = ceil(grid / stride)) when the run is for the pool, the full tower is not asked
    for, the pool is bilinear, U < tokens, there is no class token, no post-LayerNorm, no quick-GELU MLP, at least one layer, the context is not vision-only -- and, in a
    half tower, U >= 64 and B U > 64 (the half forms of the kernels exist for GEMMs above 64 rows and attention from 64 queries);
  * the projector runs on those rows under the first conditions alone (bilinear, U < tokens, no class token), and gathers them itself unless the sparse last layer left them;
  * fc1's output is piece-major when the automatic dispatch runs fc1 on the plain ring and fc2 on the ring.  From the ring rule of tests/gemm_regimes.py (M >= 512 and
    t = ceil(M / 256) ceil(N / 256) tiles with t >= 400, or t >= 192 filling >= 0.9 of whole waves of 256): fc2, N = 1152, five tile columns like 'vit_o', whose rows
    gemm_vit_o_11776 | 11777 and gemm_vit_o_20224 | 20225 pin the two edges -- ring for 11 777 <= M <= 13 056 (t = 235 .. 255) and from M = 20 225 (t = 400); fc1, N = 4352,
    17 tile columns -- ring for 3329 <= M <= 3840 (t = 238, 255) and from M = 5889 (t = 408).  Both: 11 777 .. 13 056 rows and from 20 225.  At 729 rows per frame that is
    B = 17 (12 393 rows; 16 -> 11 664, 18 -> 13 122) and B >= 28 (20 412; 27 -> 19 683); the compact block of 196 rows per frame reaches it at B = 61 (11 956; 60 -> 11 760).
    Never in the fp32 model (the ring kernels are 2-byte).
"""
from collections import namedtuple

F32, BF16, F16 = 0, 1, 2                                   # element types (MMD_F32, MMD_BF16, the launchers' MMD_F16)
RESID_EPI, RESID_F32, RESID_F16 = 0, 1, 2
EMBED_ADD_ROWS, EMBED_CLS, EMBED_F32 = 0, 1, 2
POOL_BILINEAR, POOL_AVERAGE, POOL_MAX, POOL_ADAPTIVE_AVG = 0, 1, 2, 3
MMD_ERANGE = -34
FIELDS = ('dt', 'resid', 'embed', 'sparse_last', 'pout', 'U', 'compact_rows', 'proj_compact', 'proj_gather', 'mlp_pm', 'mlp_pm_last', 'final_convert')

# mode -> (model dtype, tower_f16)
MODES = {'fp32': (F32, 0), 'bf16': (BF16, 0), 'fp16': (BF16, 1), 'fp16_resid16': (BF16, 2)}
TOWERS = {
    'true': dict(C=1152, heads=16, ipad=4352, grid=27, pool_stride=4, layers=2, max_batch=64),
    'small12': dict(C=64, heads=4, ipad=128, grid=12, pool_stride=4, layers=2, max_batch=8),
    'small16': dict(C=64, heads=4, ipad=128, grid=16, pool_stride=4, layers=2, max_batch=8),
}
TOWER_WS_BYTES = 32 << 20           # the tower's own split-K workspace

Row = namedtuple('Row', 'name mode tower B for_pool full_tower env ring model plan refusal')


def row(name, mode, tower, B, plan, for_pool=True, full_tower=False, env=None, ring=None, refusal=None, **model):
    return Row(name, mode, tower, B, for_pool, full_tower, dict(env or {}), ring, model, None if plan is None else tuple(plan), refusal)


ROWS = [
    # ---- the sparse / full gate in the 64-wide tower: grid 16 -> pout 4, U = 64 of 256 tokens; grid 12 -> pout 3, U = 36 of 144 ----
    #                                    dt  resid      embed           sparse pout U  rows  proj    pm    convert
    row('bf16_g16_b1', 'bf16', 'small16', 1, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 4, 64, 64, 1, 0, 0, 0, 0)),           # the guard is for half only
    row('bf16_g16_b2', 'bf16', 'small16', 2, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 4, 64, 128, 1, 0, 0, 0, 0)),
    row('bf16_g16_b3', 'bf16', 'small16', 3, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 4, 64, 192, 1, 0, 0, 0, 0)),
    row('bf16_g12_b1', 'bf16', 'small12', 1, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 3, 36, 36, 1, 0, 0, 0, 0)),
    row('bf16_g12_b2', 'bf16', 'small12', 2, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 3, 36, 72, 1, 0, 0, 0, 0)),
    row('bf16_g12_b3', 'bf16', 'small12', 3, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 3, 36, 108, 1, 0, 0, 0, 0)),
    row('fp16_g16_b1', 'fp16', 'small16', 1, (F16, RESID_F32, EMBED_F32, 0, 4, 64, 0, 1, 1, 0, 0, 0)),                  # B U = 64 | 128 of "> 64"
    row('fp16_g16_b2', 'fp16', 'small16', 2, (F16, RESID_F32, EMBED_F32, 1, 4, 64, 128, 1, 0, 0, 0, 0)),
    row('fp16_g16_b3', 'fp16', 'small16', 3, (F16, RESID_F32, EMBED_F32, 1, 4, 64, 192, 1, 0, 0, 0, 0)),
    row('fp16_g12_b1', 'fp16', 'small12', 1, (F16, RESID_F32, EMBED_F32, 0, 3, 36, 0, 1, 1, 0, 0, 0)),                  # U = 36 < 64: the full last layer at any B
    row('fp16_g12_b2', 'fp16', 'small12', 2, (F16, RESID_F32, EMBED_F32, 0, 3, 36, 0, 1, 1, 0, 0, 0)),
    row('fp16_g12_b3', 'fp16', 'small12', 3, (F16, RESID_F32, EMBED_F32, 0, 3, 36, 0, 1, 1, 0, 0, 0)),                  # (B U = 108 > 64 does not help)
    row('r16_g16_b1', 'fp16_resid16', 'small16', 1, (F16, RESID_F16, EMBED_ADD_ROWS, 0, 4, 64, 0, 1, 1, 0, 0, 1)),
    row('r16_g16_b2', 'fp16_resid16', 'small16', 2, (F16, RESID_F16, EMBED_ADD_ROWS, 1, 4, 64, 128, 1, 0, 0, 0, 1)),
    row('r16_g12_b2', 'fp16_resid16', 'small12', 2, (F16, RESID_F16, EMBED_ADD_ROWS, 0, 3, 36, 0, 1, 1, 0, 0, 1)),
    # ---- true width, every mode: 3 frames (588 compact rows), then fc1 / fc2 on either side of the ring: B = 16 | 17 | 18 and 27 | 28 ----
    row('fp32_true_b3', 'fp32', 'true', 3, (F32, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 588, 1, 0, 0, 0, 0)),
    row('fp32_true_b17', 'fp32', 'true', 17, (F32, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 3332, 1, 0, 0, 0, 0)),        # no 4-byte ring kernel
    row('bf16_true_b3', 'bf16', 'true', 3, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 588, 1, 0, 0, 0, 0)),
    row('bf16_true_b16', 'bf16', 'true', 16, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 3136, 1, 0, 0, 0, 0)),
    row('bf16_true_b17', 'bf16', 'true', 17, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 3332, 1, 0, 1, 0, 0)),
    row('bf16_true_b18', 'bf16', 'true', 18, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 3528, 1, 0, 0, 0, 0)),
    row('bf16_true_b27', 'bf16', 'true', 27, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 5292, 1, 0, 0, 0, 0)),
    row('bf16_true_b28', 'bf16', 'true', 28, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 5488, 1, 0, 1, 0, 0)),
    row('fp16_true_b3', 'fp16', 'true', 3, (F16, RESID_F32, EMBED_F32, 1, 7, 196, 588, 1, 0, 0, 0, 0)),
    row('fp16_true_b16', 'fp16', 'true', 16, (F16, RESID_F32, EMBED_F32, 1, 7, 196, 3136, 1, 0, 0, 0, 0)),
    row('fp16_true_b17', 'fp16', 'true', 17, (F16, RESID_F32, EMBED_F32, 1, 7, 196, 3332, 1, 0, 1, 0, 0)),
    row('fp16_true_b35', 'fp16', 'true', 35, (F16, RESID_F32, EMBED_F32, 1, 7, 196, 6860, 1, 0, 1, 0, 0)),              # the shipped tower batch
    row('r16_true_b3', 'fp16_resid16', 'true', 3, (F16, RESID_F16, EMBED_ADD_ROWS, 1, 7, 196, 588, 1, 0, 0, 0, 1)),
    row('r16_true_b16', 'fp16_resid16', 'true', 16, (F16, RESID_F16, EMBED_ADD_ROWS, 1, 7, 196, 3136, 1, 0, 0, 0, 1)),
    row('r16_true_b17', 'fp16_resid16', 'true', 17, (F16, RESID_F16, EMBED_ADD_ROWS, 1, 7, 196, 3332, 1, 0, 1, 0, 1)),
    # the compact last layer on either side of the ring: 60 | 61 frames (the full rows, 43 740 and more, are far above it)
    row('bf16_true_b60', 'bf16', 'true', 60, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 11760, 1, 0, 1, 0, 0)),
    row('bf16_true_b61', 'bf16', 'true', 61, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 11956, 1, 0, 1, 1, 0)),
    row('fp16_true_b61', 'fp16', 'true', 61, (F16, RESID_F32, EMBED_F32, 1, 7, 196, 11956, 1, 0, 1, 1, 0)),
    # ... with the piece-major intermediates switched off, and under a tower ring cap (the same kernels on a smaller grid)
    row('bf16_true_b17_no_fuse2', 'bf16', 'true', 17, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 3332, 1, 0, 0, 0, 0), env={'MMDUET_NO_FUSE': '2'}),
    row('bf16_true_b61_no_fuse1', 'bf16', 'true', 61, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 11956, 1, 0, 0, 0, 0), env={'MMDUET_NO_FUSE': '1'}),
    row('bf16_true_b17_no_fuse0', 'bf16', 'true', 17, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 3332, 1, 0, 1, 0, 0), env={'MMDUET_NO_FUSE': '0'}),
    row('fp16_true_b17_no_fuse2', 'fp16', 'true', 17, (F16, RESID_F32, EMBED_F32, 1, 7, 196, 3332, 1, 0, 0, 0, 0), env={'MMDUET_NO_FUSE': '2'}),
    row('bf16_true_b16_share', 'bf16', 'true', 16, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 3136, 1, 0, 0, 0, 0), ring=96),
    row('bf16_true_b17_share', 'bf16', 'true', 17, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 3332, 1, 0, 1, 0, 0), ring=96),
    row('fp16_true_b17_share', 'fp16', 'true', 17, (F16, RESID_F32, EMBED_F32, 1, 7, 196, 3332, 1, 0, 1, 0, 0), ring=96),
    # ---- the other terms of the sparse-last rule, each on its own at true width (the default side: the *_true_b3 rows) ----
    row('bf16_true_full_tower', 'bf16', 'true', 3, (BF16, RESID_EPI, EMBED_ADD_ROWS, 0, 7, 196, 0, 1, 1, 0, 0, 0), full_tower=True),
    row('fp16_true_full_tower', 'fp16', 'true', 3, (F16, RESID_F32, EMBED_F32, 0, 7, 196, 0, 1, 1, 0, 0, 0), full_tower=True),
    row('r16_true_full_tower_b17', 'fp16_resid16', 'true', 17, (F16, RESID_F16, EMBED_ADD_ROWS, 0, 7, 196, 0, 1, 1, 1, 0, 1), full_tower=True),
    row('bf16_true_not_for_pool', 'bf16', 'true', 3, (BF16, RESID_EPI, EMBED_ADD_ROWS, 0, 7, 196, 0, 0, 0, 0, 0, 0), for_pool=False),      # mmd_vision_tower: no projector follows
    row('fp16_true_not_for_pool_b17', 'fp16', 'true', 17, (F16, RESID_F32, EMBED_F32, 0, 7, 196, 0, 0, 0, 1, 0, 0), for_pool=False),
    row('bf16_true_stride1', 'bf16', 'true', 3, (BF16, RESID_EPI, EMBED_ADD_ROWS, 0, 27, 2916, 0, 0, 0, 0, 0, 0), pool_stride=1),          # U >= T: nothing to leave out
    row('bf16_true_stride2', 'bf16', 'true', 3, (BF16, RESID_EPI, EMBED_ADD_ROWS, 0, 14, 784, 0, 0, 0, 0, 0, 0), pool_stride=2),           # (784 of 729)
    row('bf16_true_stride3', 'bf16', 'true', 3, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 9, 324, 972, 1, 0, 0, 0, 0), pool_stride=3),
    row('bf16_true_average', 'bf16', 'true', 3, (BF16, RESID_EPI, EMBED_ADD_ROWS, 0, 7, 196, 0, 0, 0, 0, 0, 0), pool_mode=POOL_AVERAGE),
    row('bf16_true_max', 'bf16', 'true', 3, (BF16, RESID_EPI, EMBED_ADD_ROWS, 0, 7, 196, 0, 0, 0, 0, 0, 0), pool_mode=POOL_MAX),
    row('bf16_true_class_token', 'bf16', 'true', 3, (BF16, RESID_EPI, EMBED_CLS, 0, 7, 196, 0, 0, 0, 0, 0, 0), class_token=True, pre_ln=True),   # vit_seq 730: the projector keeps every row
    row('bf16_true_post_ln', 'bf16', 'true', 3, (BF16, RESID_EPI, EMBED_ADD_ROWS, 0, 7, 196, 0, 1, 1, 0, 0, 0), post_ln=True),             # the tower's last op reads every row; the projector does not
    row('r16_true_post_ln', 'fp16_resid16', 'true', 3, (F16, RESID_F16, EMBED_ADD_ROWS, 0, 7, 196, 0, 1, 1, 0, 0, 1), post_ln=True),
    row('bf16_true_quick_gelu_b17', 'bf16', 'true', 17, (BF16, RESID_EPI, EMBED_ADD_ROWS, 0, 7, 196, 0, 1, 1, 0, 0, 0), act=1),            # the activation is a pass of its own: row-major
    row('bf16_true_vision_only', 'bf16', 'true', 3, (BF16, RESID_EPI, EMBED_ADD_ROWS, 0, 7, 196, 0, 0, 0, 0, 0, 0), vision_only=True),
    row('bf16_true_zero_layers_b17', 'bf16', 'true', 17, (BF16, RESID_EPI, EMBED_ADD_ROWS, 0, 7, 196, 0, 1, 1, 0, 0, 0), layers=0),
    row('fp16_true_zero_layers', 'fp16', 'true', 3, (F16, RESID_F32, EMBED_F32, 0, 7, 196, 0, 1, 1, 0, 0, 0), layers=0),
    row('r16_true_zero_layers', 'fp16_resid16', 'true', 3, (F16, RESID_F16, EMBED_ADD_ROWS, 0, 7, 196, 0, 1, 1, 0, 0, 1), layers=0),       # the embed output is still converted
    row('fp32_true_full_tower', 'fp32', 'true', 3, (F32, RESID_EPI, EMBED_ADD_ROWS, 0, 7, 196, 0, 1, 1, 0, 0, 0), full_tower=True),
    # ---- the batch bound ----
    row('bf16_true_max_batch', 'bf16', 'true', 4, (BF16, RESID_EPI, EMBED_ADD_ROWS, 1, 7, 196, 784, 1, 0, 0, 0, 0), max_batch=4),
    row('bf16_true_over_max_batch', 'bf16', 'true', 5, None, max_batch=4, refusal='vit batch 5 exceeds max_vit_batch 4'),
    row('fp16_g16_over_max_batch', 'fp16', 'small16', 9, None, for_pool=False, refusal='vit batch 9 exceeds max_vit_batch 8'),
]

# tower_projector_plan(model, all_tokens) -> (compact, gather, pout): the projector without a tower run in front (mmd_connector_pool on feature files: every token is
# there, so compact means gather) and the stage-1 debug tap (all tokens)
ProjRow = namedtuple('ProjRow', 'name tower all_tokens model plan')
PROJECTOR_ROWS = [
    ProjRow('true', 'true', False, {}, (1, 1, 7)),
    ProjRow('true_tap', 'true', True, {}, (0, 0, 7)),
    ProjRow('small12', 'small12', False, {}, (1, 1, 3)),
    ProjRow('small16_tap', 'small16', True, {}, (0, 0, 4)),
    ProjRow('stride2', 'true', False, dict(pool_stride=2), (0, 0, 14)),
    ProjRow('average', 'true', False, dict(pool_mode=POOL_AVERAGE), (0, 0, 7)),
    ProjRow('class_token', 'true', False, dict(class_token=True), (0, 0, 7)),
    ProjRow('post_ln', 'true', False, dict(post_ln=True), (1, 1, 7)),
]


def rows_by_name():
    return {r.name: r for r in ROWS}
