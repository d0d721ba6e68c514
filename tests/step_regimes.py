"""The launch schedules of an LLM step (step_plan of mmduet_amd/csrc/step_plan.h), one row per step: which plan it must take, on both sides of every threshold
and with every A/B switch at a shape where it acts.  Plain data (imports without a GPU): tests/test_step_plan_host.py asks step_plan about every row on the host,
tests/test_gpu_step_regimes.py runs the rows a bf16 context reaches eagerly on the device, the switch rows in a context created under their environment, and
compares `step_last_plan()`.

A row is (name, segs, need, hidden_out, dyn, env, model, plan):
  * segs -- rows of each stream's segment, in order; S is their sum.
  * need -- rows the caller reads (frame_step's head rows; in a step of several streams: the last row of every stream, so need == len(segs)).  More than 64 read
    rows reach the step as no list at all (build_need_list); either way the plan is the same.
  * hidden_out -- the caller wants every row's final hidden state (forward()); never together with `need`.
  * dyn -- the step is being captured into the decode graph (host rows only).
  * env -- the A/B switches set when the context is created.
  * model -- a key of MODELS: the decoder's true widths in bf16 (the one the device test builds, with a 64 MB split-K workspace), the same in fp32, with
    fp8 weights, and with head_dim 72 (no (cos, sin) table kernels, o_proj's K = 2016 is no whole number of gemm_stream_kernel steps).
  * plan -- what mmd_op_step_last_plan must report: (schedule, rope_fused, chunk_rope, sparse_last, run0, run_n, run_all, down_slab_norm, mlp_pm).

Every plan was derived by hand from the conditions llm_step_segs evaluated before step_plan existed (fused / chain / rope_fused / chunk_rope / sparse_last, the search
for the batched attention's run, `rs > 1` behind down_proj and gemm_pair_pm) and from the GEMM regime table (tests/gemm_regimes.py) for what each GEMM kernel takes:
slabs up to 256 rows; down_proj at 65..256 rows on gemm_stream_kernel (epilogue in place, no slabs for the caller), at 257..511 on the 128-row kernel with a 3-way
split, from 512 on the split-K ring; gate_up on the plain ring from 513 rows.  A run of that older code with its decisions logged confirmed the device rows.
(rope_fused also asks that the qkv GEMM leave at most four slabs: the GEMV's split count is clamped to 1..4, so no row can reach the other side of that bound.)"""
from collections import namedtuple

TILE, FUSED, CHAIN = 0, 1, 2
FIELDS = ('schedule', 'rope_fused', 'chunk_rope', 'sparse_last', 'run0', 'run_n', 'run_all', 'down_slab_norm', 'mlp_pm')
SWITCHES = ('MMDUET_NO_FUSE', 'MMDUET_NO_CHAIN', 'MMDUET_NO_SLAB_NORM', 'MMDUET_FULL_LAST_LAYER', 'MMDUET_NO_ROPE_FUSE', 'MMDUET_NO_MULTI_FUSE', 'MMDUET_NO_MULTI_ATTN',
            'MMDUET_NO_CHUNK_ROPE')

MODELS = {
    'bf16': dict(dtype='bf16', H=3584, I=18944, nh=28, nkv=4, d=128, fp8=False),
    'fp32': dict(dtype='fp32', H=3584, I=18944, nh=28, nkv=4, d=128, fp8=False),
    'fp8': dict(dtype='bf16', H=3584, I=18944, nh=28, nkv=4, d=128, fp8=True),
    'd72': dict(dtype='bf16', H=3584, I=18944, nh=28, nkv=4, d=72, fp8=False),
}
MAX_STEP_TOKENS = 768           # of the device test's context: a 64 MB split-K workspace

Row = namedtuple('Row', 'name segs need hidden_out dyn env model plan')


def row(name, segs, plan, need=0, hidden_out=False, dyn=False, env=None, model='bf16'):
    segs = (segs,) if isinstance(segs, int) else tuple(segs)
    return Row(name, segs, need, hidden_out, dyn, dict(env or {}), model, tuple(plan))


ROWS = [
    # ---- one stream, forward(): every row's hidden state wanted ----
    row('fwd_1', 1, (CHAIN, 1, 0, 0, 0, 0, 0, 0, 0), hidden_out=True),
    row('fwd_4', 4, (CHAIN, 1, 0, 0, 0, 0, 0, 0, 0), hidden_out=True),             # decode chain: S = 4 | 5
    row('fwd_5', 5, (FUSED, 0, 0, 0, 0, 0, 0, 0, 0), hidden_out=True),
    row('fwd_63', 63, (FUSED, 0, 0, 0, 0, 0, 0, 0, 0), hidden_out=True),           # (one stream is fused up to 256 rows: no chunk RoPE, no sparse last layer at 63 .. 65)
    row('fwd_64', 64, (FUSED, 0, 0, 0, 0, 0, 0, 0, 0), hidden_out=True),
    row('fwd_256', 256, (FUSED, 0, 0, 0, 0, 0, 0, 0, 0), hidden_out=True),         # fused slabs: S = 256 | 257
    row('fwd_257', 257, (TILE, 0, 1, 0, 0, 0, 0, 1, 0), hidden_out=True),
    row('fwd_300', 300, (TILE, 0, 1, 0, 0, 0, 0, 1, 0), hidden_out=True),          # hidden_out: with | without (frame_300_need_64)
    # ---- one stream, frame_step(): the head rows' hidden states wanted ----
    row('frame_49', 49, (FUSED, 0, 0, 0, 0, 0, 0, 0, 0), need=1),
    row('frame_65', 65, (FUSED, 0, 0, 0, 0, 0, 0, 0, 0), need=1),
    row('frame_256', 256, (FUSED, 0, 0, 0, 0, 0, 0, 0, 0), need=6),
    row('frame_257', 257, (TILE, 0, 1, 1, 0, 0, 0, 1, 0), need=1),
    row('frame_300_need_0', 300, (TILE, 0, 1, 0, 0, 0, 0, 1, 0), need=0),
    row('frame_300_need_64', 300, (TILE, 0, 1, 1, 0, 0, 0, 1, 0), need=64),        # need list: 64 | 65 rows
    row('frame_300_need_65', 300, (TILE, 0, 1, 0, 0, 0, 0, 1, 0), need=65),
    row('frame_511', 511, (TILE, 0, 1, 1, 0, 0, 0, 1, 0), need=1),                 # down_proj: 128-row kernel, 3-way split | split-K ring; gate_up on the plain ring from 513
    row('frame_512', 512, (TILE, 0, 1, 1, 0, 0, 0, 1, 0), need=1),
    row('frame_513', 513, (TILE, 0, 1, 1, 0, 0, 0, 1, 1), need=1),
    row('frame_700', 700, (TILE, 0, 1, 1, 0, 0, 0, 1, 1), need=10),
    # ---- several streams in one step ----
    row('talk_1x2', (1, 1), (CHAIN, 1, 0, 0, 0, 2, 1, 0, 0), need=2),              # a round of two talkers
    row('talk_2x2', (2, 2), (CHAIN, 1, 0, 0, 0, 2, 1, 0, 0), need=2),              # rows per stream x 7 query heads per kv head: 14 | 21 of 16
    row('talk_3x2', (3, 3), (FUSED, 0, 0, 0, 0, 0, 0, 0, 0), need=2),
    row('talk_1x16', (1,) * 16, (FUSED, 1, 0, 0, 0, 16, 1, 0, 0), need=16),        # rope_fused on all-talking rounds: S = 16 | 17
    row('talk_1x17', (1,) * 17, (FUSED, 0, 0, 0, 0, 17, 1, 0, 0), need=17),
    row('talk_1x64', (1,) * 64, (FUSED, 0, 0, 0, 0, 64, 1, 0, 0), need=64),        # run length: 64 | 65
    row('talk_1x65', (1,) * 65, (FUSED, 0, 0, 0, 0, 0, 0, 0, 0), need=65),
    row('chunk_talk_1', (49, 1), (FUSED, 0, 0, 0, 0, 0, 0, 0, 0), need=2),         # run length: 1 | 2, behind a watching stream's chunk
    row('chunk_talk_2', (49, 1, 1), (FUSED, 0, 0, 0, 1, 2, 0, 0, 0), need=3),
    row('longest_run', (1, 1, 2, 2, 2), (FUSED, 0, 0, 0, 2, 3, 0, 0, 0), need=5),
    row('big_chunk_talk_2', (300, 1, 1), (TILE, 0, 1, 1, 1, 2, 0, 1, 0), need=3),
    # ---- other contexts (host only) ----
    row('fp32_1', 1, (TILE, 0, 0, 0, 0, 0, 0, 0, 0), hidden_out=True, model='fp32'),
    row('fp32_700', 700, (TILE, 0, 0, 0, 0, 0, 0, 0, 0), need=10, model='fp32'),
    row('fp32_talk_1x2', (1, 1), (TILE, 0, 0, 0, 0, 0, 0, 0, 0), need=2, model='fp32'),
    row('d72_1', 1, (CHAIN, 0, 0, 0, 0, 0, 0, 0, 0), hidden_out=True, model='d72'),
    row('d72_100', 100, (TILE, 0, 0, 1, 0, 0, 0, 0, 0), need=1, model='d72'),      # o_proj's K = 2016: no slab kernel above 64 rows (the one read row has one); down_proj on gemm_stream_kernel
    row('d72_700', 700, (TILE, 0, 0, 1, 0, 0, 0, 1, 1), need=10, model='d72'),
    row('d72_talk_1x2', (1, 1), (CHAIN, 0, 0, 0, 0, 0, 0, 0, 0), need=2, model='d72'),
    row('fp8_1', 1, (CHAIN, 1, 0, 0, 0, 0, 0, 0, 0), hidden_out=True, model='fp8'),
    row('fp8_700', 700, (TILE, 0, 1, 1, 0, 0, 0, 1, 0), need=10, model='fp8'),     # no piece-major form with a weight scale
    row('graph_1', 1, (CHAIN, 1, 0, 0, 0, 0, 0, 0, 0), dyn=True),
    # ---- each switch at a shape where it acts (a fresh context per environment) ----
    row('no_fuse_1', 1, (TILE, 0, 0, 0, 0, 0, 0, 0, 0), hidden_out=True, env={'MMDUET_NO_FUSE': '1'}),
    row('no_fuse_700', 700, (TILE, 0, 0, 0, 0, 0, 0, 0, 0), need=10, env={'MMDUET_NO_FUSE': '1'}),
    row('no_fuse_talk_1x2', (1, 1), (TILE, 0, 0, 0, 0, 0, 0, 0, 0), need=2, env={'MMDUET_NO_FUSE': '1'}),
    row('no_fuse2_700', 700, (TILE, 0, 1, 1, 0, 0, 0, 1, 0), need=10, env={'MMDUET_NO_FUSE': '2'}),
    row('no_fuse0_1', 1, (CHAIN, 1, 0, 0, 0, 0, 0, 0, 0), hidden_out=True, env={'MMDUET_NO_FUSE': '0'}),
    row('no_chain_1', 1, (FUSED, 0, 0, 0, 0, 0, 0, 0, 0), hidden_out=True, env={'MMDUET_NO_CHAIN': '1'}),
    row('no_slab_norm_700', 700, (TILE, 0, 1, 1, 0, 0, 0, 0, 1), need=10, env={'MMDUET_NO_SLAB_NORM': '1'}),
    row('full_last_layer_700', 700, (TILE, 0, 1, 0, 0, 0, 0, 1, 1), need=10, env={'MMDUET_FULL_LAST_LAYER': '1'}),
    row('no_rope_fuse_1', 1, (CHAIN, 0, 0, 0, 0, 0, 0, 0, 0), hidden_out=True, env={'MMDUET_NO_ROPE_FUSE': '1'}),
    row('no_rope_fuse_talk_1x16', (1,) * 16, (FUSED, 0, 0, 0, 0, 16, 1, 0, 0), need=16, env={'MMDUET_NO_ROPE_FUSE': '1'}),
    row('no_multi_fuse_talk_1x2', (1, 1), (TILE, 0, 0, 0, 0, 2, 1, 0, 0), need=2, env={'MMDUET_NO_MULTI_FUSE': '1'}),
    row('no_multi_fuse_1', 1, (CHAIN, 1, 0, 0, 0, 0, 0, 0, 0), hidden_out=True, env={'MMDUET_NO_MULTI_FUSE': '1'}),
    row('no_multi_fuse_63', (32, 31), (TILE, 0, 0, 0, 0, 0, 0, 0, 0), need=2, env={'MMDUET_NO_MULTI_FUSE': '1'}),      # chunk_rope: S = 63 | 64 (a tile schedule this short: several streams, unfused)
    row('no_multi_fuse_64', (32, 32), (TILE, 0, 1, 0, 0, 0, 0, 0, 0), need=2, env={'MMDUET_NO_MULTI_FUSE': '1'}),      # sparse_last: S = 64 | 65
    row('no_multi_fuse_65', (33, 32), (TILE, 0, 1, 1, 0, 0, 0, 0, 0), need=2, env={'MMDUET_NO_MULTI_FUSE': '1'}),
    row('no_multi_attn_talk_1x2', (1, 1), (CHAIN, 1, 0, 0, 0, 0, 0, 0, 0), need=2, env={'MMDUET_NO_MULTI_ATTN': '1'}),
    row('no_multi_attn_talk_1x16', (1,) * 16, (FUSED, 0, 0, 0, 0, 0, 0, 0, 0), need=16, env={'MMDUET_NO_MULTI_ATTN': '1'}),
    row('no_chunk_rope_700', 700, (TILE, 0, 0, 1, 0, 0, 0, 1, 1), need=10, env={'MMDUET_NO_CHUNK_ROPE': '1'}),
]


def rows_by_name():
    return {r.name: r for r in ROWS}


def gpu_rows():
    """the rows a bf16 context takes eagerly on the device: a fresh context per environment, since the switches are read when a context is created"""
    return [r for r in ROWS if r.model == 'bf16' and not r.dyn]
