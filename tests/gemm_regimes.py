"""The GEMM dispatch regimes of gemm_plan (mmduet_amd/csrc/gemm_plan.h), one row per shape: which kernel and which instantiation the automatic
dispatch must choose, on both sides of every threshold.  Plain data (imports without a GPU): tests/test_gemm_regime_table.py checks the table
itself, tests/test_gemm_plan_host.py asks gemm_plan about every row on the host (plan and instantiation), tests/test_gpu_gemm_regimes.py runs every
row on the device.

A row is (name, mode, width, M, max_step_tokens, plan, inst):
  * mode -- 'gemm': mmd_op_gemm, epilogue in place, variant 0 (automatic);  'slabs': mmd_op_gemm_slabs, variant 2 (the fused schedule's fp32 K
    slabs, room for SLAB_MAX_SPLITS of them);  'w8': mmd_op_gemm_w8, variant 0 (fp8-e4m3 weights with one scale per output channel).
  * width -- a key of WIDTHS: (N, K, epilogue).  Epilogues: 'bias' (none + bias), 'resid', 'swiglu' (gate / up rows interleaved in blocks of
    16), 'gelu_tanh' and 'gelu_erf' (+ bias), 'out_f32' (fp32 output, no bias: the lm_head).  Slab rows have no epilogue.
  * max_step_tokens -- the context's class of split-K workspace: 1024 -> 64 MB, 4096 (> 2048) -> 192 MB.  (Slab rows use their own buffer.)
  * plan -- what mmd_op_gemm_last_plan must report: (kernel GEMM_K_*, output tiles, K splits, blocks launched).
  * inst -- the instantiation the plan implies: MT (16-row groups) and NT (n-tiles per wave) of gemm_skinny_kernel, NT of the GEMV (two n-tiles
    per wave for SwiGLU or >= 2048 even n-tiles), MT / NT / WN (waves per block, from stream_plan's cost model) of gemm_stream_kernel.
    blocks = (NT == 2 ? tiles / 2 : tiles) * splits (GEMV), cdiv(tiles, 4 NT) * splits (skinny), cdiv(tiles, WN NT) * splits (stream).

Every plan was derived by hand from gemm_plan and what it calls: plan_kernel's branch order, plan_gemv16, plan_skinny, stream_ok / stream_plan /
stream_geometry, plan_big / big_bm160, ring_tiles_ok, ring_split_choice / plan_ring and the mid-M cost model of the 4-wave ring; the host test and the GPU
test confirm each one."""
from collections import namedtuple

# GEMM_K_* of csrc/gemm_plan.h (the host test checks the names and values against the header)
TILE64, TILE128, SKINNY, GEMV16, BIG64, BIG128, RING256, RING128X2, STREAM = range(9)
KERNEL_NAMES = {TILE64: 'TILE64', TILE128: 'TILE128', SKINNY: 'SKINNY', GEMV16: 'GEMV16', BIG64: 'BIG64', BIG128: 'BIG128', RING256: 'RING256',
                RING128X2: 'RING128X2', STREAM: 'STREAM'}

WIDTHS = {
    # the decoder (Qwen2-7B): what every LLM step and chunk multiplies
    'qkv': (4608, 3584, 'bias'), 'o': (3584, 3584, 'resid'), 'gate_up': (37888, 3584, 'swiglu'), 'down': (3584, 18944, 'resid'),
    'lm_head': (152064, 3584, 'out_f32'),
    # the vision tower and projector, where they reach a regime (or an epilogue) the decoder does not
    'vit_qkv': (3456, 1152, 'bias'), 'fc1': (4352, 1152, 'gelu_tanh'), 'fc2': (1152, 4352, 'resid'), 'vit_o': (1152, 1152, 'resid'),
    'proj0': (3584, 1152, 'gelu_erf'),
    # the K >= 8192 switch of the split-K ring, either side of it
    'k8192': (3584, 8192, 'resid'), 'k8128': (3584, 8128, 'resid'),
}
DECODER = ('qkv', 'o', 'gate_up', 'down', 'lm_head')

# M thresholds of the dispatch: gemv16 <= 16 < skinny MT 2 <= 32 < stream MT 4 (fp8: skinny MT 4) <= 64 < stream MT 8 <= 128 < stream MT 16 <= 256 <
# tile kernels; ring conditions from 512.  Each is run on both sides, at every width of SWEEPS.
THRESHOLD_MS = (1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 511, 512)
SLAB_MAX_M = 256                # mmd_op_gemm_slabs takes M <= 256
SLAB_MAX_SPLITS = 16
SWEEPS = [('gemm', w) for w in DECODER] + [('w8', w) for w in ('qkv', 'o', 'gate_up', 'down')] + [('slabs', w) for w in ('qkv', 'o', 'down')]

Row = namedtuple('Row', 'name mode width M max_step_tokens plan inst')

ROWS = [
    # ---- automatic dispatch at the decoder's widths: every threshold M ----
    Row('gemm_qkv_1', 'gemm', 'qkv', 1, 1024, (GEMV16, 288, 1, 288), dict(NT=1)),
    Row('gemm_qkv_2', 'gemm', 'qkv', 2, 1024, (GEMV16, 288, 1, 288), dict(NT=1)),
    Row('gemm_qkv_16', 'gemm', 'qkv', 16, 1024, (GEMV16, 288, 1, 288), dict(NT=1)),
    Row('gemm_qkv_17', 'gemm', 'qkv', 17, 1024, (SKINNY, 288, 7, 504), dict(MT=2, NT=1)),
    Row('gemm_qkv_32', 'gemm', 'qkv', 32, 1024, (SKINNY, 288, 7, 504), dict(MT=2, NT=1)),
    Row('gemm_qkv_33', 'gemm', 'qkv', 33, 1024, (STREAM, 288, 4, 232), dict(MT=4, NT=1, WN=5)),
    Row('gemm_qkv_64', 'gemm', 'qkv', 64, 1024, (STREAM, 288, 4, 232), dict(MT=4, NT=1, WN=5)),
    Row('gemm_qkv_65', 'gemm', 'qkv', 65, 1024, (STREAM, 288, 4, 192), dict(MT=8, NT=1, WN=6)),
    Row('gemm_qkv_128', 'gemm', 'qkv', 128, 1024, (STREAM, 288, 4, 232), dict(MT=8, NT=1, WN=5)),
    Row('gemm_qkv_129', 'gemm', 'qkv', 129, 1024, (STREAM, 288, 7, 252), dict(MT=16, NT=1, WN=8)),
    Row('gemm_qkv_256', 'gemm', 'qkv', 256, 1024, (STREAM, 288, 4, 232), dict(MT=16, NT=1, WN=5)),
    Row('gemm_qkv_257', 'gemm', 'qkv', 257, 1024, (BIG64, 216, 1, 216), {}),
    Row('gemm_qkv_511', 'gemm', 'qkv', 511, 1024, (BIG64, 288, 1, 288), {}),
    Row('gemm_qkv_512', 'gemm', 'qkv', 512, 1024, (BIG64, 288, 1, 288), {}),
    Row('gemm_o_1', 'gemm', 'o', 1, 1024, (GEMV16, 224, 1, 224), dict(NT=1)),
    Row('gemm_o_2', 'gemm', 'o', 2, 1024, (GEMV16, 224, 1, 224), dict(NT=1)),
    Row('gemm_o_16', 'gemm', 'o', 16, 1024, (GEMV16, 224, 1, 224), dict(NT=1)),
    Row('gemm_o_17', 'gemm', 'o', 17, 1024, (SKINNY, 224, 7, 392), dict(MT=2, NT=1)),
    Row('gemm_o_32', 'gemm', 'o', 32, 1024, (SKINNY, 224, 7, 392), dict(MT=2, NT=1)),
    Row('gemm_o_33', 'gemm', 'o', 33, 1024, (STREAM, 224, 4, 224), dict(MT=4, NT=1, WN=4)),
    Row('gemm_o_64', 'gemm', 'o', 64, 1024, (STREAM, 224, 4, 224), dict(MT=4, NT=1, WN=4)),
    Row('gemm_o_65', 'gemm', 'o', 65, 1024, (STREAM, 224, 4, 180), dict(MT=8, NT=1, WN=5)),
    Row('gemm_o_128', 'gemm', 'o', 128, 1024, (STREAM, 224, 4, 224), dict(MT=8, NT=1, WN=4)),
    Row('gemm_o_129', 'gemm', 'o', 129, 1024, (STREAM, 224, 8, 256), dict(MT=16, NT=1, WN=7)),
    Row('gemm_o_256', 'gemm', 'o', 256, 1024, (STREAM, 224, 8, 256), dict(MT=16, NT=1, WN=7)),
    Row('gemm_o_257', 'gemm', 'o', 257, 1024, (BIG64, 168, 1, 168), {}),
    Row('gemm_o_511', 'gemm', 'o', 511, 1024, (BIG64, 224, 1, 224), {}),
    Row('gemm_o_512', 'gemm', 'o', 512, 1024, (BIG64, 224, 1, 224), {}),
    Row('gemm_gate_up_1', 'gemm', 'gate_up', 1, 1024, (GEMV16, 2368, 1, 1184), dict(NT=2)),
    Row('gemm_gate_up_2', 'gemm', 'gate_up', 2, 1024, (GEMV16, 2368, 1, 1184), dict(NT=2)),
    Row('gemm_gate_up_16', 'gemm', 'gate_up', 16, 1024, (GEMV16, 2368, 1, 1184), dict(NT=2)),
    Row('gemm_gate_up_17', 'gemm', 'gate_up', 17, 1024, (SKINNY, 2368, 1, 296), dict(MT=2, NT=2)),
    Row('gemm_gate_up_32', 'gemm', 'gate_up', 32, 1024, (SKINNY, 2368, 1, 296), dict(MT=2, NT=2)),
    Row('gemm_gate_up_33', 'gemm', 'gate_up', 33, 1024, (STREAM, 2368, 1, 237), dict(MT=4, NT=2, WN=5)),
    Row('gemm_gate_up_64', 'gemm', 'gate_up', 64, 1024, (STREAM, 2368, 1, 237), dict(MT=4, NT=2, WN=5)),
    Row('gemm_gate_up_65', 'gemm', 'gate_up', 65, 1024, (STREAM, 2368, 1, 237), dict(MT=8, NT=2, WN=5)),
    Row('gemm_gate_up_128', 'gemm', 'gate_up', 128, 1024, (STREAM, 2368, 1, 237), dict(MT=8, NT=2, WN=5)),
    Row('gemm_gate_up_129', 'gemm', 'gate_up', 129, 1024, (STREAM, 2368, 1, 237), dict(MT=16, NT=2, WN=5)),
    Row('gemm_gate_up_256', 'gemm', 'gate_up', 256, 1024, (STREAM, 2368, 1, 237), dict(MT=16, NT=2, WN=5)),
    Row('gemm_gate_up_257', 'gemm', 'gate_up', 257, 1024, (BIG128, 888, 1, 888), {}),
    Row('gemm_gate_up_511', 'gemm', 'gate_up', 511, 1024, (BIG128, 1184, 1, 1184), {}),
    Row('gemm_gate_up_512', 'gemm', 'gate_up', 512, 1024, (BIG128, 1184, 1, 1184), {}),
    Row('gemm_gate_up_513', 'gemm', 'gate_up', 513, 1024, (RING256, 444, 1, 256), {}),
    Row('gemm_down_1', 'gemm', 'down', 1, 1024, (GEMV16, 224, 1, 224), dict(NT=1)),
    Row('gemm_down_2', 'gemm', 'down', 2, 1024, (GEMV16, 224, 1, 224), dict(NT=1)),
    Row('gemm_down_16', 'gemm', 'down', 16, 1024, (GEMV16, 224, 1, 224), dict(NT=1)),
    Row('gemm_down_17', 'gemm', 'down', 17, 1024, (SKINNY, 224, 8, 448), dict(MT=2, NT=1)),
    Row('gemm_down_32', 'gemm', 'down', 32, 1024, (SKINNY, 224, 8, 448), dict(MT=2, NT=1)),
    Row('gemm_down_33', 'gemm', 'down', 33, 1024, (STREAM, 224, 8, 256), dict(MT=4, NT=1, WN=7)),
    Row('gemm_down_64', 'gemm', 'down', 64, 1024, (STREAM, 224, 8, 256), dict(MT=4, NT=1, WN=7)),
    Row('gemm_down_65', 'gemm', 'down', 65, 1024, (STREAM, 224, 9, 252), dict(MT=8, NT=1, WN=8)),
    Row('gemm_down_128', 'gemm', 'down', 128, 1024, (STREAM, 224, 9, 252), dict(MT=8, NT=1, WN=8)),
    Row('gemm_down_129', 'gemm', 'down', 129, 1024, (STREAM, 224, 9, 252), dict(MT=16, NT=1, WN=8)),
    Row('gemm_down_256', 'gemm', 'down', 256, 1024, (STREAM, 224, 9, 252), dict(MT=16, NT=1, WN=8)),
    Row('gemm_down_257', 'gemm', 'down', 257, 1024, (BIG64, 168, 3, 504), {}),
    Row('gemm_down_511', 'gemm', 'down', 511, 1024, (BIG64, 224, 3, 672), {}),
    Row('gemm_down_512', 'gemm', 'down', 512, 1024, (RING256, 28, 9, 252), {}),
    Row('gemm_lm_head_1', 'gemm', 'lm_head', 1, 1024, (GEMV16, 9504, 1, 4752), dict(NT=2)),
    Row('gemm_lm_head_2', 'gemm', 'lm_head', 2, 1024, (GEMV16, 9504, 1, 4752), dict(NT=2)),
    Row('gemm_lm_head_16', 'gemm', 'lm_head', 16, 1024, (GEMV16, 9504, 1, 4752), dict(NT=2)),
    Row('gemm_lm_head_17', 'gemm', 'lm_head', 17, 1024, (SKINNY, 9504, 1, 1188), dict(MT=2, NT=2)),
    Row('gemm_lm_head_32', 'gemm', 'lm_head', 32, 1024, (SKINNY, 9504, 1, 1188), dict(MT=2, NT=2)),
    Row('gemm_lm_head_33', 'gemm', 'lm_head', 33, 1024, (SKINNY, 9504, 1, 1188), dict(MT=4, NT=2)),
    Row('gemm_lm_head_64', 'gemm', 'lm_head', 64, 1024, (SKINNY, 9504, 1, 1188), dict(MT=4, NT=2)),
    Row('gemm_lm_head_65', 'gemm', 'lm_head', 65, 1024, (TILE64, 4752, 1, 4752), {}),
    Row('gemm_lm_head_128', 'gemm', 'lm_head', 128, 1024, (TILE64, 4752, 1, 4752), {}),
    Row('gemm_lm_head_129', 'gemm', 'lm_head', 129, 1024, (TILE64, 7128, 1, 7128), {}),
    Row('gemm_lm_head_256', 'gemm', 'lm_head', 256, 1024, (TILE128, 2376, 1, 2376), {}),
    Row('gemm_lm_head_257', 'gemm', 'lm_head', 257, 1024, (TILE128, 3564, 1, 3564), {}),
    Row('gemm_lm_head_511', 'gemm', 'lm_head', 511, 1024, (TILE128, 4752, 1, 4752), {}),
    Row('gemm_lm_head_512', 'gemm', 'lm_head', 512, 1024, (TILE128, 4752, 1, 4752), {}),
    Row('gemm_lm_head_255', 'gemm', 'lm_head', 255, 1024, (TILE64, 9504, 1, 9504), {}),
    # ---- ring and cost-model edges above 512 rows ----
    Row('gemm_qkv_1280', 'gemm', 'qkv', 1280, 1024, (BIG64, 720, 1, 720), {}),
    Row('gemm_qkv_1281', 'gemm', 'qkv', 1281, 1024, (RING128X2, 216, 1, 216), {}),
    Row('gemm_qkv_1408', 'gemm', 'qkv', 1408, 1024, (RING128X2, 216, 1, 216), {}),
    Row('gemm_qkv_1409', 'gemm', 'qkv', 1409, 1024, (BIG128, 432, 1, 432), {}),
    Row('gemm_qkv_3072', 'gemm', 'qkv', 3072, 1024, (BIG128, 864, 1, 864), {}),
    Row('gemm_qkv_3073', 'gemm', 'qkv', 3073, 1024, (RING256, 234, 1, 234), {}),
    Row('gemm_o_1280', 'gemm', 'o', 1280, 1024, (BIG64, 448, 1, 448), {}),
    Row('gemm_o_1664', 'gemm', 'o', 1664, 1024, (BIG64, 728, 1, 728), {}),
    Row('gemm_o_1665', 'gemm', 'o', 1665, 1024, (RING128X2, 196, 1, 196), {}),
    Row('gemm_down_2304', 'gemm', 'down', 2304, 1024, (RING256, 126, 2, 252), {}),
    Row('gemm_down_2305', 'gemm', 'down', 2305, 1024, (BIG128, 532, 1, 532), {}),
    Row('gemm_vit_o_11776', 'gemm', 'vit_o', 11776, 1024, (BIG128, 828, 1, 828), {}),
    Row('gemm_vit_o_11777', 'gemm', 'vit_o', 11777, 1024, (RING256, 235, 1, 235), {}),
    Row('gemm_vit_o_20224', 'gemm', 'vit_o', 20224, 1024, (BIG128, 1422, 1, 1422), {}),
    Row('gemm_vit_o_20225', 'gemm', 'vit_o', 20225, 1024, (RING256, 400, 1, 256), {}),
    Row('gemm_down_2305_ws4096', 'gemm', 'down', 2305, 4096, (RING256, 140, 3, 420), {}),
    # ---- tower / projector widths: epilogues and split branches the decoder does not reach; the K >= 8192 switch; the 192 MB workspace ----
    Row('gemm_fc1_33', 'gemm', 'fc1', 33, 1024, (STREAM, 272, 1, 68), dict(MT=4, NT=1, WN=4)),
    Row('gemm_fc1_257', 'gemm', 'fc1', 257, 1024, (BIG64, 204, 1, 204), {}),
    Row('gemm_fc2_33', 'gemm', 'fc2', 33, 1024, (STREAM, 72, 5, 90), dict(MT=4, NT=1, WN=4)),
    Row('gemm_fc2_257', 'gemm', 'fc2', 257, 1024, (BIG64, 54, 4, 216), {}),
    Row('gemm_proj0_129', 'gemm', 'proj0', 129, 1024, (STREAM, 224, 3, 168), dict(MT=16, NT=1, WN=4)),
    Row('gemm_proj0_257', 'gemm', 'proj0', 257, 1024, (BIG64, 168, 1, 168), {}),
    Row('gemm_vit_qkv_129', 'gemm', 'vit_qkv', 129, 1024, (STREAM, 216, 3, 162), dict(MT=16, NT=1, WN=4)),
    Row('gemm_k8192_512', 'gemm', 'k8192', 512, 1024, (RING256, 28, 8, 224), {}),
    Row('gemm_k8128_512', 'gemm', 'k8128', 512, 1024, (BIG64, 224, 1, 224), {}),
    Row('gemm_down_512_ws4096', 'gemm', 'down', 512, 4096, (RING256, 28, 9, 252), {}),
    # ---- fp8 weights: gemv16-W8, skinny-W8 (MT 2 and 4: the streaming kernel starts at 65 rows here), then stream / tile / ring kernels on bf16(q) ----
    Row('w8_qkv_1', 'w8', 'qkv', 1, 1024, (GEMV16, 288, 1, 288), dict(NT=1)),
    Row('w8_qkv_2', 'w8', 'qkv', 2, 1024, (GEMV16, 288, 1, 288), dict(NT=1)),
    Row('w8_qkv_16', 'w8', 'qkv', 16, 1024, (GEMV16, 288, 1, 288), dict(NT=1)),
    Row('w8_qkv_17', 'w8', 'qkv', 17, 1024, (SKINNY, 288, 7, 504), dict(MT=2, NT=1)),
    Row('w8_qkv_32', 'w8', 'qkv', 32, 1024, (SKINNY, 288, 7, 504), dict(MT=2, NT=1)),
    Row('w8_qkv_33', 'w8', 'qkv', 33, 1024, (SKINNY, 288, 7, 504), dict(MT=4, NT=1)),
    Row('w8_qkv_64', 'w8', 'qkv', 64, 1024, (SKINNY, 288, 7, 504), dict(MT=4, NT=1)),
    Row('w8_qkv_65', 'w8', 'qkv', 65, 1024, (STREAM, 288, 4, 192), dict(MT=8, NT=1, WN=6)),
    Row('w8_qkv_128', 'w8', 'qkv', 128, 1024, (STREAM, 288, 4, 232), dict(MT=8, NT=1, WN=5)),
    Row('w8_qkv_129', 'w8', 'qkv', 129, 1024, (STREAM, 288, 7, 252), dict(MT=16, NT=1, WN=8)),
    Row('w8_qkv_256', 'w8', 'qkv', 256, 1024, (STREAM, 288, 4, 232), dict(MT=16, NT=1, WN=5)),
    Row('w8_qkv_257', 'w8', 'qkv', 257, 1024, (BIG64, 216, 1, 216), {}),
    Row('w8_qkv_511', 'w8', 'qkv', 511, 1024, (BIG64, 288, 1, 288), {}),
    Row('w8_qkv_512', 'w8', 'qkv', 512, 1024, (BIG64, 288, 1, 288), {}),
    Row('w8_o_1', 'w8', 'o', 1, 1024, (GEMV16, 224, 1, 224), dict(NT=1)),
    Row('w8_o_2', 'w8', 'o', 2, 1024, (GEMV16, 224, 1, 224), dict(NT=1)),
    Row('w8_o_16', 'w8', 'o', 16, 1024, (GEMV16, 224, 1, 224), dict(NT=1)),
    Row('w8_o_17', 'w8', 'o', 17, 1024, (SKINNY, 224, 7, 392), dict(MT=2, NT=1)),
    Row('w8_o_32', 'w8', 'o', 32, 1024, (SKINNY, 224, 7, 392), dict(MT=2, NT=1)),
    Row('w8_o_33', 'w8', 'o', 33, 1024, (SKINNY, 224, 7, 392), dict(MT=4, NT=1)),
    Row('w8_o_64', 'w8', 'o', 64, 1024, (SKINNY, 224, 7, 392), dict(MT=4, NT=1)),
    Row('w8_o_65', 'w8', 'o', 65, 1024, (STREAM, 224, 4, 180), dict(MT=8, NT=1, WN=5)),
    Row('w8_o_128', 'w8', 'o', 128, 1024, (STREAM, 224, 4, 224), dict(MT=8, NT=1, WN=4)),
    Row('w8_o_129', 'w8', 'o', 129, 1024, (STREAM, 224, 8, 256), dict(MT=16, NT=1, WN=7)),
    Row('w8_o_256', 'w8', 'o', 256, 1024, (STREAM, 224, 8, 256), dict(MT=16, NT=1, WN=7)),
    Row('w8_o_257', 'w8', 'o', 257, 1024, (BIG64, 168, 1, 168), {}),
    Row('w8_o_511', 'w8', 'o', 511, 1024, (BIG64, 224, 1, 224), {}),
    Row('w8_o_512', 'w8', 'o', 512, 1024, (BIG64, 224, 1, 224), {}),
    Row('w8_gate_up_1', 'w8', 'gate_up', 1, 1024, (GEMV16, 2368, 1, 1184), dict(NT=2)),
    Row('w8_gate_up_2', 'w8', 'gate_up', 2, 1024, (GEMV16, 2368, 1, 1184), dict(NT=2)),
    Row('w8_gate_up_16', 'w8', 'gate_up', 16, 1024, (GEMV16, 2368, 1, 1184), dict(NT=2)),
    Row('w8_gate_up_17', 'w8', 'gate_up', 17, 1024, (SKINNY, 2368, 1, 296), dict(MT=2, NT=2)),
    Row('w8_gate_up_32', 'w8', 'gate_up', 32, 1024, (SKINNY, 2368, 1, 296), dict(MT=2, NT=2)),
    Row('w8_gate_up_33', 'w8', 'gate_up', 33, 1024, (SKINNY, 2368, 1, 296), dict(MT=4, NT=2)),
    Row('w8_gate_up_64', 'w8', 'gate_up', 64, 1024, (SKINNY, 2368, 1, 296), dict(MT=4, NT=2)),
    Row('w8_gate_up_65', 'w8', 'gate_up', 65, 1024, (STREAM, 2368, 1, 237), dict(MT=8, NT=2, WN=5)),
    Row('w8_gate_up_128', 'w8', 'gate_up', 128, 1024, (STREAM, 2368, 1, 237), dict(MT=8, NT=2, WN=5)),
    Row('w8_gate_up_129', 'w8', 'gate_up', 129, 1024, (STREAM, 2368, 1, 237), dict(MT=16, NT=2, WN=5)),
    Row('w8_gate_up_256', 'w8', 'gate_up', 256, 1024, (STREAM, 2368, 1, 237), dict(MT=16, NT=2, WN=5)),
    Row('w8_gate_up_257', 'w8', 'gate_up', 257, 1024, (BIG128, 888, 1, 888), {}),
    Row('w8_gate_up_511', 'w8', 'gate_up', 511, 1024, (BIG128, 1184, 1, 1184), {}),
    Row('w8_gate_up_512', 'w8', 'gate_up', 512, 1024, (BIG128, 1184, 1, 1184), {}),
    Row('w8_down_1', 'w8', 'down', 1, 1024, (GEMV16, 224, 1, 224), dict(NT=1)),
    Row('w8_down_2', 'w8', 'down', 2, 1024, (GEMV16, 224, 1, 224), dict(NT=1)),
    Row('w8_down_16', 'w8', 'down', 16, 1024, (GEMV16, 224, 1, 224), dict(NT=1)),
    Row('w8_down_17', 'w8', 'down', 17, 1024, (SKINNY, 224, 8, 448), dict(MT=2, NT=1)),
    Row('w8_down_32', 'w8', 'down', 32, 1024, (SKINNY, 224, 8, 448), dict(MT=2, NT=1)),
    Row('w8_down_33', 'w8', 'down', 33, 1024, (SKINNY, 224, 8, 448), dict(MT=4, NT=1)),
    Row('w8_down_64', 'w8', 'down', 64, 1024, (SKINNY, 224, 8, 448), dict(MT=4, NT=1)),
    Row('w8_down_65', 'w8', 'down', 65, 1024, (STREAM, 224, 9, 252), dict(MT=8, NT=1, WN=8)),
    Row('w8_down_128', 'w8', 'down', 128, 1024, (STREAM, 224, 9, 252), dict(MT=8, NT=1, WN=8)),
    Row('w8_down_129', 'w8', 'down', 129, 1024, (STREAM, 224, 9, 252), dict(MT=16, NT=1, WN=8)),
    Row('w8_down_256', 'w8', 'down', 256, 1024, (STREAM, 224, 9, 252), dict(MT=16, NT=1, WN=8)),
    Row('w8_down_257', 'w8', 'down', 257, 1024, (BIG64, 168, 3, 504), {}),
    Row('w8_down_511', 'w8', 'down', 511, 1024, (BIG64, 224, 3, 672), {}),
    Row('w8_down_512', 'w8', 'down', 512, 1024, (RING256, 28, 9, 252), {}),
    Row('w8_gate_up_513', 'w8', 'gate_up', 513, 1024, (RING256, 444, 1, 256), {}),
    Row('w8_qkv_1281', 'w8', 'qkv', 1281, 1024, (RING128X2, 216, 1, 216), {}),
    # ---- slab mode (variant 2): the fused schedule's qkv / o / down K slabs ----
    Row('slabs_qkv_1', 'slabs', 'qkv', 1, 1024, (GEMV16, 288, 2, 576), dict(NT=1)),
    Row('slabs_qkv_2', 'slabs', 'qkv', 2, 1024, (GEMV16, 288, 2, 576), dict(NT=1)),
    Row('slabs_qkv_16', 'slabs', 'qkv', 16, 1024, (GEMV16, 288, 2, 576), dict(NT=1)),
    Row('slabs_qkv_17', 'slabs', 'qkv', 17, 1024, (SKINNY, 288, 7, 504), dict(MT=2, NT=1)),
    Row('slabs_qkv_32', 'slabs', 'qkv', 32, 1024, (SKINNY, 288, 7, 504), dict(MT=2, NT=1)),
    Row('slabs_qkv_33', 'slabs', 'qkv', 33, 1024, (STREAM, 288, 4, 232), dict(MT=4, NT=1, WN=5)),
    Row('slabs_qkv_64', 'slabs', 'qkv', 64, 1024, (STREAM, 288, 4, 232), dict(MT=4, NT=1, WN=5)),
    Row('slabs_qkv_65', 'slabs', 'qkv', 65, 1024, (STREAM, 288, 4, 192), dict(MT=8, NT=1, WN=6)),
    Row('slabs_qkv_128', 'slabs', 'qkv', 128, 1024, (STREAM, 288, 4, 232), dict(MT=8, NT=1, WN=5)),
    Row('slabs_qkv_129', 'slabs', 'qkv', 129, 1024, (STREAM, 288, 7, 252), dict(MT=16, NT=1, WN=8)),
    Row('slabs_qkv_256', 'slabs', 'qkv', 256, 1024, (STREAM, 288, 4, 232), dict(MT=16, NT=1, WN=5)),
    Row('slabs_o_1', 'slabs', 'o', 1, 1024, (GEMV16, 224, 2, 448), dict(NT=1)),
    Row('slabs_o_2', 'slabs', 'o', 2, 1024, (GEMV16, 224, 2, 448), dict(NT=1)),
    Row('slabs_o_16', 'slabs', 'o', 16, 1024, (GEMV16, 224, 2, 448), dict(NT=1)),
    Row('slabs_o_17', 'slabs', 'o', 17, 1024, (SKINNY, 224, 7, 392), dict(MT=2, NT=1)),
    Row('slabs_o_32', 'slabs', 'o', 32, 1024, (SKINNY, 224, 7, 392), dict(MT=2, NT=1)),
    Row('slabs_o_33', 'slabs', 'o', 33, 1024, (STREAM, 224, 4, 224), dict(MT=4, NT=1, WN=4)),
    Row('slabs_o_64', 'slabs', 'o', 64, 1024, (STREAM, 224, 4, 224), dict(MT=4, NT=1, WN=4)),
    Row('slabs_o_65', 'slabs', 'o', 65, 1024, (STREAM, 224, 4, 180), dict(MT=8, NT=1, WN=5)),
    Row('slabs_o_128', 'slabs', 'o', 128, 1024, (STREAM, 224, 4, 224), dict(MT=8, NT=1, WN=4)),
    Row('slabs_o_129', 'slabs', 'o', 129, 1024, (STREAM, 224, 8, 256), dict(MT=16, NT=1, WN=7)),
    Row('slabs_o_256', 'slabs', 'o', 256, 1024, (STREAM, 224, 8, 256), dict(MT=16, NT=1, WN=7)),
    Row('slabs_down_1', 'slabs', 'down', 1, 1024, (GEMV16, 224, 4, 896), dict(NT=1)),
    Row('slabs_down_2', 'slabs', 'down', 2, 1024, (GEMV16, 224, 4, 896), dict(NT=1)),
    Row('slabs_down_16', 'slabs', 'down', 16, 1024, (GEMV16, 224, 4, 896), dict(NT=1)),
    Row('slabs_down_17', 'slabs', 'down', 17, 1024, (SKINNY, 224, 8, 448), dict(MT=2, NT=1)),
    Row('slabs_down_32', 'slabs', 'down', 32, 1024, (SKINNY, 224, 8, 448), dict(MT=2, NT=1)),
    Row('slabs_down_33', 'slabs', 'down', 33, 1024, (STREAM, 224, 8, 256), dict(MT=4, NT=1, WN=7)),
    Row('slabs_down_64', 'slabs', 'down', 64, 1024, (STREAM, 224, 8, 256), dict(MT=4, NT=1, WN=7)),
    Row('slabs_down_65', 'slabs', 'down', 65, 1024, (STREAM, 224, 9, 252), dict(MT=8, NT=1, WN=8)),
    Row('slabs_down_128', 'slabs', 'down', 128, 1024, (STREAM, 224, 9, 252), dict(MT=8, NT=1, WN=8)),
    Row('slabs_down_129', 'slabs', 'down', 129, 1024, (STREAM, 224, 9, 252), dict(MT=16, NT=1, WN=8)),
    Row('slabs_down_256', 'slabs', 'down', 256, 1024, (STREAM, 224, 9, 252), dict(MT=16, NT=1, WN=8)),
]

EDGES = [  # (what switches, row below, row above): both rows exist and their plans differ
    ('gemv16 -> skinny MT 2, K split', 'gemm_qkv_16', 'gemm_qkv_17'),
    ('lm_head: gemv16 (two tiles per wave) -> skinny NT 2', 'gemm_lm_head_16', 'gemm_lm_head_17'),
    ('skinny MT 2 -> stream MT 4', 'gemm_down_32', 'gemm_down_33'),
    ('lm_head: skinny MT 2 -> MT 4', 'gemm_lm_head_32', 'gemm_lm_head_33'),
    ('lm_head: skinny -> generic 64-row tiles (out_f32 excludes stream / big)', 'gemm_lm_head_64', 'gemm_lm_head_65'),
    ('lm_head: 64-row -> 128-row generic tiles', 'gemm_lm_head_255', 'gemm_lm_head_256'),
    ('fp8: skinny-W8 MT 4 -> stream on bf16(q)', 'w8_qkv_64', 'w8_qkv_65'),
    ('fp8: skinny-W8 MT 2 -> MT 4', 'w8_o_32', 'w8_o_33'),
    ('stream MT 8 -> MT 16', 'gemm_qkv_128', 'gemm_qkv_129'),
    ('stream -> 64-wide big tiles', 'gemm_o_256', 'gemm_o_257'),
    ('stream (SwiGLU) -> 128-wide big tiles', 'gemm_gate_up_256', 'gemm_gate_up_257'),
    ('big tiles with a 3-way K split -> split-K ring (K >= 8192, M >= 512)', 'gemm_down_511', 'gemm_down_512'),
    ('the split-K ring needs K >= 8192', 'gemm_k8128_512', 'gemm_k8192_512'),
    ('gate_up: 296 -> 444 ring tiles (>= 400)', 'gemm_gate_up_512', 'gemm_gate_up_513'),
    ('mid-M cost model: big64 -> 4-wave ring', 'gemm_qkv_1280', 'gemm_qkv_1281'),
    ('mid-M cost model: 4-wave ring -> big128 (t128 >= 400)', 'gemm_qkv_1408', 'gemm_qkv_1409'),
    ('mid-M cost model at the o width', 'gemm_o_1664', 'gemm_o_1665'),
    ('ring tile fill: 216 tiles (0.84 of a wave) -> 234 (0.91)', 'gemm_qkv_3072', 'gemm_qkv_3073'),
    ('ring tile fill: 230 tiles (0.898) -> 235 (0.918)', 'gemm_vit_o_11776', 'gemm_vit_o_11777'),
    ('ring tiles: 395 -> 400', 'gemm_vit_o_20224', 'gemm_vit_o_20225'),
    ('split ring: t256 <= 128 (2 splits) -> the cost model, no split in 64 MB', 'gemm_down_2304', 'gemm_down_2305'),
    ('workspace class: 64 MB -> 192 MB (3-way split ring)', 'gemm_down_2305', 'gemm_down_2305_ws4096'),
]

COVERAGE = {  # rows kept for what they reach besides the thresholds and edges above
    'gemm_o_1280': 'big64 in its 160-row form (448 tiles)',
    'gemm_fc1_33': 'GELU(tanh) through the stream kernel + split-K reduce',
    'gemm_fc1_257': 'GELU(tanh) in the big-tile epilogue',
    'gemm_proj0_129': 'GELU(erf) through the stream kernel MT 16 + split-K reduce',
    'gemm_proj0_257': 'GELU(erf) in the big-tile epilogue',
    'gemm_fc2_33': 'stream kernel with 5 K splits at N = 1152',
    'gemm_fc2_257': 'big64 with the short-K split (tiles < 128, K >= 2048)',
    'gemm_vit_qkv_129': 'stream kernel MT 16 at K = 1152',
    'gemm_down_512_ws4096': 'split-K ring, 9 splits in the 192 MB workspace too',
    'w8_gate_up_513': 'fp8 scale in the 8-wave ring SwiGLU epilogue',
    'w8_qkv_1281': 'fp8 scale in the 4-wave ring epilogue',
}


def rows_by_name():
    return {r.name: r for r in ROWS}


def shape(row):
    """-> (N, K, epilogue) of a row; slab rows have no epilogue"""
    N, K, epi = WIDTHS[row.width]
    return N, K, ('slab' if row.mode == 'slabs' else epi)
