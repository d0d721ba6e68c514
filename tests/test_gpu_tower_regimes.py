"""The tower regime table (tests/tower_regimes.py) on the device: the rows a context reaches are run, and `tower_last_plan()` -- the plan the tower launched from -- must
equal the table's; after each run the debug tap refuses exactly when the plan says sparse_last.  (tests/test_tower_plan_host.py checks every row against tower_plan() on
the host.)

  * the 64-wide tower of test_fp16_tower_small_grids_fall_back_to_the_full_last_layer at grids 12 and 16, bf16 and fp16 tower, B = 1 / 2 / 3: the sparse / full gate.  Where
    the gate keeps the full last layer, the default encode and the set_full_tower(True) one ran the same schedule: torch.equal, as that test establishes;
  * one true-width build (C = 1152, 2 tower layers) per tower mode, built for 17 frames so that B = 16 | 17 reaches both sides of the row count at which fc1 and fc2 take
    the ring (mlp_pm), with 3 frames for the compact last layer; the full-tower and tower_features rows; the ring cap of set_tower_share; MMDUET_NO_FUSE=2 in a context
    created under it."""
import pytest
import torch

pytestmark = pytest.mark.gpu
import tower_regimes as T

TORCH_DTYPE = {T.F32: torch.float32, T.BF16: torch.bfloat16}
TOWER_DTYPE = {'fp32': None, 'bf16': 'bf16', 'fp16': 'fp16', 'fp16_resid16': 'fp16_resid16'}
R = T.rows_by_name()


def _finalized(pcfg, mode, max_vit_batch, seed):
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    from mmduet_amd.weights import synthetic_weights
    dtype = TORCH_DTYPE[T.MODES[mode][0]]
    if TOWER_DTYPE[mode]:
        pcfg.tower_dtype = TOWER_DTYPE[mode]
    m = VideoHeadLiveLlavaQwenForCausalLM(pcfg, torch_dtype=dtype, max_vit_batch=max_vit_batch, max_step_tokens=64, kv_initial_tokens=256)
    assert m.tower_dtype == mode
    for name, t in synthetic_weights(pcfg, seed=seed, device=m.device, dtype=dtype, scale='unit'):
        m.load_tensor(name, t)
    m.finalize()
    return m


def _pixels(m, B, seed):
    s = m.config.vit_image_size
    return torch.randn(B, 3, s, s, generator=torch.Generator().manual_seed(seed)).to(m.dtype).cuda()


def _check(m, row, B):
    """the plan of the run just made is the row's, and the stage-0 tap refuses exactly when it says sparse_last"""
    from mmduet_amd._lib import MmduetError
    plan = m.tower_last_plan()
    assert tuple(plan) == T.FIELDS and tuple(plan.values()) == row.plan, (row.name, plan)
    if plan['sparse_last']:
        with pytest.raises(MmduetError, match='set_full_tower'):
            m.vit_debug_tap(0, B)
    else:
        assert torch.isfinite(m.vit_debug_tap(0, B).float()).all()


def _run(m, row, seed=5):
    """a row through the public entry that reaches it: visual_embed (for the pool), under set_full_tower / set_tower_share where the row says so"""
    assert row.for_pool and not row.model and m.max_vit_batch >= row.B
    if row.ring is not None:
        m.set_tower_share(row.ring)
    m.set_full_tower(row.full_tower)
    try:
        y = m.visual_embed(_pixels(m, row.B, seed))
        _check(m, row, row.B)
    finally:
        m.set_full_tower(False)
    assert y.shape == (row.B * m.tokens_per_frame, m.config.hidden_size) and torch.isfinite(y.float()).all(), row.name
    return y


# ---- the sparse / full gate -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=[(mode, grid) for mode in ('bf16', 'fp16') for grid in (12, 16)], ids=lambda p: f'{p[0]}-grid{p[1]}')
def small(request):
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    mode, grid = request.param
    img, out = grid * 14, -(-grid // 4)
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                                        vit_hidden_size=64, vit_intermediate_size=128, vit_num_hidden_layers=3, vit_layers_removed=1, vit_num_attention_heads=4,
                                        vit_image_size=img, vit_patch_size=14, video_pooling_stride=4, frame_num_tokens=out * out, frame_resolution=img, v_placeholder='<image>')
    m = _finalized(pcfg, mode, 8, seed=7)
    yield mode, grid, m
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize('B', [1, 2, 3])
def test_small_tower_takes_the_gate_of_the_table(small, B):
    mode, grid, m = small
    row = R[f'{mode}_g{grid}_b{B}']
    assert T.TOWERS[row.tower]['grid'] == grid and T.TOWERS[row.tower]['max_batch'] == m.max_vit_batch
    ve = _run(m, row, seed=grid + B)
    full = _run(m, row._replace(full_tower=True, plan=_full(row.plan)), seed=grid + B)
    if not row.plan[T.FIELDS.index('sparse_last')]:          # both calls ran the SAME (full) schedule
        assert torch.equal(ve, full)


def _full(plan):
    """the same run under set_full_tower(True): no compact last layer, the projector gathers its rows itself"""
    p = dict(zip(T.FIELDS, plan))
    p.update(sparse_last=0, compact_rows=0, proj_gather=p['proj_compact'], mlp_pm_last=0)
    return tuple(p.values())


def test_the_full_tower_plan_of_the_table_is_the_rule_used_above():
    for a, b in (('bf16_true_b3', 'bf16_true_full_tower'), ('fp16_true_b3', 'fp16_true_full_tower'), ('fp32_true_b3', 'fp32_true_full_tower')):
        assert _full(R[a].plan) == R[b].plan


# ---- true width: residual forms, piece-major on both sides of the ring's row count -------------------------------------------------------------------------------------
MAX_B = 17
TRUE_ROWS = {
    'fp32': ('fp32_true_b3', 'fp32_true_full_tower', 'fp32_true_b17'),
    'bf16': ('bf16_true_b3', 'bf16_true_full_tower', 'bf16_true_b16', 'bf16_true_b17', 'bf16_true_b16_share', 'bf16_true_b17_share'),
    'fp16': ('fp16_true_b3', 'fp16_true_full_tower', 'fp16_true_b16', 'fp16_true_b17', 'fp16_true_b17_share'),
    'fp16_resid16': ('r16_true_b3', 'r16_true_b16', 'r16_true_b17', 'r16_true_full_tower_b17'),
}


def _true_model(mode):
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=1, vit_num_hidden_layers=3, vit_layers_removed=1, frame_num_tokens=49, frame_resolution=384,
                                        v_placeholder='<image>')
    return _finalized(pcfg, mode, MAX_B, seed=3)


@pytest.fixture(scope='module', params=list(TRUE_ROWS))
def true_width(request):
    m = _true_model(request.param)
    yield request.param, m
    del m
    torch.cuda.empty_cache()


def test_true_width_takes_the_plans_of_the_table(true_width):
    mode, m = true_width
    t = T.TOWERS['true']
    assert (m.config.vit_hidden_size, m.config.vit_grid, m.config.video_pooling_stride) == (t['C'], t['grid'], t['pool_stride'])
    for name in TRUE_ROWS[mode]:          # (the ring-cap rows last: set_tower_share stays set)
        assert R[name].mode == mode and R[name].tower == 'true', name
        _run(m, R[name])
    # tower_features: a full-tower encode of its own (the caller's setting survives it)
    f = m.tower_features(_pixels(m, 3, 9))
    assert tuple(m.tower_last_plan().values()) == _full(R[TRUE_ROWS[mode][0]].plan) and torch.isfinite(f.float()).all()
    assert _run(m, R[TRUE_ROWS[mode][0]]) is not None          # ... sparse again afterwards


def test_no_fuse_2_keeps_the_intermediates_row_major(monkeypatch):
    monkeypatch.setenv('MMDUET_NO_FUSE', '2')          # read when the context is created
    m = _true_model('bf16')
    monkeypatch.delenv('MMDUET_NO_FUSE')
    _run(m, R['bf16_true_b17_no_fuse2'])
    assert R['bf16_true_b17'].plan[T.FIELDS.index('mlp_pm')] == 1 and R['bf16_true_b17_no_fuse2'].plan[T.FIELDS.index('mlp_pm')] == 0


def test_the_plan_is_the_contexts_most_recent_run(true_width):
    mode, m = true_width
    names = TRUE_ROWS[mode]
    _run(m, R[names[0]])
    _run(m, R[names[1]])
    assert tuple(m.tower_last_plan().values()) == R[names[1]].plan
