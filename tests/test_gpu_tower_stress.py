"""The vision tower on the statistics of a real checkpoint (tests/tower_stress.py), in every tower mode: the fp32 model, the bf16 tower, the autocast tower with the
fp32 residual stream ('fp16') and with the fp16 one ('fp16_resid16').  True width (C = 1152, 16 heads of 72, 729 tokens), 2 tower layers, 3 frames in a model built
for 4 (B x 196 = 588 compact rows: the fp16 towers take the sparse last layer).  One model per (mode, pattern) at a time -- weights cannot be reloaded once finalized.

Per mode and pattern:
  * tower_features (full last layer) against the fp32 oracle, the error bounded SEPARATELY on the pattern's outlier channels and on all other channels;
  * visual_embed with the sparse last layer (the default; vit_debug_tap must refuse afterwards) and with set_full_tower(True) (the tap must work), each against the
    oracle's visual_embed, the error bounded separately on the pooled rows whose 2 x 2 taps include a register token and on the rest; sparse against full no farther
    apart than the farther of the two is from the fp32 oracle;
  * the stage-0 tap on the rows that feed the pool's border taps (tower_stress.border_tap_tokens: no tap of the 27 -> 7 pool clamps, see that module), by channel group;
  * half_overflow: the frames that hold a non-finite value are the same in the product and in oracle.duet_oracle.vit_forward_autocast_fp16 (the one frame whose fc2
    output passes 65 520: fp16 gives inf there; a tower that saturated at 65 504 would stay finite and fail), every other frame finite and inside the bound.
The bound of a group is the project's existing form, keyed on the mode alone: 1e-3 x scale for the fp32 model, 3 x d_oracle + 2e-2 x scale for a 16-bit tower, where
d_oracle is the matching-precision oracle's own distance to the fp32 oracle and scale = max(1, max|ref|), BOTH over the same group.
Besides: visual_embed_frames == preprocess -> visual_embed bit for bit on frames that make the resampler clip at both ends, and preprocess == Pillow's resampler
restated + normalise, bit for bit, on the golden model for 56, 28, 84, 112 and 57 -> 56.

Every measured (ours, oracle, scale) goes through _record of tests/test_gpu_production.py (keys 'tower_stress/...'); the table is profiles/r13_tower_stress.md.

Measured on an MI355X, largest d_ours / bound per mode: fp32 0.002, bf16 0.21 (register_tokens, tap on the border rows, other channels), fp16 0.16
(outlier_channels, visual_embed, other rows), fp16_resid16 0.18 (gelu_saturation, tower_features).  Sparse and full last layer: the same bits in the fp32 and both fp16
towers, within one bf16 ulp in the bf16 tower.  No kernel bug was found by these cases.

Mutants (throw-away builds of the library, each run once over this file and the older tower tests; details in profiles/r13_tower_stress.md):
  (a) gather_pool_rows_kernel takes y0 for both vertical taps: test_what_the_llm_sees... fails in 14 of 16 cases (not under half_range, where the channel at 45 056 sets
      the scale); older: test_tower_batch_of_35_frames_true_width, test_fp32_mode_true_width_meets_1e3, test_fp16_tower_true_width_error_against_fp32,
      test_vit_projector_pool_true_shape, test_fp32_mode_full_depth_30_frames_meets_1e3, test_fp16_tower_small_grids_fall_back_to_the_full_last_layer fail too.
  (b) resid32_layernorm_kernel with the variance as E[x^2] - mean^2 (the kernel has the two-pass form): survives everything, and is equivalent within rounding on these
      inputs -- the one-pass form loses 2^-24 (1 + mean^2 / var) of the variance, and a row with a few channels at 10^3 .. 10^4 among 1152 has |mean| << its standard
      deviation.  Only a common offset of thousands of standard deviations on a whole row would separate the two; neither a real checkpoint's statistics nor a
      pattern here has one.
  (c) f2h / from_f<f16_t> clamp to +-65 504: all four half_overflow tests fail (the product stays finite where the oracle is inf); no older test notices.
  (d) the sparse last layer's n_ctx one 64-key tile short: caught by the sparse-versus-full clause under gelu_saturation (all modes) and fp32-outlier_channels, and by
      the older test_fp32_mode_full_depth_30_frames_meets_1e3; register_tokens did not see it with its keys at tokens 0, 52 and 93, which is why the third register token
      now sits in the last key tile (token 714) -- changed after the run, the mutant was not run again.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from oracle import duet_oracle as O
from oracle.preprocess import pil_resize_bicubic_u8
import tower_stress as TS

N_FRAMES = 3
CASES = [(mode, pattern) for mode in TS.MODES for pattern in TS.PATTERNS if pattern not in TS.HALF_ONLY or mode.startswith('fp16')]


def _record(key, **vals):
    from test_gpu_production import _record as record          # the suite's record of measured parity figures; these rows sit under 'tower_stress/'
    record('tower_stress/' + key, **vals)


def _build(mode, pattern):
    """as _build(1, 2, ...) of tests/test_gpu_production.py, with the tower tensors of `pattern` (None: the plain scale='unit' weights)"""
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    from mmduet_amd.weights import synthetic_weights
    dtype, tower = TS.MODES[mode]
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=1, vit_num_hidden_layers=3, vit_layers_removed=1, frame_num_tokens=49, frame_resolution=384,
                                        v_placeholder='<image>')
    ocfg = O.OracleConfig(vocab_size=2048, num_hidden_layers=1, vit_layers=2)
    if tower:
        pcfg.tower_dtype = tower
    m = VideoHeadLiveLlavaQwenForCausalLM(pcfg, torch_dtype=dtype, max_vit_batch=4, max_step_tokens=64, kv_initial_tokens=256)
    assert m.tower_dtype == mode
    w = dict(synthetic_weights(pcfg, seed=3, device=m.device, dtype=dtype, scale='unit'))
    if pattern:
        w = TS.stress_tower_weights(w, ocfg, pattern)
    for name, t in w.items():
        m.load_tensor(name, t)
    m.finalize()
    vis = {k: v for k, v in w.items() if k.startswith(O.VT) or k.startswith('model.mm_projector')}          # all the oracles of this file need
    return m, vis, ocfg


class Case:
    pass


@pytest.fixture(scope='module', params=CASES, ids=[f'{m}-{p}' for m, p in CASES])
def case(request):
    """model, pixels and the references of one (mode, pattern): the references are computed once here, shared by the tests below and never changed"""
    c = Case()
    c.mode, c.pattern = request.param
    c.m, w, c.cfg = _build(c.mode, c.pattern)
    dtype = TS.MODES[c.mode][0]
    c.px = TS.stress_pixels(c.pattern, N_FRAMES, seed=7, device=c.m.device, dtype=dtype)
    w32 = {k: v.float() for k, v in w.items()}
    half = c.mode.startswith('fp16')
    c.ref_tower = O.vit_forward(w32, c.cfg, c.px.float())
    c.ref_embed = O.visual_embed(w32, c.cfg, c.px.float())
    if c.mode == 'fp32':
        c.or_tower = c.or_embed = None
    else:
        c.or_tower = (O.vit_forward_autocast_fp16 if half else O.vit_forward)(w, c.cfg, c.px).float()
        c.or_embed = O.visual_embed(w, c.cfg, c.px, tower_autocast_fp16=half).float()
    # the frames in which the matching-precision oracle is finite: all of them, but for the offset frame of half_overflow
    c.bad_frames = [TS.BRIGHT_FRAME] if c.pattern == 'half_overflow' else []
    c.good = [b for b in range(N_FRAMES) if b not in c.bad_frames]
    assert torch.isfinite(c.ref_tower).all() and torch.isfinite(c.ref_embed).all()
    if c.or_tower is not None:
        assert _bad_frames(c.or_tower) == c.bad_frames and _bad_frames(c.or_embed.view(N_FRAMES, -1)) == c.bad_frames
    # the statistic the pattern is named for holds on THESE weights and pixels too (tests/test_tower_stress_host.py checks all of them on the host's)
    ch = TS.outlier_channels_of(c.pattern)
    if c.pattern == 'outlier_channels':
        assert all(1e3 <= c.ref_tower[..., k].abs().min().item() and c.ref_tower[..., k].abs().max().item() <= 1e4 for k in ch)
    if c.pattern == 'register_tokens':
        reg = TS.register_tokens(c.cfg)
        for s in TS.trace_fp32(w32, c.cfg, c.px[:1].float())['scores']:
            assert 30.0 <= s[..., reg].min().item() and s[..., reg].max().item() <= 80.0
            assert torch.softmax(s.double(), -1)[..., reg].sum(-1).min().item() >= 1 - 1e-3
    if c.pattern in TS.HALF_ONLY:
        v = c.ref_tower[c.good][..., TS.HALF_CH]
        assert 3e4 <= v.min().item() and v.max().item() <= 6e4
    c.ch_groups = TS.channel_groups(c.cfg.vit_hidden_size, ch, device=c.m.device)
    yield c
    c.__dict__.clear()          # the model is freed before the next one is built
    del w, w32
    torch.cuda.empty_cache()


def _bad_frames(t):
    return [b for b in range(t.shape[0]) if not bool(torch.isfinite(t[b].float()).all())]


def _hold(c, what, ours, oracle, ref, groups):
    """record and assert the grouped bound; returns the largest |ours - ref| over the groups"""
    worst = 0.0
    res = TS.grouped_distances(ours.float(), oracle, ref, groups)
    fails = []
    for name, (d, d_or, scale) in res.items():
        bound = TS.bound_of(c.mode, d_or, scale)
        print(f'{c.mode} {c.pattern} {what} {name}: ours {d:.4g} oracle {d_or:.4g} scale {scale:.4g} bound {bound:.4g} ratio {d / bound:.3f}')
        _record(f'{c.mode}/{c.pattern}/{what}/{name}', ours=d, oracle=d_or, scale=scale, bound=bound, ratio=d / bound)
        worst = max(worst, d)
        if not d <= bound:
            fails.append((name, d, d_or, scale, bound))
    assert not fails, (c.mode, c.pattern, what, fails)
    return worst


def _frames(t, idx, per):
    """the rows of frames `idx` of a [B * per, H] tensor"""
    return t.view(-1, per, t.shape[-1])[idx].reshape(-1, t.shape[-1])


def test_full_tower_against_the_oracle_by_channel_group(case):
    c = case
    f = c.m.tower_features(c.px)
    assert f.shape == (N_FRAMES, 729, 1152) and f.dtype == TS.MODES[c.mode][0]
    assert _bad_frames(f) == c.bad_frames
    if c.bad_frames:          # inf on the overflowing channel -- in every token, as in the oracle -- and nothing else
        col = f[TS.BRIGHT_FRAME][:, TS.HALF_CH].float()
        assert torch.isinf(col).all() and (col > 0).all()
        assert torch.equal(torch.isfinite(f[TS.BRIGHT_FRAME].float()), torch.isfinite(c.or_tower[TS.BRIGHT_FRAME]))
    _hold(c, 'tower_features', f[c.good], None if c.or_tower is None else c.or_tower[c.good], c.ref_tower[c.good], c.ch_groups)


def test_what_the_llm_sees_sparse_and_full_by_row_group(case):
    from mmduet_amd._lib import MmduetError
    c = case
    per = c.cfg.frame_num_tokens
    sparse = c.m.visual_embed(c.px)
    with pytest.raises(MmduetError, match='set_full_tower'):          # the sparse last layer really ran: there is no full tower output to tap
        c.m.vit_debug_tap(0, N_FRAMES)
    c.m.set_full_tower(True)
    try:
        full = c.m.visual_embed(c.px)
        tap = c.m.vit_debug_tap(0, N_FRAMES).view(N_FRAMES, 729, 1152)
    finally:
        c.m.set_full_tower(False)
    assert sparse.shape == full.shape == (N_FRAMES * per, 3584)
    groups = TS.embed_row_groups(c.cfg, len(c.good), device=c.m.device)
    ref = _frames(c.ref_embed, c.good, per)
    oracle = None if c.or_embed is None else _frames(c.or_embed, c.good, per)
    d = {}
    for name, y in (('visual_embed_sparse', sparse), ('visual_embed_full', full)):
        assert _bad_frames(y.view(N_FRAMES, -1)) == c.bad_frames, name
        d[name] = _hold(c, name, _frames(y, c.good, per), oracle, ref, groups)
    apart = (_frames(sparse, c.good, per).float() - _frames(full, c.good, per).float()).abs().max().item()
    _record(f'{c.mode}/{c.pattern}/sparse_vs_full', apart=apart, sparse_vs_fp32=d['visual_embed_sparse'], full_vs_fp32=d['visual_embed_full'])
    assert apart <= max(d.values()), (apart, d)
    # the stage-0 tap (the full last layer's output) on the rows that feed the pool's border taps
    rows = torch.tensor(TS.border_tap_tokens(c.cfg), device=c.m.device)
    pick = lambda t: t[c.good][:, rows]
    _hold(c, 'tap0_border_rows', pick(tap), None if c.or_tower is None else pick(c.or_tower), pick(c.ref_tower), c.ch_groups)


# ---- the fused uint8 entry on saturated pixels --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=list(TS.MODES))
def plain(request):
    m, _, _ = _build(request.param, None)
    yield m
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize('R', [336, 384, 768])
def test_fused_entry_is_bit_identical_on_saturated_frames(plain, R):
    m = plain
    for kind in TS.FRAME_KINDS:
        fr = TS.stress_frames(kind, 2, R)
        pv = m.get_vision_tower().image_processor.preprocess(fr)['pixel_values']
        assert pv.shape == (2, 3, 384, 384) and pv.float().abs().max().item() <= 1.0
        two = m.visual_embed(pv)
        one = m.visual_embed_frames(fr)
        assert torch.isfinite(one.float()).all() and torch.equal(one, two), (kind, R)


@pytest.fixture(scope='module')
def golden():
    from helpers import hip_model
    ms = {dt: hip_model('A', dt)[0] for dt in (torch.float32, torch.bfloat16)}
    yield ms
    ms.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('R', [56, 28, 84, 112, 57])
def test_preprocess_equals_the_restated_resampler_on_saturated_frames(golden, R):
    for kind in TS.FRAME_KINDS:
        fr = TS.stress_frames(kind, 2, R)
        u8 = np.stack([pil_resize_bicubic_u8(f.transpose(1, 2, 0), 56).transpose(2, 0, 1) for f in fr.numpy()])
        ref = (torch.from_numpy(u8).float() * np.float32(1 / 255) - 0.5) / 0.5
        for dt, m in golden.items():
            pv = m.get_vision_tower().image_processor.preprocess(fr)['pixel_values']
            assert pv.dtype == dt and torch.equal(pv.cpu(), ref.to(dt)), (kind, R, dt)
