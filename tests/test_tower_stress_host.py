"""The builders of tests/tower_stress.py really build what their names claim, checked on the host in the fp32 oracle at the true tower width (C = 1152, 16 heads of
72, 729 tokens, 2 layers, one frame; two for half_overflow) -- so tests/test_gpu_tower_stress.py cannot silently turn benign when someone retunes a constant --, the
matching-precision oracles stay finite wherever the GPU test demands a finite product, and the grouped bound closes the gap it was written for: a tower output whose
non-outlier channels are all zero passes the old whole-tensor bound and fails the grouped one.  Pillow's resampler and its restatement agree on the saturated frames."""
import functools
import numpy as np
import pytest
import torch
from oracle import duet_oracle as O
from oracle.preprocess import pil_resize_bicubic_u8
import tower_stress as TS

CFG = O.OracleConfig(vocab_size=64, num_hidden_layers=0, vit_layers=2)


@functools.lru_cache(maxsize=None)
def _base():
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    from mmduet_amd.weights import synthetic_weights
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=64, num_hidden_layers=0, vit_num_hidden_layers=3, vit_layers_removed=1, frame_num_tokens=49, frame_resolution=384,
                                        v_placeholder='<image>')
    return {n: t for n, t in synthetic_weights(pcfg, seed=3, device='cpu', dtype=torch.bfloat16, scale='unit') if n.startswith(O.VT)}


@functools.lru_cache(maxsize=None)
def _case(pattern):
    """(weights, pixels, fp32 trace) of one pattern: computed once, shared, never changed"""
    w = TS.stress_tower_weights(_base(), CFG, pattern)
    px = TS.stress_pixels(pattern, 2 if pattern == 'half_overflow' else 1).to(torch.bfloat16)
    return w, px, TS.trace_fp32(w, CFG, px)


def test_trace_is_the_oracle():
    w, px, tr = _case('outlier_channels')
    assert torch.equal(tr['out'], O.vit_forward({k: v.float() for k, v in w.items()}, CFG, px.float()))


def test_only_tower_tensors_change_and_the_copy_keeps_names_and_dtypes():
    base = dict(_base()); base['model.mm_projector.0.weight'] = torch.ones(2, 2)
    for pattern in TS.PATTERNS:
        w = TS.stress_tower_weights(base, CFG, pattern)
        assert w.keys() == base.keys() and all(w[k].dtype == base[k].dtype and w[k].shape == base[k].shape for k in base)
        changed = [k for k in base if not torch.equal(w[k], base[k])]
        assert changed and all(k.startswith(O.VT) for k in changed), (pattern, changed)
        assert w['model.mm_projector.0.weight'] is base['model.mm_projector.0.weight']
    assert torch.equal(_base()[O.VT + 'embeddings.position_embedding.weight'], base[O.VT + 'embeddings.position_embedding.weight'])          # the input is not written


def test_no_tap_of_the_true_pool_clamps_and_the_register_tokens_sit_where_the_names_say():
    """27 -> 7: 14 distinct indices per axis, none at the border, 196 distinct tokens (module docstring of tests/tower_stress.py)"""
    taps, compact, axis = TS.pool_geometry(CFG)
    assert axis == [1, 2, 5, 6, 9, 10, 13, 14, 16, 17, 20, 21, 24, 25]
    assert all(i1 == i0 + 1 for i0, i1, _ in taps) and len(set(compact)) == len(compact) == 196
    assert [round(t[2], 6) == 0 for t in taps] == [False, False, False, True, False, False, False]
    t1, t2, t3 = TS.register_tokens(CFG)
    assert t1 == 0 and divmod(t2, 27) == (1, 25) and t1 not in compact and t3 not in compact and compact.index(t2) == 13
    assert divmod(t3, 27) == (26, 12) and t3 >= 729 // 64 * 64          # a key of the last, 25-wide tile: a kernel that lost its tail keys loses a third of the mass
    assert TS.pooled_rows_reading(CFG, [t1, t2, t3]) == [6]
    border = TS.border_tap_tokens(CFG)
    assert t2 in border and len(border) == 14 * 14 - 11 * 11 and set(border) <= set(compact)


def test_outlier_channels_grow_per_layer_into_the_thousands():
    _, _, tr = _case('outlier_channels')
    rest = TS.channel_groups(1152, list(TS.OUTLIER_CH))['other_channels']
    peak = [[h[..., c].abs().max().item() for c in TS.OUTLIER_CH] for h in tr['h']]
    print('outlier_channels: max|h| per layer', peak, 'elsewhere', tr['out'][..., rest].abs().max().item())
    for k in range(2):
        assert peak[0][k] < peak[1][k] < peak[2][k]
        assert 1e3 <= peak[2][k] <= 1e4
        assert tr['out'][..., TS.OUTLIER_CH[k]].abs().min().item() >= 1e3          # on every token
    assert all(h[..., rest].abs().max().item() < 100.0 for h in tr['h'])


def test_register_tokens_take_the_attention_mass_of_every_row():
    _, _, tr = _case('register_tokens')
    reg = TS.register_tokens(CFG)
    for s in tr['scores']:
        hot = s[..., reg]
        rest = s.clone(); rest[..., reg] = float('-inf')
        mass = torch.softmax(s.double(), -1)[..., reg].sum(-1)
        print(f'register_tokens: scores on the three keys {hot.min().item():.1f} .. {hot.max().item():.1f}, others <= {rest.max().item():.1f}, least mass {mass.min().item():.9f}')
        assert 30.0 <= hot.min().item() and hot.max().item() <= 80.0
        assert rest.max().item() <= 15.0 and s.median().abs().item() < 3.0
        assert mass.min().item() >= 1 - 1e-3
    # ... so the attention contribution of every row is pinned to those tokens' V rows: out_proj of a convex combination of three rows
    w, px, _ = _case('register_tokens')
    w32 = {k: v.float() for k, v in w.items()}
    p = O.VT + 'encoder.layers.0.'
    x = O.layer_norm(tr['h'][0], w32[p + 'layer_norm1.weight'], w32[p + 'layer_norm1.bias'], CFG.vit_layer_norm_eps)
    v = O.linear(x, w32[p + 'self_attn.v_proj.weight'], w32[p + 'self_attn.v_proj.bias']).view(1, 729, 16, 72).transpose(1, 2)
    a3 = torch.softmax(tr['scores'][0][..., reg], -1)
    o3 = torch.matmul(a3, v[:, :, reg]).transpose(1, 2).reshape(1, 729, 1152)
    pinned = O.linear(o3, w32[p + 'self_attn.out_proj.weight'], w32[p + 'self_attn.out_proj.bias'])
    assert (pinned - tr['out_proj'][0]).abs().max().item() <= 1e-3


def test_gelu_saturation_reaches_6_to_50_on_both_signs():
    _, _, tr = _case('gelu_saturation')
    for pre in tr['pre']:
        mx, mn = pre.amax((0, 1)), pre.amin((0, 1))
        print('gelu_saturation: columns reaching >= 6:', int((mx >= 6).sum()), ' <= -6:', int((mn <= -6).sum()), ' max|x|', pre.abs().max().item())
        assert int((mx >= 6).sum()) >= 200 and int((mn <= -6).sum()) >= 200
        assert pre.abs().max().item() <= 50.0
        benign = torch.maximum(mx, -mn) < 6          # the other ~3900 columns stay O(1)
        assert pre[..., benign].abs().max().item() < 6.0 and int(benign.sum()) >= 3800


def test_half_range_and_overflow_land_where_fp16_has_an_ulp_of_32_and_past_65520():
    _, _, tr = _case('half_range')
    y = tr['fc2'][-1][..., TS.HALF_CH]
    assert 3e4 <= y.min().item() and y.max().item() <= 6e4 and y.min().item() != y.max().item()
    _, _, tr = _case('half_overflow')
    y = tr['fc2'][-1][..., TS.HALF_CH]
    print('half_overflow: pre-rounding fc2 value per frame', [(y[b].min().item(), y[b].max().item()) for b in range(2)])
    assert 3e4 <= y[0].min().item() and y[0].max().item() <= 6e4
    assert y[TS.BRIGHT_FRAME].min().item() > 65520.0          # every token of that frame, so every compact row of the sparse last layer too
    assert TS.HALF_BASE == float(torch.tensor(TS.HALF_BASE).to(torch.bfloat16)) == float(torch.tensor(TS.HALF_BASE).to(torch.float16))


@pytest.mark.parametrize('pattern', TS.PATTERNS)
def test_matching_precision_oracles_are_finite_where_the_product_must_be(pattern):
    w, px, tr = _case(pattern)
    assert torch.isfinite(tr['out']).all()
    if pattern not in TS.HALF_ONLY:
        assert torch.isfinite(O.vit_forward(w, CFG, px).float()).all()          # the bf16 tower's oracle
    ac = O.vit_forward_autocast_fp16(w, CFG, px).float()
    bad = [b for b in range(px.shape[0]) if not torch.isfinite(ac[b]).all()]
    assert bad == ([TS.BRIGHT_FRAME] if pattern == 'half_overflow' else []), bad
    if pattern == 'half_overflow':
        col = ac[TS.BRIGHT_FRAME][:, TS.HALF_CH]
        assert torch.isinf(col).all() and (col > 0).all()          # inf, not 65504: torch's half rounds to nearest, and 65520 is the tie that goes to 2^16
        rest = TS.channel_groups(1152, [TS.HALF_CH])['other_channels']
        assert torch.isfinite(ac[TS.BRIGHT_FRAME][:, rest]).all()


def test_a_tower_output_without_its_small_channels_passes_the_old_bound_and_fails_the_grouped_one():
    """`bad` = the bf16 oracle's output with every non-outlier channel set to zero.  The old measure, one max-norm figure over the whole tensor held to
    3 x |bf16 oracle - fp32 oracle| + 2e-2 x max|ref|, allows ~100 on every element here (max|ref| ~ 5000) and the small channels are all below 70: it passes.  Over the
    other-channels group alone the same form allows 3 x 0.7 + 2e-2 x 70."""
    w, px, tr = _case('outlier_channels')
    ref = tr['out']
    good = O.vit_forward(w, CFG, px).float()
    groups = TS.channel_groups(1152, list(TS.OUTLIER_CH))
    bad = good.clone(); bad[..., groups['other_channels']] = 0.0
    scale = ref.abs().max().item()
    old_bound = 3 * (good - ref).abs().max().item() + 2e-2 * max(1.0, scale)
    assert (good - ref).abs().max().item() <= old_bound and (bad - ref).abs().max().item() <= old_bound          # the gap: the old bound is blind to it
    res_good, res_bad = TS.grouped_distances(good, good, ref, groups), TS.grouped_distances(bad, good, ref, groups)
    print('grouped:', {k: (round(v[0], 3), round(TS.bound_of('bf16', v[1], v[2]), 3)) for k, v in res_bad.items()}, 'old bound', round(old_bound, 1))
    for name in groups:
        d, d_or, sc = res_good[name]
        assert d <= TS.bound_of('bf16', d_or, sc)
    d, d_or, sc = res_bad['other_channels']
    assert d > 10 * TS.bound_of('bf16', d_or, sc)
    d, d_or, sc = res_bad['outlier_channels']
    assert d <= TS.bound_of('bf16', d_or, sc)


def test_stress_frames_are_saturated_and_seeded():
    for kind in TS.FRAME_KINDS:
        fr = TS.stress_frames(kind, 3, 57)
        assert fr.dtype == torch.uint8 and fr.shape == (3, 3, 57, 57) and set(fr.unique().tolist()) <= {0, 255}
        assert torch.equal(fr, TS.stress_frames(kind, 3, 57))
        assert torch.equal(fr[:, 1], 255 - fr[:, 0]) and torch.equal(fr[:, 2], fr[:, 0])
    assert int(TS.stress_frames('zeros', 1, 8)[:, 0].max()) == 0 and int(TS.stress_frames('full', 1, 8)[:, 0].min()) == 255
    c1, c2, st = (TS.stress_frames(k, 2, 8)[0, 0] for k in ('checker1', 'checker2', 'stripes'))
    assert (c1[0, :4].tolist(), c1[1, :4].tolist()) == ([0, 255, 0, 255], [255, 0, 255, 0])
    assert (c2[0, :4].tolist(), c2[2, :4].tolist()) == ([0, 0, 255, 255], [255, 255, 0, 0])
    assert st[0].tolist() == [0, 0, 0, 255, 255, 255, 0, 0] and torch.equal(st[0], st[5])
    assert torch.equal(TS.stress_frames('stripes', 2, 8)[1, 0], st.T)


@pytest.mark.parametrize('R', [56, 28, 84, 112, 57])
@pytest.mark.parametrize('kind', TS.FRAME_KINDS)
def test_resampler_restatement_equals_pillow_on_saturated_frames(kind, R):
    fr = TS.stress_frames(kind, 2, R).numpy()
    mine = [pil_resize_bicubic_u8(f.transpose(1, 2, 0), 56) for f in fr]
    if kind in ('checker1', 'checker2', 'stripes') and (R == 28 or (R == 57 and kind != 'checker1')):
        assert {0, 255} <= set(np.unique(mine[0][..., 0]).tolist()) and len(np.unique(mine[0])) > 2          # the bicubic overshoot is clipped at both ends
    try:
        from PIL import Image
    except ImportError:
        return          # (the restatement ran; only the comparison needs Pillow)
    for f, m in zip(fr, mine):
        ref = np.asarray(Image.fromarray(f.transpose(1, 2, 0)).resize((56, 56), resample=Image.BICUBIC))
        assert np.array_equal(m, ref), (kind, R)
