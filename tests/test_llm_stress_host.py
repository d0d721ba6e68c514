"""The builders of tests/llm_stress.py really build what their names claim, checked on the host in the fp32 oracle at the true decoder width (H 3584, I 18944, 28 / 4
heads of 128, 2 layers) over one 330-row stream and one 1100-row stream (the 1000-row prefix of the device test and 100 step rows) -- on the very weights, prefixes and
seeds tests/test_gpu_llm_stress.py uses, so that test cannot silently turn benign when someone retunes a constant.  The sink's mass band is also checked on rows
4192 .. 4899 of the device test's longest stream (its 4200-row prefix and the 700-row step behind it).  The bf16 oracle stays finite on every pattern, and
nothing but the named decoder tensors changes."""
import functools
import math
import pytest
import torch
from oracle import duet_oracle as O
import llm_stress as LS


@functools.lru_cache(maxsize=1)
def _case(pattern):
    """(weights, config, {S: (rows, fp32 trace)}) of one pattern: computed once, shared by the tests of that pattern, never changed"""
    cfg = LS.oracle_config()
    w = LS.stress_llm_weights(LS.base_weights(), cfg, pattern)
    xs = {330: LS.prefix_embeds(cfg, 330), 1100: torch.cat([LS.prefix_embeds(cfg, 1000), LS.stress_embeds(cfg, 100, False, LS.STEP_SEED)])}
    return w, cfg, {S: (x, LS.trace_fp32(w, cfg, x)) for S, x in xs.items()}


@pytest.fixture(scope='module', params=LS.PATTERNS)
def case(request):
    return (request.param,) + _case(request.param)


def test_trace_is_the_oracle_and_the_bf16_oracle_stays_finite(case):
    pattern, w, cfg, runs = case
    x, tr = runs[330]
    w32 = {k: w[k].float() for k in LS.decoder_names(w)}
    ref, _ = O.llm_forward(w32, cfg, x.float(), None)
    assert torch.equal(tr['out'], ref) and torch.isfinite(ref).all() and torch.isfinite(runs[1100][1]['out']).all()
    h16, kv = O.llm_forward(w, cfg, x, None)
    assert h16.dtype == torch.bfloat16 and torch.isfinite(h16.float()).all() and len(kv) == 330


def test_only_the_named_decoder_tensors_change(case):
    pattern, w, cfg, _ = case
    base = LS.base_weights()
    named = {'sink': ('input_layernorm.weight', 'q_proj.weight', 'q_proj.bias', 'k_proj.weight', 'k_proj.bias'),
             'qk_bias': ('q_proj.bias', 'k_proj.bias'),
             'outlier_channels': ('v_proj.bias', 'o_proj.weight', 'down_proj.weight', 'input_layernorm.weight', 'post_attention_layernorm.weight', 'q_proj.weight',
                                  'k_proj.weight', 'v_proj.weight', 'gate_proj.weight', 'up_proj.weight', 'model.norm.weight'),
             'swiglu_saturation': ('gate_proj.weight',)}[pattern]
    assert w.keys() == base.keys()
    changed = [k for k in base if w[k] is not base[k]]
    assert changed and all(k in LS.decoder_names(base) and k.endswith(named) for k in changed), changed
    assert all(not torch.equal(w[k], base[k]) and w[k].dtype == base[k].dtype and w[k].shape == base[k].shape for k in changed)
    assert any(k.startswith(O.VT) for k in base) and 'lm_head.weight' in base          # the tower, the projector, the embedding and the heads: the input's own tensors


def _sink_key_0_takes_half_to_99_percent_of_every_later_rows_mass(w, cfg, runs):
    for S, (x, tr) in runs.items():
        assert x[0, list(LS.SINK_CH)].float().abs().min().item() >= 1e3 and x[0].float().abs().max().item() <= 1e4
        rest = LS.channel_groups(cfg.hidden_size, list(LS.SINK_CH))['other_channels']
        assert x[1:].float().abs().max().item() < 10 and x[0, rest].float().abs().max().item() < 10
        for h in tr['h'] + tr['mid']:          # ... and the residual stream keeps it: row 0 alone, on those two channels alone
            assert h[0, list(LS.SINK_CH)].abs().min().item() >= 1e3 and h[1:].abs().max().item() < 100 and h[0, rest].abs().max().item() < 100
        for i, s in enumerate(tr['scores']):
            mass = torch.softmax(s.double(), -1)[:, 1:, 0]          # [head, later row]
            print(f'sink: {S} rows, layer {i}: key 0 takes {mass.min().item():.3f} .. {mass.max().item():.3f} of the mass (row 1: {mass[:, 0].min().item():.3f} .. '
                  f'{mass[:, 0].max().item():.3f}, last row: {mass[:, -1].min().item():.3f} .. {mass[:, -1].max().item():.3f}); its score {s[:, 1:, 0].min().item():.1f} .. '
                  f'{s[:, 1:, 0].max().item():.1f}')
            assert 0.5 <= mass.min().item() and mass.max().item() <= 0.99
    # ... and behind the longest context of the device test: the last 8 rows of the 4200-row prefix it builds and of a 700-row step behind it
    tail = LS.tail_scores_fp32(w, cfg, torch.cat([LS.prefix_embeds(cfg, 4200), LS.stress_embeds(cfg, 700, False, LS.STEP_SEED + 8000 + 700)]), 708)
    for i, s in enumerate(tail):
        mass = torch.softmax(s.double(), -1)[:, :, 0]
        for name, part in (('4192 .. 4199', mass[:, :8]), ('4892 .. 4899', mass[:, -8:]), ('4192 .. 4899', mass)):
            print(f'sink: layer {i}: rows {name}: key 0 takes {part.min().item():.3f} .. {part.max().item():.3f} of the mass')
        assert 0.5 <= mass.min().item() and mass.max().item() <= 0.99
    # the rotation of the sink's pairs over the longest context of the device test
    assert LS.inv_freq(cfg)[LS.SINK_PAIRS[0]].item() * 4300 < 0.011


def _qk_bias_scores_span_100_both_ways_and_the_maximum_moves(w, cfg, runs):
    nh = cfg.num_attention_heads
    for i in range(cfg.num_hidden_layers):
        p = f'model.layers.{i}.self_attn.'
        for b, lo in ((w[p + 'q_proj.bias'], LS.QKB_Q), (w[p + 'k_proj.bias'], LS.QKB_K)):
            big = b.float().abs() >= 50
            assert 4 <= int(big.sum()) <= 64 and b.float().abs().max().item() <= 300          # a few dimensions at 50 .. 300
    x, tr = runs[1100]
    for i, s in enumerate(tr['scores']):
        row = s[:, 1000]                                   # a query behind a 1000-key context: keys 0 .. 1000
        top = row.argmax(-1)
        print(f'qk_bias: layer {i}: scores {row[:, :1001].min().item():.0f} .. {row.max().item():.0f}; key of the maximum per head {top.tolist()}')
        assert (row.max(-1).values >= 100).all() and (row[:, :1001].min(-1).values <= -100).all()          # every head spans +-100
        # the maximum of at least one head sits in the last key split however the 1000 keys are split (the last 64-key tile), of another head in the first half, and
        # the heads of one group put it in at least four different 64-key tiles
        assert (top >= 1001 - 64).any() and (top < 500).any()
        assert len({int(t) // 64 for t in top[:nh // cfg.num_key_value_heads]}) >= 4
        # a function of the distance: A cos(phase + w D) with A = QKB_Q QKB_K / sqrt(d) = 265, up to the random parts of q and k against the other side's bias
        # (0.7 x 50 / 11.3 and 0.7 x 60 / 11.3 per element: a standard deviation of ~ 5, 4.5 of them over 28 000 scores)
        rep = nh // cfg.num_key_value_heads
        dist = (1000 - torch.arange(1001)).double()
        for h in range(nh):
            om = LS.inv_freq(cfg)[LS.QKB_PAIRS[h // rep]]
            model = LS.QKB_Q * LS.QKB_K / math.sqrt(cfg.head_dim) * torch.cos(2 * math.pi * (h % rep) / rep + om * dist)
            assert (row[h, :1001].double() - model).abs().max().item() <= 40, h
    x, tr = runs[330]
    for s in tr['scores']:
        assert s[:, -1].max().item() >= 100 and s[:, -1].min().item() <= -100


def _outlier_channels_carry_hundreds_on_every_token(w, cfg, runs):
    pattern = 'outlier_channels'
    ch = list(LS.OUTLIER_CH)
    rest = LS.channel_groups(cfg.hidden_size, LS.outlier_channels_of(pattern))['other_channels']
    for S, (x, tr) in runs.items():
        for h in tr['mid'] + tr['h'][1:]:          # from the first attention sublayer on
            print(f'outlier_channels: {S} rows: |h| on the channels {h[:, ch].abs().min().item():.0f} .. {h[:, ch].abs().max().item():.0f}, elsewhere <= {h[:, rest].abs().max().item():.1f}')
            assert 1e2 <= h[:, ch].abs().min().item() and h[:, ch].abs().max().item() <= 1e3
            assert h[:, rest].abs().max().item() < 30
    for k in LS.decoder_names(w):
        if 'norm' in k:
            assert all(5 <= w[k][c].item() <= 20 for c in ch), k


def _swiglu_gates_reach_6_to_50_on_both_signs(w, cfg, runs):
    for S, (x, tr) in runs.items():
        for gate, up in zip(tr['gate'], tr['up']):
            mx, mn = gate.amax(0), gate.amin(0)
            print(f'swiglu_saturation: {S} rows: columns reaching >= 6: {int((mx >= 6).sum())}, <= -6: {int((mn <= -6).sum())}, max|gate| {gate.abs().max().item():.1f}, '
                  f'max|up| {up.abs().max().item():.1f}, rms up {up.pow(2).mean().sqrt().item():.2f}')
            assert int(((mx >= 6) & (mn <= -6)).sum()) >= 256 and gate.abs().max().item() <= 50
            assert up.abs().max().item() < 6 and 0.2 < up.pow(2).mean().sqrt().item() < 2          # `up` O(1)
            benign = torch.maximum(mx, -mn) < 6
            assert int(benign.sum()) >= cfg.intermediate_size - LS.SAT_COLS - 64          # the other columns stay below 6


PROPERTY = {'sink': _sink_key_0_takes_half_to_99_percent_of_every_later_rows_mass, 'qk_bias': _qk_bias_scores_span_100_both_ways_and_the_maximum_moves,
            'outlier_channels': _outlier_channels_carry_hundreds_on_every_token, 'swiglu_saturation': _swiglu_gates_reach_6_to_50_on_both_signs}


def test_the_pattern_shows_the_statistic_it_is_named_for(case):
    pattern, w, cfg, runs = case
    PROPERTY[pattern](w, cfg, runs)
    assert set(PROPERTY) == set(LS.PATTERNS)
