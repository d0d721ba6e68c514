"""The stress builders of tests/stress_inputs.py really build what their names claim, checked in float64 on the host at reduced sizes -- so the GPU stress
suites cannot silently turn benign when someone retunes a constant -- and the element-wise GEMM bound closes the gap it was written for: it passes a
correct bf16 product of the outlier operands and fails one that dropped the K - 6 non-outlier channels, which the old max-norm bound lets through."""
import math
import pytest
import torch
import stress_inputs as SI
from parity_common import ref_attention, ref_attention_rows

SHAPES = [(33, 4, 2, 32, 500), (49, 7, 1, 128, 4047), (2, 7, 1, 128, 1000)]          # S, nh, nkv, d, n_ctx
ATTN_BOUND = 1.8e-2                                                                    # of the GPU stress tests: max|o - ref| <= 1.8e-2 max(1, max|ref|)


def _scores(c, nh, nkv, d, causal=True):
    """float64 scaled scores [nh, S, n_tot] of the valid keys, masked ones at -inf"""
    S = c.q.shape[0]; n_tot = c.n_ctx + S; rep = nh // nkv
    qh = c.q.double().view(S, nh, d).transpose(0, 1)
    kk = c.K[:, :n_tot].double().repeat_interleave(rep, 0)
    s = qh @ kk.transpose(1, 2) * d ** -0.5
    if causal:
        mask = torch.arange(n_tot)[None, :] > (torch.arange(S)[:, None] + c.n_ctx)
        s = s.masked_fill(mask[None], float('-inf'))
    return s


def _entropy(s):
    p = torch.softmax(s, -1)
    return -(p * torch.log(p.clamp_min(1e-300))).sum(-1)


@pytest.mark.parametrize('S,nh,nkv,d,n_ctx', SHAPES)
@pytest.mark.parametrize('name', ['sink', 'last_hot', 'first_row_only'])
def test_one_hot_patterns_put_one_key_40_above_the_rest(name, S, nh, nkv, d, n_ctx):
    c = SI.ATTN_PATTERNS[name](S, nh, nkv, d, n_ctx, seed=S + n_ctx)
    s = _scores(c, nh, nkv, d)
    hot = s[:, :, c.hot]
    rest = s.clone(); rest[:, :, c.hot] = float('-inf')
    gap = hot - rest.amax(-1)                                    # (a row that sees the hot key alone: +inf)
    assert c.hot == (max(c.n_ctx - 1, 0) if name == 'last_hot' else 0)
    assert (c.n_ctx == 0) == (name == 'first_row_only' or n_ctx == 0)
    assert gap.min().item() >= 40.0, gap.min().item()
    assert _entropy(s).max().item() < 0.1
    # ... so the exact result of every row is the hot key's V row
    ref = ref_attention(c.q, c.K, c.V, nh, nkv, d, c.n_ctx, torch.float64).view(S, nh, d)
    want = c.V[:, c.hot].double().repeat_interleave(nh // nkv, 0)[None]
    assert (ref - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize('S,nh,nkv,d,n_ctx', SHAPES)
def test_rising_raises_the_max_on_every_key_tile(S, nh, nkv, d, n_ctx):
    c = SI.rising(S, nh, nkv, d, n_ctx, seed=S)
    s = _scores(c, nh, nkv, d, causal=False)
    n = s.shape[-1] // 64 * 64
    tile_max = s[:, :, :n].reshape(nh, S, -1, 64).amax(-1)
    assert tile_max.shape[-1] >= 8 and (tile_max[:, :, 1:] > tile_max[:, :, :-1]).all()
    assert s.amax().item() >= 350.0


def test_rising_steps_sit_on_both_sides_of_the_deferred_rescale():
    """ATTN_DEFER is 4 in the exp2 domain (2.77 in nats): ~6 per 64-key tile at n = 4096, ~0.4 at n = 70 000"""
    for n_tot, lo, hi in ((4096, 5.0, 8.0), (70000, 0.2, 0.6)):
        step = 400.0 * 64 / n_tot
        assert lo <= step <= hi
    assert 400.0 * 64 / 4096 > 4.0 / math.log2(math.e) > 400.0 * 64 / 70000


@pytest.mark.parametrize('S,nh,nkv,d,n_ctx', SHAPES)
def test_huge_scores_are_in_the_thousands_and_rows_one_hot(S, nh, nkv, d, n_ctx):
    c = SI.huge(S, nh, nkv, d, n_ctx, seed=S)
    s = _scores(c, nh, nkv, d)
    assert s[torch.isfinite(s)].abs().max().item() >= 1000.0
    # one-hot rows: the top two of n scores of standard deviation ~900 are ~200 apart; a row whose top two fall within 3 of each other (P ~ 1.5 %) is two-hot
    ent = _entropy(s)
    assert (ent < 0.1).double().mean().item() >= 0.95 and ent.median().item() < 1e-6


def test_outlier_dims_scores_come_from_three_huge_products():
    S, nh, nkv, d, n_ctx = 49, 7, 1, 128, 4047
    c = SI.outlier_dims(S, nh, nkv, d, n_ctx, seed=3)
    s = _scores(c, nh, nkv, d, causal=False)
    ch = SI.outlier_channels(d)
    qo = c.q.double().view(S, nh, d)[:, :, ch]; ko = c.K[0, :n_ctx + S][:, ch].double()
    part = torch.einsum('shc,nc->hsn', qo, ko) * d ** -0.5
    assert len(set(ch)) == 3 and qo.abs().amin().item() > 200
    assert s.abs().max().item() >= 100.0
    assert (s - part).abs().max().item() <= 8.0                  # the 125 other channels: O(1)


@pytest.mark.parametrize('name', sorted(SI.ATTN_PATTERNS))
def test_poison_sits_behind_every_valid_key_and_inputs_are_bf16_and_seeded(name):
    S, nh, nkv, d, n_ctx = 20, 4, 2, 16, 77
    a = SI.ATTN_PATTERNS[name](S, nh, nkv, d, n_ctx, seed=5); b = SI.ATTN_PATTERNS[name](S, nh, nkv, d, n_ctx, seed=5)
    n_tot = a.n_ctx + S
    assert a.q.dtype == a.K.dtype == a.V.dtype == torch.bfloat16 and a.K.shape[1] % 64 == 0 and a.K.shape[1] >= n_tot + 100
    assert (a.K[:, n_tot:] == 1e4).all() and (a.V[:, n_tot:] == 1e4).all() and a.V[:, :n_tot].abs().max() < 10
    assert torch.equal(a.q, b.q) and torch.equal(a.K, b.K) and torch.equal(a.V, b.V)


@pytest.mark.parametrize('name', sorted(SI.ATTN_PATTERNS))
def test_references_agree_far_inside_the_bound(name):
    """The GPU stress tests compare with ref_attention in float64.  Two float64 formulations (the full softmax, and the streamed running (max, sum) one in
    key blocks) agree to less than 1e-3 of the bound on every pattern; the float32 softmax differs from float64 by at most 4e-4 (one-hot rows over scores of
    4000: a few float32 ulps of the score) -- inside 1e-2 of the bound, which is why float32 would do and float64 removes the question."""
    S, nh, nkv, d, n_ctx = 49, 7, 1, 128, 4047
    c = SI.ATTN_PATTERNS[name](S, nh, nkv, d, n_ctx, seed=11)
    r64 = ref_attention(c.q, c.K, c.V, nh, nkv, d, c.n_ctx, torch.float64)
    rows = list(range(S))
    s64 = ref_attention_rows(c.q, c.K, c.V, nh, nkv, d, c.n_ctx, rows, torch.float64)
    r32 = ref_attention(c.q, c.K, c.V, nh, nkv, d, c.n_ctx, torch.float32)
    bound = ATTN_BOUND * max(1.0, r64.abs().max().item())
    d64 = (r64 - s64).abs().max().item(); d32 = (r32.double() - r64).abs().max().item()
    print(f'{name}: two float64 references differ by {d64:.2e}, float32 from float64 by {d32:.2e}, bound {bound:.2e}')
    assert d64 < 1e-3 * bound
    assert d32 < 1e-2 * bound


# ---- GEMM operands and the element-wise bound -------------------------------------------------------------------------------------------------------------
def test_outlier_x_has_six_channels_in_the_thousands():
    X, ch = SI.outlier_x(49, 3584, seed=2)
    Xd = X.double()
    assert X.dtype == torch.bfloat16 and len(set(ch.tolist())) == 6
    med = Xd[:, ch].abs().median(0).values
    assert all(0.7 * abs(a) <= m <= 1.3 * abs(a) for a, m in zip(SI.OUTLIER_AMPS, med.tolist()))
    assert (torch.sign(Xd[:, ch]) == torch.sign(torch.tensor(SI.OUTLIER_AMPS, dtype=torch.float64))[None]).all()
    rest = Xd.clone(); rest[:, ch] = 0
    assert rest.abs().max().item() < 5.0 and 0.6 < rest.std().item() < 0.8


@pytest.mark.parametrize('amp', [8.0, 40.0, 50.0, 120.0])
def test_saturating_reaches_its_amplitude(amp):
    X, W = SI.saturating(70, 136, 192, amp, seed=1)
    pre = X.double() @ W.double().T
    assert 0.85 * amp / 3 <= pre.std().item() <= 1.15 * amp / 3
    assert pre.max().item() >= amp and pre.min().item() <= -amp


C_ACC = SI.C_ACC


@pytest.mark.parametrize('M,N,K', [(49, 512, 3584), (49, 256, 18944), (130, 384, 1152)])
def test_elementwise_bound_passes_a_right_product_and_fails_one_without_the_small_channels(M, N, K):
    """bf16(torch's float32 product) of the outlier operands is inside |Y - ref| <= 2^-8 (|ref| + a) + a; the same product with the K - 6 non-outlier
    channels left out is outside it on a quarter of the elements or more (the dropped part has standard deviation 0.7, the tolerance a median of ~0.7) and INSIDE the old max|err| / max|ref| <= 2.4e-2 (measured at 49 x 512 x 3584: the old bound allows
    ~21 absolute on every element where the median element-wise tolerance is ~0.7)."""
    X, ch = SI.outlier_x(M, K, seed=M + K); W = SI.weights(N, K, seed=N)
    Xd, Wd = X.double(), W.double()
    ref = Xd @ Wd.T
    a = SI.acc_floor(Xd, Wd, C_ACC)
    tol = SI.rounding_tol([ref], a)
    f32 = X.float() @ W.float().T
    ratio_acc = ((f32.double() - ref).abs() / (a / C_ACC)).max().item()
    good = f32.to(torch.bfloat16)
    worst = ((good.double() - ref).abs() / tol).max().item()
    Xo = torch.zeros_like(X); Xo[:, ch] = X[:, ch]
    bad = (Xo.float() @ W.float().T).to(torch.bfloat16)
    d_bad = (bad.double() - ref).abs()
    print(f'{M}x{N}x{K}: fp32 summation error / (sqrt(K) 2^-24 A) = {ratio_acc:.3f}; bf16(fp32) worst |err| / tol = {worst:.3f}; median tol {tol.median().item():.3f}, '
          f'max|ref| {ref.abs().max().item():.1f}, old bound allows {2.4e-2 * ref.abs().max().item():.1f}; outliers-only: old measure {SI.old_max_norm_err(bad, ref):.2e}, '
          f'{(d_bad > tol).double().mean().item():.2f} of the elements outside the new bound')
    assert ratio_acc <= 1.0
    assert worst <= 1.0
    assert SI.old_max_norm_err(good, ref) <= 2.4e-2
    assert SI.old_max_norm_err(bad, ref) <= 2.4e-2                                    # the gap: the old bound is blind to it
    assert (d_bad > tol).double().mean().item() > 0.1                                 # ... the element-wise bound is not
    assert tol.median().item() < 0.1 * 2.4e-2 * ref.abs().max().item()
