"""tests/residual_stream.py on the host: the restatement of the residual stream's rounding points agrees with float64 math, its order-sensitive inputs really tell one slab
order from another, and the case lists of tests/test_gpu_residual_stream.py cover every instantiation and boundary they name."""
import pytest
import torch

import residual_stream as RS

BF = torch.bfloat16


def _ulp(x):
    """one bf16 ulp at |x| (float64 tensor)"""
    return 2.0 ** (torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


@pytest.mark.parametrize('splits', [1, 3, 8])
@pytest.mark.parametrize('with_scale', [False, True])
def test_slab_resid_is_float64_math_to_one_rounding(splits, with_scale):
    """random slabs: h is within one bf16 ulp of the float64 sum (two roundings of at most half an ulp each -- of the linear part, which is no larger than 3 ulp-widths of h
    here -- and fp32 adds far below either)"""
    g = torch.Generator().manual_seed(splits)
    slabs = torch.randn(splits, 5, 1028, generator=g) / splits ** 0.5
    resid = (3 * torch.randn(5, 1028, generator=g)).to(BF)
    ws = 2.0 ** -9 * (1 + 15 * torch.rand(1028, generator=g)) if with_scale else None
    h = RS.slab_resid(slabs, resid, ws)
    assert h.dtype == BF
    lin = slabs.double().sum(0) * (ws.double() if with_scale else 1.0)
    ref = lin + resid.double()
    err = (h.double() - ref).abs()
    assert bool((err <= 0.5 * _ulp(ref) + 0.5 * _ulp(lin) + 1e-6).all()), err.max().item()
    assert bool((err <= _ulp(ref).clamp_min(_ulp(lin))).all())


@pytest.mark.parametrize('splits', [s for s in RS.SLAB_SPLITS if s >= 3])
@pytest.mark.parametrize('with_scale', [False, True])
def test_reversed_slab_order_changes_bits(splits, with_scale):
    """what the GPU test relies on to tell a kernel that sums its slabs in another order: on the order-sensitive inputs the reversed sum gives another h"""
    slabs, resid, gamma, ws = RS.slab_inputs(splits, 3, 1024, seed=splits)
    ws = ws if with_scale else None
    fwd = RS.slab_resid(slabs, resid, ws)
    rev = RS.slab_resid(slabs, resid, ws, order=range(splits - 1, -1, -1))
    changed = int((fwd.view(torch.int16) != rev.view(torch.int16)).sum())
    assert changed > 0
    assert float(slabs.double().sum(0).abs().max()) < 50          # the large terms cancel: h is O(1), not 1e4
    # ... and the scale's place too: applied after the first rounding it gives another h
    if with_scale:
        late = ((slabs.sum(0) if splits == 1 else sum(slabs[s] for s in range(splits))).to(BF).float() * ws).to(BF)
        late = (late.float() + resid.float()).to(BF)
        assert int((late.view(torch.int16) != fwd.view(torch.int16)).sum()) > 0


def test_stress_rows_and_the_norm_rule():
    slabs, resid, gamma, ws = RS.slab_inputs(5, 3, 3584, seed=1)
    h = RS.slab_resid(slabs, resid)
    assert float(h[1].float().abs().max()) >= 9e3 and bool((h[2] == 0).all())
    ref, tol = RS.rms_image(h, gamma, 1e-6)
    assert bool((ref[2] == 0).all()) and torch.isfinite(ref).all()
    # the rule accepts the plain fp32 evaluation of the same formula, and refuses one with another row's 1/rms
    hf = h.float()
    inv = torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + 1e-6)
    y = (gamma.float() * (hf * inv).to(BF).float()).to(BF)
    assert RS.rms_image_excess(y, h, gamma, 1e-6).max().item() <= 0
    y0 = (gamma.float() * (hf * inv[0:1]).to(BF).float()).to(BF)
    assert RS.rms_image_excess(y0, h, gamma, 1e-6)[1].max().item() > 0
    # ties are rare and flagged
    assert 0 <= int(RS.rms_ties(h, gamma, 1e-6).sum()) < h.numel() // 100


def test_tile_ssq_and_consumer_rows():
    h, gamma = RS.chain_h(4, 96, seed=0)
    q = RS.tile_ssq(h)
    assert q.shape == (4, 6) and q.dtype == torch.float32
    assert torch.allclose(q.double().sum(-1), h.double().pow(2).sum(-1), rtol=1e-6)
    rms = h.double().pow(2).mean(-1).sqrt()
    assert bool((rms[1:] / rms[:-1] >= 25).all())          # a 1/rms from the wrong row is off by ~30 x or more


def test_case_lists_cover_what_they_name():
    # slab consumer: both sides of the instantiation boundaries, and the top
    assert {4, 5, 8, 9, 16, 1} <= set(RS.SLAB_SPLITS) and set(RS.SLAB_MAXS.values()) == {4, 8, 16}
    assert all(RS.SLAB_MAXS[s] == (4 if s <= 4 else 8 if s <= 8 else 16) for s in RS.SLAB_SPLITS)
    assert {1, 3, 64} == set(RS.SLAB_MS)
    hs = set(RS.SLAB_HS)
    assert any(h < 1024 for h in hs) and {1024, 1028, 3584, 4096} <= hs and all(h % 4 == 0 and h <= 4096 for h in hs)
    assert dict(splits=17) in RS.SLAB_REFUSED and dict(H=4100) in RS.SLAB_REFUSED and dict(H=70) in RS.SLAB_REFUSED
    # producer
    shapes = {(c[1], c[2], c[3]) for c in RS.PRODUCER_CASES}
    assert {(3584, 3584, False), (3584, 3584, True), (3584, 18944, False), (3584, 18944, True), (4096, 64, False), (16, 2048, False)} == shapes
    assert set(RS.PRODUCER_MS) == {1, 2, 4}
    assert all(N <= 16 * RS.SSQ_STRIDE for N, _, _ in shapes) and any(N == 16 * RS.SSQ_STRIDE for N, _, _ in shapes)
    # consumer: both forms, both split counts, the three bands of a wave's K range, a ragged range, fp8 at the true widths
    assert set(RS.CONSUMER_MS) == {1, 3, 4} and max(RS.CONSUMER_MS) == RS.CHAIN_ROWS
    got = {(epi, N, K) for _, epi, N, K, _, _ in RS.CONSUMER_CASES}
    assert {('none', 4608, 3584), ('none', 512, 4096), ('none', 16, 96), ('swiglu', 37888, 3584), ('swiglu', 64, 4096), ('swiglu', 32, 1056)} == got
    assert {(epi, N, K) for _, epi, N, K, fp8, _ in RS.CONSUMER_CASES if fp8} == {('none', 4608, 3584), ('swiglu', 37888, 3584)}
    for (name, epi, N, K, fp8, room), (splits, kw, rag) in RS.CONSUMER_CASES.items():
        assert RS.wave_k(K, splits, fp8) == kw and RS.ragged(K, splits, fp8) == rag and kw <= 1024, name
        assert epi == 'none' or splits == 1, name
    plans = list(RS.CONSUMER_CASES.values())
    assert {s for s, _, _ in plans} == {1, 2}
    assert {s for (_, epi, *_), (s, _, _) in RS.CONSUMER_CASES.items() if epi == 'none'} == {1, 2}
    kws = [kw for _, kw, _ in plans]
    assert any(kw < 512 for kw in kws) and any(512 < kw < 1024 for kw in kws) and any(kw == 1024 for kw in kws) and any(kw == 512 for kw in kws)
    assert any(rag for _, _, rag in plans)
    # refusals: one step past each bound the planner holds
    assert RS.CHAIN_REFUSED['consumer_m5'][1] == RS.CHAIN_ROWS + 1
    _, _, _, K, room = RS.CHAIN_REFUSED['consumer_k8192_one_split']
    assert room == 1 and RS.wave_k(K, 1, False) > 1024
    assert RS.CHAIN_REFUSED['producer_n4112'][2] == 16 * RS.SSQ_STRIDE + 16
