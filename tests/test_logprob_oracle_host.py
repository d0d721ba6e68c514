"""tests/logprob_oracle.py against torch.log_softmax in float64 and against the sampling oracle's own intervals (no GPU)."""
import numpy as np
import pytest
import torch

import logprob_oracle as LO
import sampling_oracle as SO


@pytest.mark.parametrize('family', LO.FAMILIES)
@pytest.mark.parametrize('V', (1000, 257, 8, 1))
def test_logprob_is_log_softmax(family, V):
    l = LO.family_rows(family, V)[:3].double()
    want = torch.log_softmax(l, dim=-1).numpy()
    for i in range(3):
        for t in {0, V // 2, V - 1}:
            got = LO.logprob(l[i].numpy(), t)
            assert got == want[i, t] if np.isneginf(want[i, t]) else abs(got - want[i, t]) <= 1e-12
        ids, lps = LO.top_n(l[i].numpy(), 8)
        k = min(8, V)
        assert np.allclose(lps[:k], want[i, ids[:k]], rtol=0, atol=1e-12)          # (-inf equals -inf)
        assert (ids[k:] == -1).all() and np.isneginf(lps[k:]).all()
        assert (np.diff(l[i].numpy()[ids[:k]]) <= 0).all()


@pytest.mark.parametrize('params', ((1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, 0.9), (1.3, 20, 0.5), (1.0, 1, 1.0)), ids=str)
def test_sampling_logprob_is_the_log_of_the_draw_interval(params):
    T, top_k, top_p = params
    for family in ('randn4', 'ties', 'neginf'):
        l = LO.family_rows(family, 1000)[1].numpy()
        z = SO.scores(l, [0, 999, 3, 3, 0], 1.3, T)
        keep = SO.analyse(z, top_k, top_p)[2]
        for t in np.flatnonzero(keep & np.isfinite(z))[:5]:
            lo, hi, w = SO.draw_interval(z, keep, t)
            assert LO.sampling_logprob(z, keep, t) == pytest.approx(np.log(hi - lo), abs=1e-9)
        # greedy: everything kept at T = 1
        lp, slp, _, _ = LO.record(l, 5, [0, 999, 3, 3, 0], 1.3, greedy=True)
        zg = SO.scores(l, [0, 999, 3, 3, 0], 1.3)
        assert slp == pytest.approx(torch.log_softmax(torch.from_numpy(zg), 0)[5].item(), abs=1e-12)
        assert lp == pytest.approx(torch.log_softmax(torch.from_numpy(l).double(), 0)[5].item(), abs=1e-12)


def test_top_n_order_on_ties_and_short_rows():
    l = np.array([1.0, 3.0, 3.0, -np.inf, 3.0, 0.0, -0.0, 1.0], dtype=np.float32)
    ids, lps = LO.top_n(l, 8)
    assert ids.tolist() == [1, 2, 4, 0, 7, 5, 6, 3]          # equal values in index order (0.0 == -0.0), -inf last
    assert np.isneginf(lps[-1]) and np.isfinite(lps[:-1]).all()
    assert LO.top_n(l, 3)[0].tolist() == [1, 2, 4] and LO.top_n(l, 0)[0].tolist() == []
    ids, lps = LO.top_n(np.full(5, 0.7), 8)
    assert ids.tolist() == [0, 1, 2, 3, 4, -1, -1, -1] and np.allclose(lps[:5], -np.log(5)) and np.isneginf(lps[5:]).all()
    big = LO.family_rows('ties', 152064)[0].numpy()
    want = sorted(range(len(big)), key=lambda i: (-big[i], i))[:8]
    assert LO.top_n(big, 8)[0].tolist() == want


def test_single_entry_vocabulary_and_nan():
    lp, slp, ids, lps = LO.record(np.array([-3.5]), 0, [0], 1.3, temperature=0.7, top_k=5, top_p=0.5, n_top=2)
    assert lp == 0.0 and slp == 0.0 and ids.tolist() == [0, -1] and lps[0] == 0.0 and np.isneginf(lps[1])
    l = np.array([0.5, np.nan, 1.0])
    assert np.isnan(LO.logprob(l, 0)) and LO.top_n(l, 3)[0].tolist() == [2, 0, -1]
    assert LO.bound(-10.0) == 5e-6 + 10 * 2.0 ** -21
