"""CPU restatement of the log-probability contract (DESIGN.md "Log-probabilities"), float64 and literal, plus the input families the GPU tests draw their rows from.

For the token t a step ended with, l the step's fp32 logits:
  logprob          = l[t] - logsumexp(l)                                   the model's log-probability
  sampling_logprob = z[t] - logsumexp_{j kept} z[j]                        z = pen(l) / T and the kept set as tests/sampling_oracle.py states them
                                                                           (arg-max path: T = 1, everything kept)
  top_n            = the top_n largest l, by (value descending, index ascending), as ids and logprobs; id -1 and -inf where the row is shorter
logsumexp subtracts the maximum; -inf entries have mass 0; a NaN anywhere in the row gives NaN.
"""
import numpy as np
import torch

import sampling_oracle as SO

FAMILIES = ('randn', 'randn4', 'equal', 'spike', 'ties', 'neginf')
VS = (152064, 1000, 257, 8, 1)
_rows = {}


def family_rows(family, V):
    """32 rows [32, V] fp32 of one input family (built once per process; callers slice the first n rows and never write to them)."""
    if (family, V) not in _rows:
        g = torch.Generator().manual_seed(VS.index(V) * 16 + FAMILIES.index(family))
        x = torch.randn(32, V, generator=g)
        if family == 'randn4':
            x = x * 4
        elif family == 'equal':
            x = torch.full((32, V), 0.7)
        elif family == 'spike':
            x[torch.arange(32), torch.randint(0, V, (32,), generator=g)] += 80.0
        elif family == 'ties':
            x = torch.round(x * 2)
        elif family == 'neginf':
            x[torch.rand(32, V, generator=g) < 0.1] = -float('inf')
            x[:, V // 2] = 0.25          # (never a row without a finite entry)
        _rows[(family, V)] = x
    return _rows[(family, V)]


def logsumexp(x, keep=None):
    """max + log(sum exp(x - max)) over `keep` (all of x if None); -inf entries add nothing; NaN in x -> NaN."""
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).any():
        return np.nan
    if keep is not None:
        x = x[np.asarray(keep, bool)]
    m = x.max()
    if not np.isfinite(m):
        return m
    with np.errstate(invalid='ignore'):
        return m + np.log(np.where(np.isneginf(x), 0.0, np.exp(x - m)).sum())


def logprob(l, token):
    l = np.asarray(l, dtype=np.float64)
    return l[token] - logsumexp(l)


def sampling_logprob(z, keep, token):
    z = np.asarray(z, dtype=np.float64)
    return z[token] - logsumexp(z, keep)


def top_order(l, n):
    """The first n indices of the order (value descending, index ascending); NaN entries never appear."""
    l = np.asarray(l, dtype=np.float64)
    idx = np.flatnonzero(~np.isnan(l))
    if len(idx) > n > 0:          # (only the entries that can make it: everything at or above the n-th largest value)
        kth = np.partition(l[idx], len(idx) - n)[len(idx) - n]
        idx = idx[l[idx] >= kth]
    order = idx[np.lexsort((idx, -l[idx]))]          # last key first: value descending, then index ascending
    return order[:n]


def top_n(l, n):
    """-> (ids int64 [n], logprobs float64 [n]), padded with -1 / -inf."""
    l = np.asarray(l, dtype=np.float64)
    ids = np.full(n, -1, dtype=np.int64)
    lps = np.full(n, -np.inf)
    o = top_order(l, n)
    ids[:len(o)] = o
    with np.errstate(invalid='ignore'):
        lps[:len(o)] = l[o] - logsumexp(l)
    return ids, lps


def record(l, token, prev_ids=None, penalty=None, temperature=1.0, top_k=0, top_p=1.0, n_top=0, greedy=False):
    """The whole record of one step from its logits: (logprob, sampling_logprob, top ids, top logprobs)."""
    z = SO.scores(l, prev_ids, penalty, 1.0 if greedy else temperature)
    keep = np.ones(len(z), bool) if greedy else SO.analyse(z, top_k, top_p)[2]
    ids, lps = top_n(l, n_top)
    return logprob(l, token), sampling_logprob(z, keep, token), ids, lps


def bound(lp):
    """The device's error bound on a log-probability: fp32 exp (~2 ulp), fixed-point truncation (<= V 2^-40 ~ 1.4e-7), one log, two subtractions that scale with |lp|."""
    return 5e-6 + 2.0 ** -21 * np.abs(lp)
