"""CPU restatement of the constrained score (DESIGN.md "Constraints"), built on tests/sampling_oracle.py:

    z_i = mask_i(pen(l_i + b_i)) / T

b: the bias table (0 for ids it does not hold, -inf = suppressed); pen: the repetition penalty, once per id, on l + b; mask = -inf for a suppressed id and, while fewer than
min_new tokens have been returned (`step` < min_new), for the EOS ids.  `scores` is float64 and literal; `scores32` evaluates the same operations in torch fp32, in the
order HF's processors apply them (sequence bias, repetition penalty, bad words / min-new-tokens / suppress, temperature), and is what the host test pins against the
installed `transformers` bit for bit and what the device's scores are held against.

`table_for(V, row, family_row)` builds the tables the GPU tests use: the places where a kernel that scatters into column slices can go wrong.
"""
import numpy as np
import torch

import sampling_oracle as SO

NEG_INF = -float('inf')


def scores(logits, cons, step=0, prev_ids=None, penalty=None, temperature=1.0):
    """cons: anything with .eos, .min_new, .ids, .bias (mmduet_amd.constraints.Constraints).  float64."""
    l = np.asarray(logits, dtype=np.float64).copy()
    ids, bias = np.asarray(cons.ids, dtype=np.int64), np.asarray(cons.bias, dtype=np.float64)
    fin = np.isfinite(bias)
    l[ids[fin]] += bias[fin]
    z = SO.scores(l, prev_ids, penalty, 1.0)
    z[ids[~fin]] = NEG_INF
    if step < cons.min_new and len(cons.eos):
        z[np.asarray(cons.eos, dtype=np.int64)] = NEG_INF
    return z / temperature


def scores32(logits, cons, step=0, prev_ids=None, penalty=None, temperature=1.0):
    """The same in torch fp32, operation for operation: [V] or [n, V] fp32 in, the same shape out."""
    z = logits.clone().float()
    ids, bias = torch.tensor(list(cons.ids), dtype=torch.long), torch.tensor(list(cons.bias), dtype=torch.float32)
    fin = torch.isfinite(bias)
    z[..., ids[fin]] = z[..., ids[fin]] + bias[fin]
    if penalty and prev_ids is not None and len(prev_ids):
        p = torch.tensor(sorted(set(int(t) for t in prev_ids)), dtype=torch.long)
        z[..., p] = torch.where(z[..., p] > 0, z[..., p] / penalty, z[..., p] * penalty)
    z[..., ids[~fin]] = NEG_INF
    if step < cons.min_new and len(cons.eos):
        z[..., torch.tensor(list(cons.eos), dtype=torch.long)] = NEG_INF
    z = z / temperature
    return torch.where(z == 0, torch.zeros_like(z), z)          # -0 canonicalised, as the chain does


def slices(V):
    """The column slices of the sampling chain: (count, columns per slice) -- sample_topkp_slices / slice_of of csrc/sample.hip."""
    n = min(64, max(1, -(-V // 256)))
    return n, -(-V // n)


def table_for(V, row, l):
    """-> (dict of generate-style arguments for constraints.merge, step) for row `row` of a batch with logits l [V] (numpy).  Ten kinds, cycled over the rows:
    0 ids 0 and V - 1 biased | 1 the first and last column of a middle slice, one biased one suppressed | 2 an id of the penalty list (3 % V, listed twice there) biased |
    3 -inf on the raw arg-max | 4 a positive bias that lifts a non-maximal finite id over the maximum | 5 the raw arg-max is an EOS id, step < min_new | 6 the same at
    step == min_new (allowed again) | 7 every id but one suppressed | 8 a 256-entry table | 9 nothing (an unconstrained row among constrained ones)."""
    kind = row % 10
    am = int(np.argmax(np.where(np.isnan(l), -np.inf, l)))
    n_sl, per = slices(V)
    sb, sup, eos, min_new, step = {}, [], [], 0, 0
    if kind == 0:
        sb = {(0,): 1.5, (V - 1,): -2.25}
    elif kind == 1:
        s = n_sl // 2
        beg, end = min(V, s * per), min(V, s * per + per)
        sb = {(beg,): 3.0}
        sup = [end - 1] if end - 1 != beg else []
    elif kind == 2:
        sb = {(3 % V,): 2.0}
    elif kind == 3:
        sup = [am] if V > 1 else []
    elif kind == 4:
        fin = np.flatnonzero(np.isfinite(l))
        other = int(fin[fin != am][0]) if len(fin[fin != am]) else am
        sb = {(other,): float(abs(l[am] - l[other]) + 50.0)}
    elif kind in (5, 6):
        eos, min_new = ([am, (am + 1) % V] if V > 2 else [am]) if V > 1 else [], 3
        step = 2 if kind == 5 else 3
    elif kind == 7:
        keep = int(np.flatnonzero(np.isfinite(l))[-1])
        sup = [i for i in range(V) if i != keep][:256] if V <= 257 else []
        if V == 257:
            sup = sup[:255]          # (256 entries at most; 255 suppressed of 257 leaves two)
    elif kind == 8:
        g = np.random.default_rng(V + row)
        pick = g.choice(V, size=min(256, V - 1), replace=False) if V > 1 else []
        sb = {(int(i),): float(b) for i, b in zip(pick, g.normal(size=len(pick)) * 3)}
    return dict(eos_token_id=eos or None, min_new_tokens=min_new, suppress_tokens=sup, sequence_bias=sb or None), step
