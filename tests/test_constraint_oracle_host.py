"""Host side of constrained decoding: tests/constraint_oracle.py pinned against the installed `transformers` logits processors, the merging rules of
mmduet_amd/constraints.py, the refusals that remain, and the new symbols.  No GPU."""
import math

import numpy as np
import pytest
import torch

import constraint_oracle as CO
import logprob_oracle as LO
from mmduet_amd import constraints as CS

PREV = lambda V: [0, V - 1, 3 % V, 3 % V, 0]          # duplicates, both ends of the row (as tests/test_gpu_sampling.py)


def hf_chain(l, V, args, step, prev, pen, T):
    """HF's processors in the order of generation/utils.py::_get_logits_processor on rows l [n, V]; the penalty list stands in for input_ids."""
    from transformers.generation.logits_process import (SequenceBiasLogitsProcessor, RepetitionPenaltyLogitsProcessor, NoBadWordsLogitsProcessor,
                                                        MinNewTokensLengthLogitsProcessor, SuppressTokensLogitsProcessor, TemperatureLogitsWarper)
    n = l.shape[0]
    ids = torch.tensor([prev] * n, dtype=torch.long)
    s = l.clone()
    if args.get('sequence_bias'):
        s = SequenceBiasLogitsProcessor(sequence_bias=dict(args['sequence_bias']))(ids, s)
    if pen:
        s = RepetitionPenaltyLogitsProcessor(penalty=pen)(ids, s)
    eos = args.get('eos_token_id') or []
    if args.get('bad_words_ids'):
        s = NoBadWordsLogitsProcessor(args['bad_words_ids'], eos_token_id=eos or None)(ids, s)
    if args.get('min_new_tokens') and eos:
        s = MinNewTokensLengthLogitsProcessor(len(prev) - step, args['min_new_tokens'], eos, device='cpu')(ids, s)
    if args.get('suppress_tokens'):
        s = SuppressTokensLogitsProcessor(args['suppress_tokens'], device='cpu')(ids, s)
    if T != 1.0:
        s = TemperatureLogitsWarper(T)(ids, s)
    return s


@pytest.mark.parametrize('V', (1000, 257, 8))
@pytest.mark.parametrize('family', LO.FAMILIES)
def test_oracle_equals_hf_processors(V, family):
    pytest.importorskip('transformers')
    rows = LO.family_rows(family, V)
    for row in range(10):
        l = rows[row:row + 1]
        args, step = CO.table_for(V, row, l[0].numpy())
        if row % 10 == 3 and args['suppress_tokens']:          # the same suppression through bad_words_ids, for NoBadWordsLogitsProcessor
            args = dict(args, bad_words_ids=[[t] for t in args['suppress_tokens']], suppress_tokens=[])
        cons = CS.merge(V, **args)
        for pen, T in ((None, 1.0), (1.3, 0.7)):
            want = hf_chain(l, V, args, step, PREV(V), pen, T)
            got = CO.scores32(l, cons, step, PREV(V), pen, T)
            want = torch.where(want == 0, torch.zeros_like(want), want)
            assert torch.equal(torch.isneginf(got), torch.isneginf(want)), (row, pen)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (row, pen, (got != want).nonzero()[:4])
            # the float64 statement agrees with the fp32 one to fp32 rounding: three operations of 2^-24 each, the add's relative to |l| + |b| (it may cancel)
            z64 = CO.scores(l[0].numpy(), cons, step, PREV(V), pen, T)
            fin = np.isfinite(z64)
            assert np.array_equal(fin, np.isfinite(got[0].numpy()))
            mag = np.abs(np.where(np.isfinite(l[0].numpy()), l[0].numpy().astype(np.float64), 0.0))
            mag[list(cons.ids)] += np.abs(np.where(np.isfinite(cons.bias), cons.bias, 0.0))
            err = 4 * 2.0 ** -24 * mag * (pen or 1.0) / T
            assert (np.abs(got[0].numpy()[fin] - z64[fin]) <= err[fin]).all()


def test_mask_and_order_of_operations():
    l = np.array([2.0, -1.0, 0.5, 3.0, 1.0])
    cons = CS.merge(5, eos_token_id=[3, 4], min_new_tokens=2, suppress_tokens=[2], sequence_bias={(0,): -3.0, (1,): 4.0})
    z = CO.scores(l, cons, step=1, prev_ids=[0, 0, 1], penalty=2.0, temperature=0.5)
    assert np.array_equal(z, np.array([(2.0 - 3.0) * 2.0, (-1.0 + 4.0) / 2.0, -np.inf, -np.inf, -np.inf]) / 0.5)          # the penalty sees l + b, once per id
    z = CO.scores(l, cons, step=2, prev_ids=[0, 0, 1], penalty=2.0, temperature=0.5)
    assert np.array_equal(z, np.array([-2.0, 1.5, -np.inf, 3.0, 1.0]) / 0.5)          # step == min_new: EOS is allowed again


def test_merge_rules():
    c = CS.merge(100, [3, 3, 4], 2, [7, 9, 7], [[9], [11]], {(7,): 2.0, (12,): -1.5, (13,): -math.inf})
    assert c.eos == (3, 4) and c.min_new == 2 and c.ids == (7, 9, 11, 12, 13)
    assert c.bias == (-math.inf, -math.inf, -math.inf, -1.5, -math.inf) and c.on          # biased + suppressed = suppressed
    assert CS.merge(100, None, None, [], None, [[[5], 1.0], [[5], 2.0]]).bias == (2.0,)          # list-of-pairs form; the later entry replaces
    assert CS.merge(100, 7).eos == (7,) and not CS.merge(100).on and not CS.OFF.on
    assert CS.merge(100, None, 3).on


def test_merge_limits():
    with pytest.raises(ValueError):
        CS.merge(1000, list(range(9)))
    assert len(CS.merge(1000, list(range(8))).eos) == 8
    with pytest.raises(ValueError):
        CS.merge(1000, suppress_tokens=list(range(257)))
    assert len(CS.merge(1000, suppress_tokens=list(range(256))).ids) == 256
    with pytest.raises(ValueError):
        CS.merge(1000, suppress_tokens=list(range(200)), sequence_bias={(i,): 1.0 for i in range(200, 257)})          # 257 after merging
    for bad in (math.nan, math.inf):
        with pytest.raises(ValueError):
            CS.merge(1000, sequence_bias={(1,): bad})
    for tok in (-1, 1000):
        with pytest.raises(ValueError):
            CS.merge(1000, suppress_tokens=[tok])
        with pytest.raises(ValueError):
            CS.merge(1000, [tok])
    with pytest.raises(ValueError):
        CS.merge(1000, min_new_tokens=-1)
    with pytest.raises(ValueError):
        CS.merge(8, [7], suppress_tokens=list(range(7)))          # suppressed + EOS cover the vocabulary
    assert CS.merge(8, [6], suppress_tokens=list(range(7))).on          # (EOS already suppressed: id 7 is left)
    for kw in (dict(bad_words_ids=[[1, 2]]), dict(sequence_bias={(1, 2): 1.0})):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            CS.merge(1000, **kw)


def test_generate_refusals_that_remain():
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM as M, _GENERATE_OFF

    class Cfg:
        vocab_size, eos_token_id = 100, 5
    m = object.__new__(M)          # the argument checks come before anything touches the device
    m.config = Cfg()
    ids = torch.zeros(1, 2, dtype=torch.long)
    for kw in (dict(no_repeat_ngram_size=2), dict(min_length=3), dict(forced_eos_token_id=1), dict(stopping_criteria=[1]), dict(output_scores=True), dict(num_beams=2),
               dict(bad_words_ids=[[1, 2]]), dict(sequence_bias={(1, 2): 1.0})):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            M.generate(m, input_ids=ids, **kw)
    with pytest.raises(ValueError):
        M.generate(m, input_ids=ids, eos_token_id=list(range(9)))
    assert not {'min_new_tokens', 'sequence_bias', 'bad_words_ids', 'suppress_tokens'} & set(_GENERATE_OFF)


def test_new_symbols_are_bound():
    from mmduet_amd import _lib
    names = ('mmd_set_generate_constraints', 'mmd_sampler_set_constraints', 'mmd_op_sample_constrained')
    assert all(n in _lib.EXPORTED_SYMBOLS for n in names)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names)
