"""The plain greedy arg-max without a GPU: tests/greedy_oracle.py against transformers' RepetitionPenaltyLogitsProcessor followed by torch.argmax on fp32 CPU tensors (scores
bit for bit, tokens equal) on every row of tests/test_gpu_greedy.py that the processor can be asked (no NaN, every listed id in range), the NaN rule, the state advance, and
the comparison rule of the kernels restated next to the one it replaced."""
import numpy as np
import pytest
import torch
import greedy_oracle as GO


def hf_scores(row, prev, penalty):
    from transformers import RepetitionPenaltyLogitsProcessor
    if penalty is None or penalty <= 0:
        return row.clone()
    ids = torch.tensor([prev], dtype=torch.long).reshape(1, -1)
    return RepetitionPenaltyLogitsProcessor(penalty=float(penalty))(ids, row[None].clone())[0]


@pytest.mark.parametrize('V', GO.VS)
def test_oracle_is_hf_penalty_then_torch_argmax(V):
    seen = 0
    for cs in GO.cases(V):
        if not cs.hf_expressible:
            continue
        want = hf_scores(cs.row, cs.prev, cs.penalty)
        assert want.dtype == torch.float32
        got = GO.scores(cs.row.numpy(), cs.prev, cs.penalty)
        assert np.array_equal(got.view(np.int32), want.numpy().view(np.int32)), cs.name
        tok = GO.pick(cs.row.numpy(), cs.prev, cs.penalty)
        assert tok == int(torch.argmax(want)), cs.name
        if cs.want is not None:
            assert tok == cs.want, cs.name          # and what the row was built to give
        seen += 1
    assert seen >= 20 or V < 3


@pytest.mark.parametrize('V', GO.VS)
def test_nan_gives_minus_one_exactly_where_a_raw_logit_is_nan(V):
    n_nan = 0
    for cs in GO.cases(V):
        tok = GO.pick(cs.row.numpy(), cs.prev, cs.penalty)
        assert (tok == -1) == bool(torch.isnan(cs.row).any()), cs.name
        assert tok == -1 or 0 <= tok < V
        if cs.want is not None:
            assert tok == cs.want, cs.name
        n_nan += tok == -1
    assert n_nan >= 5
    # ids outside the row are dropped, not wrapped: the out-of-range list leaves the scores alone
    cs = next(c for c in GO.cases(V) if c.name == 'list_out_of_range')
    assert np.array_equal(GO.scores(cs.row.numpy(), cs.prev, cs.penalty).view(np.int32), cs.row.numpy().view(np.int32))


def test_case_lists_cover_what_they_claim():
    names = {V: [c.name for c in GO.cases(V)] for V in GO.VS}
    for V in GO.VS:
        assert len(set(names[V])) == len(names[V])
        p = GO.per(V)
        assert all(0 <= i < j < V for i, j in GO.tie_pairs(V))
    big = GO.tie_pairs(152064)
    p = GO.per(152064)
    assert p == 2376 and GO.per(4097) == 65
    assert (0, 152063) in big and (p - 1, p) in big and (31 * p - 1, 31 * p) in big and (63 * p - 1, 63 * p) in big and (p - 1, 63 * p) in big
    assert any(j - i == 256 and i // p == j // p for i, j in big) and (63, 64) in big
    assert (63, 64) in GO.tie_pairs(4097) and (64, 65) in GO.tie_pairs(4097)          # per = 65: a wave boundary inside slice 0, and the boundary of slices 0 / 1
    assert GO.tie_pairs(2) == [(0, 1)] and GO.tie_pairs(1) == []
    assert 'list_all' in names[255] and 'list_2048' in names[152064]
    assert len(next(c for c in GO.cases(152064) if c.name == 'list_2048').prev) == 2048


def test_advance():
    s0 = dict(prev=[7, 8, -5, -5, -9], n_prev=2, n_ctx=100, step=3)          # prev_cap 4: slot 4 is the guard behind the list
    s = GO.advance(s0, 11, eos=2, use_penalty=1, prev_cap=4)
    assert s == dict(prev=[7, 8, 11, -5, -9], n_prev=3, n_ctx=101, step=4) and s0['prev'][2] == -5
    assert GO.advance(s0, 2, eos=2, use_penalty=1, prev_cap=4) == dict(prev=s0['prev'], n_prev=2, n_ctx=101, step=4)
    assert GO.advance(s0, 11, eos=2, use_penalty=0, prev_cap=4) == dict(prev=s0['prev'], n_prev=2, n_ctx=101, step=4)
    s = GO.advance(GO.advance(s, 12, 2, 1, 4), 13, 2, 1, 4)
    assert s == dict(prev=[7, 8, 11, 12, -9], n_prev=4, n_ctx=103, step=6)          # the last slot is used, then the list is full and the guard stays


@pytest.mark.parametrize('V', [v for v in GO.VS if v <= 255])
def test_comparison_rule_and_the_one_it_replaced(V):
    """The kernels' `better` folded over pen(l): with the NaN clause and the final check it gives the oracle's token on every row; the rule before this check existed gives the
    same token on every row WITHOUT a NaN and a made-up index -- never -1 -- on every row with one (so the NaN rows of tests/test_gpu_greedy.py fail against it, the others
    pass)."""
    for cs in GO.cases(V):
        z = GO.scores(cs.row.numpy(), cs.prev, cs.penalty)
        want = GO.pick(cs.row.numpy(), cs.prev, cs.penalty)
        assert GO.fold(z, GO.better_new, True) == want, cs.name
        before = GO.fold(z, GO.better_before, False)
        if cs.has_nan:
            assert before != -1 and (before == GO.INT_MAX or 0 <= before < V), cs.name
            if bool(torch.isnan(cs.row).all()):
                assert before == GO.INT_MAX
        else:
            assert before == want, cs.name


def test_new_symbols_are_bound():
    from mmduet_amd import _lib
    names = ('mmd_op_argmax', 'mmd_op_advance_state', 'mmd_op_embed_feed')
    assert all(n in _lib.EXPORTED_SYMBOLS for n in names)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names)


def test_nan_code_becomes_value_error_for_the_greedy_calls_too():
    from mmduet_amd import _lib
    _lib.lib()
    for what in ('mmd_greedy_generate', 'mmd_round_multi', 'mmd_sample_generate'):
        with pytest.raises(ValueError):
            _lib.check(_lib.MMD_EDOM, None, what)
