"""Sampling without a GPU: the CPU restatement of the contract (tests/sampling_oracle.py) against published Philox vectors and the literal HF warpers, the new symbols,
the model class's surface, and the chi-square guard of the statistical GPU test."""
import numpy as np
import pytest
import torch
import sampling_oracle as SO

CHI_LOGITS = [2.0, 1.0, 0.0, -1.0, -2.0, 0.5, 0.5, -np.inf]


def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32 10 rounds: the all-zero, the all-ones and the digits-of-pi vectors."""
    assert SO.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    f = 0xffffffff
    assert SO.philox4x32_10((f, f, f, f), (f, f)) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert SO.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def test_philox_word_layout():
    x = SO.philox4x32_10((5, 1, 7, 0), (0x89abcdef, 0x01234567))
    assert SO.philox_word(0x0123456789abcdef, (1 << 32) + 5, lane=7) == (x[0] << 32) | x[1]


def hf_keep(z, top_k, top_p):
    """TopKLogitsWarper then TopPLogitsWarper (min_tokens_to_keep = 1) as transformers writes them, float64."""
    s = z.clone()
    if 0 < top_k < s.numel():
        s = s.masked_fill(s < torch.topk(s, top_k)[0][-1], -float('inf'))
    if top_p < 1.0:
        sl, si = torch.sort(s, descending=False)
        remove = sl.softmax(-1).cumsum(-1) <= (1 - top_p)
        remove[-1:] = False
        s = s.masked_fill(torch.zeros_like(remove).scatter(0, si, remove), -float('inf'))
    return ~torch.isinf(s)


@pytest.mark.parametrize('top_k', [1, 5, 50])
@pytest.mark.parametrize('top_p', [0.3, 0.9, 1.0])
def test_oracle_keeps_what_hf_keeps(top_k, top_p):
    g = torch.Generator().manual_seed(1000 * top_k + int(top_p * 10))
    done = 0
    while done < 8:
        z = torch.randn(1000, generator=g, dtype=torch.float64) * 4
        if z.unique().numel() != z.numel():
            continue
        rank, above, keep = SO.analyse(z.numpy(), top_k, top_p)
        if top_p < 1.0 and np.abs(above - top_p).min() < 1e-9:          # a boundary nobody can call: another row, not an excuse
            continue
        assert np.array_equal(keep, hf_keep(z, top_k, top_p).numpy()), (top_k, top_p)
        assert keep[int(z.argmax())]
        done += 1


@pytest.mark.parametrize('top_k,top_p', [(0, 1.0), (3, 1.0), (0, 0.6), (4, 0.5), (1, 1.0), (40, 1e-6)])
def test_class_form_equals_literal_form(top_k, top_p):
    rng = np.random.default_rng(7)
    for z in (rng.standard_normal(33) * 3, np.round(rng.standard_normal(33) * 2), np.where(rng.random(33) < 0.2, -np.inf, rng.standard_normal(33)), np.zeros(9)):
        z[0] = max(z[0], 0.0)          # (never a row of -inf only)
        a, b = SO.analyse(z, top_k, top_p), SO.analyse_literal(z, top_k, top_p)
        assert np.array_equal(a[0], b[0]) and np.allclose(a[1], b[1], rtol=0, atol=1e-14) and np.array_equal(a[2], b[2])
        assert a[2][int(np.argmax(z))]
        kept_min = z[a[2]].min()
        assert np.array_equal(a[2], z >= kept_min)          # the kept set is a threshold set


def test_penalty_is_applied_once_per_id():
    l = np.array([2.0, -1.0, 0.5, 3.0])
    z = SO.scores(l, prev_ids=[0, 0, 1, 0], penalty=2.0, temperature=0.5)
    assert np.array_equal(z, np.array([1.0, -2.0, 0.5, 3.0]) / 0.5)


def test_new_symbols_are_bound():
    from mmduet_amd import _lib
    names = ('mmd_sampler_set_sampling', 'mmd_sample_generate', 'mmd_op_sample', 'mmd_set_sample_lane', 'mmd_sampler_lane', 'mmd_sampler_offset')
    assert all(n in _lib.EXPORTED_SYMBOLS for n in names)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names)


def test_model_class_has_generate():
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM as M
    assert callable(getattr(M, 'generate', None)) and callable(getattr(M, 'generate_after_embed', None)) and callable(getattr(M, 'sample_generate', None))
    m = object.__new__(M)          # the argument checks come before anything touches the device
    for kw in (dict(num_beams=2), dict(num_return_sequences=3), dict(min_p=0.1), dict(typical_p=0.5)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            M.generate(m, input_ids=torch.zeros(1, 2, dtype=torch.long), **kw)


def test_nan_code_becomes_value_error():
    from mmduet_amd import _lib
    _lib.lib()
    with pytest.raises(ValueError):
        _lib.check(_lib.MMD_EDOM, None, 'mmd_sample_generate')


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_chi_square_guard(seed):
    """4096 draws from the 8-entry row through the oracle's own Philox words: chi-square below the 0.999 quantile at 6 degrees of freedom (7 live categories)."""
    z = SO.scores(CHI_LOGITS)
    keep = SO.analyse(z)[2]
    n = 4096
    counts = np.bincount([SO.draw(z, keep, SO.philox_word(seed, off))[0] for off in range(n)], minlength=8)
    p = np.exp(z - z.max()); p /= p.sum()
    assert counts[7] == 0
    chi = float((((counts[:7] - n * p[:7]) ** 2) / (n * p[:7])).sum())
    print('chi-square', seed, chi)
    assert chi < 24.32
