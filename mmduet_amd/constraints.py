"""Host side of constrained decoding (DESIGN.md "Constraints"): the HF-shaped generate arguments merged into what mmd_set_generate_constraints takes.

HF's processors, in the order of generation/utils.py::_get_logits_processor -- sequence bias, repetition penalty, bad words / min-new-tokens / suppress, temperature --
collapse to one table of (id, bias) with -inf meaning "suppressed", an EOS set and min_new_tokens:
    z_i = mask_i(pen(l_i + b_i)) / T
Pure Python: nothing here touches the device, so the limits are testable without one.  The native call checks them again.
"""
import math
from collections import namedtuple

MAX_TABLE, MAX_EOS = 256, 8

Constraints = namedtuple('Constraints', 'eos min_new ids bias')
Constraints.on = property(lambda c: bool(c.eos) or c.min_new > 0 or bool(c.ids))
OFF = Constraints((), 0, (), ())


def _single(entry, what):
    """The one token id of a bad_words_ids / sequence_bias entry; a sequence of several tokens is not built."""
    if isinstance(entry, int):
        return int(entry)
    ids = [int(t) for t in entry]
    if len(ids) != 1:
        raise NotImplementedError(f'generate: {what} entries of {len(ids)} tokens are not supported, single tokens only')
    return ids[0]


def merge(vocab_size, eos_token_id=None, min_new_tokens=None, suppress_tokens=None, bad_words_ids=None, sequence_bias=None):
    """-> Constraints(eos, min_new, ids, bias), ids ascending and unique.
    eos_token_id: None, an id or a list (duplicates dropped, order kept).  suppress_tokens: ids.  bad_words_ids: [[id], ...].  sequence_bias: {(id,): bias} or
    [[[id], bias], ...]; a bias of -inf suppresses; a later entry for an id replaces an earlier one.  An id both biased and suppressed is suppressed.
    ValueError: more than 8 EOS ids or 256 table ids, an id outside [0, vocab_size), a NaN or +inf bias, a negative min_new_tokens, or suppressed ids that together with
    the EOS ids cover the vocabulary.  NotImplementedError: a multi-token bad_words_ids / sequence_bias entry."""
    V = int(vocab_size)
    if eos_token_id is None:
        eos = []
    elif isinstance(eos_token_id, (list, tuple)):
        eos = list(dict.fromkeys(int(t) for t in eos_token_id))
    else:
        eos = [int(eos_token_id)]
    min_new = int(min_new_tokens or 0)
    if min_new < 0:
        raise ValueError(f'min_new_tokens={min_new} is negative')
    table = {}
    if sequence_bias:
        items = sequence_bias.items() if isinstance(sequence_bias, dict) else [(e[0], e[1]) for e in sequence_bias]
        for key, b in items:
            b = float(b)
            if math.isnan(b) or b == math.inf:
                raise ValueError(f'sequence_bias: the bias {b} is neither finite nor -inf')
            table[_single(key, 'sequence_bias')] = b
    for t in (bad_words_ids or ()):
        table[_single(t, 'bad_words_ids')] = -math.inf
    for t in (suppress_tokens or ()):
        table[int(t)] = -math.inf
    for t in list(table) + eos:
        if not 0 <= t < V:
            raise ValueError(f'token id {t} is outside the vocabulary of {V}')
    if len(eos) > MAX_EOS:
        raise ValueError(f'{len(eos)} EOS ids: at most {MAX_EOS}')
    if len(table) > MAX_TABLE:
        raise ValueError(f'{len(table)} biased / suppressed ids: at most {MAX_TABLE}')
    ids = sorted(table)
    covered = {t for t in ids if table[t] == -math.inf} | set(eos)
    if (ids or eos) and len(covered) >= V:
        raise ValueError(f'the suppressed ids and the EOS ids cover the whole vocabulary of {V}: no token could be returned')
    return Constraints(tuple(eos), min_new, tuple(ids), tuple(table[t] for t in ids))


def c_arrays(cons):
    """The ctypes arguments of mmd_set_generate_constraints / mmd_sampler_set_constraints behind the handle: (eos, n_eos, min_new, ids, bias, n)."""
    import ctypes as C
    cons = cons or OFF
    eos = (C.c_int64 * max(1, len(cons.eos)))(*cons.eos)
    ids = (C.c_int32 * max(1, len(cons.ids)))(*cons.ids)
    bias = (C.c_float * max(1, len(cons.bias)))(*cons.bias)
    return eos, len(cons.eos), int(cons.min_new), ids, bias, len(cons.ids)
