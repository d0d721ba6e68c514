"""What responses return -- token ids and log-probability records as raw bit patterns -- for the recorder behind tests/golden/response_parent.json and
tests/test_gpu_response_state.py.

The fixture was recorded before csrc/response_plan.h and model.hip's `Response` existed; that change moved host bookkeeping only, so every entry must come back bit for bit.
    python tests/response_record.py OUT.json        records every case twice (fresh contexts each time); an entry that differs between the two is left out and listed
None may be left out of the fp32 cases, at most one in eight of the bf16 ones.

Cases (12 new tokens, the prompt is cfgA_ops.npz `step0_in`):
    f32_*     generate calls on the tiny golden model (cfgA) in fp32: {arg-max, sampled} x {penalty off, 1.3} x {constraints off, on} x {records off, top_n = 3}
    bf16_*    the same model in bf16 (tests/test_gpu_logprobs.py::test_generate_end_to_end_bf16): {arg-max, sampled} x {every switch off, every switch on}.  Its head_dim is
              16, so its decode steps are launched one by one ...
    graph_*   ... and the captured decode step gets the same four on the 2-layer true-width bf16 model created with MMDUET_GRAPH=1 (tests/llm_stress.py weights)
    rounds    three samplers -- plain arg-max with a penalty, constrained arg-max, sampled + recording -- sharing mmd_round_multi rounds on the fp32 model: a response that
              runs into max_new, a response on the same samplers that ends on EOS (the constrained one through the fallback to begin()'s eos id), and a second turn on the
              same samplers and caches
The constraint set is built from the free arg-max ids (`f32_base`): EOS = the sixth of them, min_new = 3, the second suppressed."""
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

NEW_TOKENS, PEN, PREV, TOP_N = 12, 1.3, [3, 4, 4, 11], 3
SAMPLING = dict(temperature=0.9, top_k=20, top_p=0.9, seed=7)
BF16_LEFT_OUT_CAP = 1 / 8


def switches_name(sampled, pen, cons, rec):
    return ('draw' if sampled else 'argmax') + ('_pen' if pen else '') + ('_cons' if cons else '') + ('_lp' if rec else '')


CROSS = [(s, p, c, r) for s in (0, 1) for p in (0, 1) for c in (0, 1) for r in (0, 1)]
CORNERS = [(s, a, a, a) for s in (0, 1) for a in (0, 1)]
CASES = (['f32_base'] + ['f32_' + switches_name(*k) for k in CROSS] + ['bf16_' + switches_name(*k) for k in CORNERS] + ['graph_' + switches_name(*k) for k in CORNERS]
         + ['rounds'])


def bits(t):
    return t.contiguous().view(torch.int32).flatten().tolist()


def records(rec):
    if rec is None:
        return None
    return dict(logprobs=bits(rec['logprobs']), sampling_logprobs=bits(rec['sampling_logprobs']), top_logprobs=bits(rec['top_logprobs']),
                top_logprob_ids=rec['top_logprob_ids'].flatten().tolist())


def prompt(m):
    from conftest import load_npz
    x = torch.from_numpy(load_npz('cfgA_ops.npz')['step0_in'])
    if x.shape[-1] != m.config.hidden_size:          # the true-width model: rows of its own width from a host generator
        x = torch.randn(x.shape[0], m.config.hidden_size, generator=torch.Generator().manual_seed(5)) * 0.5
    return x[None].to(m.dtype).cuda()


def build(kind):
    from helpers import hip_model
    if kind == 'f32':
        return hip_model('A', torch.float32)[0]
    if kind == 'bf16':
        return hip_model('A', torch.bfloat16)[0]
    import llm_stress as LS
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('MMDUET_GRAPH', '1')
        m = VideoHeadLiveLlavaQwenForCausalLM(LS.product_config(), torch_dtype=torch.bfloat16, max_vit_batch=1, max_step_tokens=64, kv_initial_tokens=1024)
    m.load_state_dict(LS.base_weights())
    return m


def generate(m, x, sampled, pen, cons, rec, max_new=NEW_TOKENS, prev=PREV, eos=-1, top_n=TOP_N):
    """one native generate call under the switches; the context's settings are put back.  -> dict(ids, prev, rec)"""
    m.set_generate_logprobs(top_n if rec else -1)
    m.set_generate_constraints(cons if cons else None)
    try:
        lst = list(prev) if pen else None
        if sampled:
            ids = m.sample_generate(x, None, eos, max_new, PEN if pen else None, lst, **SAMPLING)[0]
        else:
            ids = m.greedy_generate(x, None, eos, max_new, PEN if pen else None, lst)[0]
        return dict(ids=ids, prev=lst, rec=records(m.last_generate_logprobs()))
    finally:
        m.set_generate_logprobs(-1)
        m.set_generate_constraints(None)


def constraints_from(m, base_ids):
    from mmduet_amd import constraints as CS
    return CS.merge(m.config.vocab_size, eos_token_id=[base_ids[5]], min_new_tokens=3, suppress_tokens=[base_ids[1]])


def record_generate(m, prefix, keys):
    x = prompt(m)
    base = generate(m, x, 0, 0, None, 0)
    assert len(base['ids']) == NEW_TOKENS
    cons = constraints_from(m, base['ids'])
    out = {prefix + 'base': base} if prefix == 'f32_' else {}
    for s, p, c, r in keys:
        out[prefix + switches_name(s, p, c, r)] = generate(m, x, s, p, cons if c else None, r)
    return out


def record_rounds(m):
    """-> dict(response name -> dict(tokens per round [[plain, constrained, sampled] ...], prev_len of the three samplers, the sampled one's records))"""
    from mmduet_amd import constraints as CS
    from mmduet_amd._lib import lib
    H, V = m.config.hidden_size, m.config.vocab_size
    g = torch.Generator().manual_seed(41)
    first = [torch.randn(5, H, generator=g).cuda() * 0.5 for _ in range(3)]
    turn = [torch.randn(2, H, generator=g).cuda() * 0.5 for _ in range(3)]
    cons = CS.merge(V, min_new_tokens=2, suppress_tokens=[7], sequence_bias={(9,): 1.5})          # no EOS ids of its own: begin()'s eos id is the response's
    smps = [m.new_sampler() for _ in range(3)]
    smps[2].set_logprobs(TOP_N)

    def begin(eos, prev, max_new, restart):
        smps[0].begin(eos[0], PEN, prev[0], max_new)
        smps[1].begin(eos[1], None, None, max_new, constraints=cons)
        smps[2].begin(eos[2], PEN, prev[2], max_new, sampling=dict(restart=restart, **SAMPLING))

    def respond(xs, caches, eos, max_new):
        """rounds until every sampler's response is over: a sampler stops sampling behind its EOS or its max_new-th token"""
        live, rounds, seen = [0, 1, 2], [], [[], [], []]
        out = m.round_multi([dict(x=xs[i], cache=caches[i], sampler=smps[i], sample=True) for i in live])
        while True:
            toks = [None] * 3
            for i, o in zip(live, out):
                toks[i], caches[i] = o['token'], o['cache']
                seen[i].append(o['token'])
            rounds.append(toks)
            live = [i for i in live if toks[i] != eos[i] and len(seen[i]) < max_new]
            if not live:
                break
            out = m.round_multi([dict(x=None, cache=caches[i], sampler=smps[i], feed=True, sample=True) for i in live])
        return dict(tokens=rounds, prev_len=[int(lib().mmd_sampler_prev_len(s.h)) for s in smps], rec=records(smps[2].read_logprobs())), seen

    res = {}
    caches = [None] * 3
    begin([-1] * 3, [list(PREV), None, list(PREV)], 5, restart=True)
    res['runs_into_max_new'], seen = respond(first, caches, [-1] * 3, 5)
    eos = [s[2] for s in seen]          # the third token of each: with the same inputs (the draw's offset restarts) the next response ends there, or earlier
    caches = [None] * 3
    begin(eos, [list(PREV), None, list(PREV)], NEW_TOKENS, restart=True)
    res['ends_on_eos'], seen = respond(first, caches, eos, NEW_TOKENS)
    prev = [list(PREV) + [t for t in s if t != e] for s, e in zip(seen, eos)]
    begin([-1] * 3, prev, 4, restart=False)
    res['second_turn'], _ = respond(turn, caches, [-1] * 3, 4)
    return res


def record_all():
    out = {}
    m = build('f32')
    out.update(record_generate(m, 'f32_', CROSS))
    out['rounds'] = record_rounds(m)
    del m
    out.update(record_generate(build('bf16'), 'bf16_', CORNERS))
    out.update(record_generate(build('graph'), 'graph_', CORNERS))
    assert sorted(out) == sorted(CASES)
    return out


def left_out_within_the_caps(left_out):
    bf = [c for c in CASES if not c.startswith('f32_') and c != 'rounds']
    return all(c in bf for c in left_out) and len(left_out) <= BF16_LEFT_OUT_CAP * len(bf)


if __name__ == '__main__':
    a, b = record_all(), record_all()
    left_out = sorted(k for k in a if a[k] != b[k])
    res = dict(entries={k: v for k, v in a.items() if k not in left_out}, left_out=left_out)
    with open(sys.argv[1], 'w') as f:
        json.dump(res, f, sort_keys=True, separators=(',', ':'))
        f.write('\n')
    print('recorded', len(res['entries']), 'left out', left_out, 'within the caps:', left_out_within_the_caps(left_out))
