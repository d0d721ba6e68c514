#!/usr/bin/env python
"""Log-probability probe on the 7B synthetic config: what recording per-token log-probabilities costs per decode step.
    python tools/logprob_probe.py [tokens=32] [context=15000] [repeats=7] [out.json]
Per-token decode time of mmd_greedy_generate and mmd_sample_generate with the recording off, on with top_n = 0 and on with top_n = 8, same process, same context (declared
live with mmd_kv_debug_set_len: same traffic, no prefill): events around a (1 + tokens)-token response and around a 1-token response, per decode step = the difference /
tokens; median and spread over the repeats, the settings interleaved so that a clock drift hits all alike.  A build without the feature times the `off` setting alone (the
figure to compare a branch with its parent).  MMDUET_GRAPH=1 in the environment puts the decode loops on their captured steps (a change of the setting re-captures: the
probe lets that happen in an untimed two-token call)."""
import json, os, statistics, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import torch, bench
from mmduet_amd._lib import lib, check

ntok = int(sys.argv[1]) if len(sys.argv) > 1 else 32
nctx = int(sys.argv[2]) if len(sys.argv) > 2 else 15000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
out_json = sys.argv[4] if len(sys.argv) > 4 else None
sys.argv = [sys.argv[0]]
args = bench.parse(['--weights', 'bf16']); args.multi_stream = 0
dev = torch.device('cuda', 0)
model, tok, cfg = bench.build(args, dev)
cache = model.new_cache(initial_tokens=nctx + 4096)
check(lib().mmd_kv_debug_set_len(cache.arena.h, nctx), model._ctx, 'set_len')
prompt = (torch.randn(1, 5, cfg.hidden_size, device=dev) * 0.5).to(torch.bfloat16)
SAMPLING = dict(temperature=0.7, top_k=50, top_p=0.9, seed=7)
SETTINGS = (('off', -1), ('top0', 0), ('top8', 8)) if hasattr(model, 'set_generate_logprobs') else (('off', None),)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); r = fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b), r


def greedy(n):
    return model.greedy_generate(prompt, type(cache)(cache.arena, nctx), -1, n)[0]


def sampled(n):
    return model.sample_generate(prompt, type(cache)(cache.arena, nctx), -1, n, **SAMPLING)[0]


def setting(top):
    if top is not None:
        model.set_generate_logprobs(top)


res = dict(tokens=ntok, context=nctx, repeats=reps, graph=os.environ.get('MMDUET_GRAPH') == '1', decode={})
per = {(f.__name__, s): [] for f in (greedy, sampled) for s, _ in SETTINGS}
for rep in range(reps + 1):           # (repeat 0 is the warm-up: allocations, graph capture)
    for fn in (greedy, sampled):
        for name, top in SETTINGS:
            setting(top)
            if res['graph'] and len(SETTINGS) > 1:
                fn(2)          # (the captured step is keyed by the setting: capture outside the timed calls)
            t_long, ids = timed(lambda: fn(ntok + 1))
            t_one, _ = timed(lambda: fn(1))
            if rep:
                per[(fn.__name__, name)].append((t_long - t_one) / ntok)
            res.setdefault('ids', {})[f'{fn.__name__}_{name}'] = ids
setting(-1 if SETTINGS[0][1] is not None else None)
for (fn, name), v in per.items():
    res['decode'][f'{fn}_{name}'] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    print(f'{fn:8s} logprobs {name:5s} {statistics.median(v):.4f} ms/token (min {min(v):.4f}, max {max(v):.4f}) over {reps} repeats of {ntok} tokens at context {nctx}', flush=True)
res['ids_equal'] = all(res['ids'][f'{fn}_{name}'] == res['ids'][f'{fn}_off'] for fn in ('greedy', 'sampled') for name, _ in SETTINGS)
print('ids equal across the settings:', res['ids_equal'], flush=True)
if out_json:
    json.dump(res, open(out_json, 'w'), indent=1)
