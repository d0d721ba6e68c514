#!/usr/bin/env python
"""Sampling probe on the 7B synthetic config: what sampled decoding costs beside greedy decoding, and what the sampling chain costs alone.
    python tools/sampling_probe.py [tokens=32] [context=4096] [repeats=7] [out.json]
  1. per-token decode time of mmd_sample_generate against mmd_greedy_generate, same process, same context (declared live with mmd_kv_debug_set_len: same traffic, no
     prefill): events around a (1 + tokens)-token response and around a 1-token response, per decode step = the difference / tokens; median and spread over the repeats.
  2. the sampling chain alone (mmd_op_sample) at n = 1 and n = 8 rows of V = 152064 random logits, three parameter sets, events around `iters` calls.  The raw operator
     allocates and frees its scratch and synchronises per call, so these are upper bounds of the chain inside a decode step.
MMDUET_GRAPH=1 in the environment puts both decode loops on their captured steps; the ids of the sampled response are printed so that the two routes can be compared."""
import json, os, statistics, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import torch, bench
from mmduet_amd._lib import lib, check

ntok = int(sys.argv[1]) if len(sys.argv) > 1 else 32
nctx = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); r = fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b), r


def greedy(n):
    return model.greedy_generate(prompt, type(cache)(cache.arena, nctx), -1, n)[0]


def sampled(n):
    return model.sample_generate(prompt, type(cache)(cache.arena, nctx), -1, n, **SAMPLING)[0]


res = dict(tokens=ntok, context=nctx, repeats=reps, graph=os.environ.get('MMDUET_GRAPH') == '1', decode={}, chain={})
for fn in (greedy, sampled):          # warm-up: allocations, graph capture
    fn(ntok + 1); fn(1)
per = dict(greedy=[], sampled=[])
for _ in range(reps):                 # interleaved, so a clock drift hits both alike
    for name, fn in (('greedy', greedy), ('sampled', sampled)):
        t_long, ids = timed(lambda: fn(ntok + 1))
        t_one, _ = timed(lambda: fn(1))
        per[name].append((t_long - t_one) / ntok)
    res['sampled_ids'] = ids
for name, v in per.items():
    res['decode'][name] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    print(f'{name:8s} {statistics.median(v):.4f} ms/token (min {min(v):.4f}, max {max(v):.4f}) over {reps} repeats of {ntok} tokens at context {nctx}', flush=True)
g, s = res['decode']['greedy']['median_ms'], res['decode']['sampled']['median_ms']
print(f'sampled / greedy = {s / g:.4f}   sampled ids: {res["sampled_ids"]}', flush=True)

V, iters = 152064, 50
gen = torch.Generator(device='cpu').manual_seed(3)
for n in (1, 8):
    lg = (torch.randn(n, V, generator=gen) * 3).to(dev)
    for T, k, p in ((1.0, 0, 1.0), (0.7, 50, 1.0), (0.7, 0, 0.9), (0.7, 50, 0.9)):
        for _ in range(5):
            model.sample_op(lg, temperature=T, top_k=k, top_p=p, seed=1)
        ms, _ = timed(lambda: [model.sample_op(lg, temperature=T, top_k=k, top_p=p, seed=1, offset=i) for i in range(iters)])
        res['chain'][f'n{n}_T{T}_k{k}_p{p}'] = ms / iters
        print(f'chain n={n} T={T} k={k} p={p}: {ms / iters * 1e3:.1f} us per call (raw operator: with its scratch allocation and synchronisation)', flush=True)
if out_json:
    json.dump(res, open(out_json, 'w'), indent=1)
