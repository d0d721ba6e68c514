"""Cost of one mmd_round_multi round of 4 talking streams at 7B bf16 (synthetic weights, the vision tower cut to 2 layers: it does not run here), with the samplers'
log-probability recording off, on with top_n 0 and on with top_n 8.  The three configurations are interleaved, repetition by repetition, on one device.

    python tools/round_logprobs_bench.py [--context 2048] [--tokens 48] [--reps 5] [--out FILE.json]

A round = one decode row per stream through the LLM, lm_head over the 4 rows, the plain arg-max block, the record's launches when on, and the round's one
synchronisation; ms per round = wall time of `tokens` feed rounds / tokens, the median over the repetitions.  The library under test is the one the package loads."""
import argparse, json, os, sys, time
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--streams', type=int, default=4)
    ap.add_argument('--context', type=int, default=2048)
    ap.add_argument('--tokens', type=int, default=48)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    from mmduet_amd.weights import synthetic_weights
    cfg = VideoHeadLiveLlavaQwenConfig(frame_num_tokens=49, frame_resolution=384, v_placeholder='<image>', vit_num_hidden_layers=2, vit_layers_removed=1)
    m = VideoHeadLiveLlavaQwenForCausalLM(cfg, torch_dtype=torch.bfloat16, device='cuda', max_vit_batch=1, max_step_tokens=512, kv_initial_tokens=a.context + 4096)
    for name, t in synthetic_weights(cfg, seed=0, device='cuda', dtype=torch.bfloat16, scale='init02'):
        m.load_tensor(name, t)
    m.finalize()
    H = cfg.hidden_size
    g = torch.Generator().manual_seed(1)
    ctx = [(torch.randn(a.context, H, generator=g) * 0.02).to(torch.bfloat16).cuda() for _ in range(a.streams)]
    smps = [m.new_sampler() for _ in range(a.streams)]
    can_record = hasattr(smps[0], 'set_logprobs')
    configs = [('off', -1)] + ([('top_n_0', 0), ('top_n_8', 8)] if can_record else [])
    times = {name: [] for name, _ in configs}

    def response(top):
        caches = []
        for x in ctx:          # the context of every stream, 512 rows a step
            c = None
            for i in range(0, a.context, 512):
                c = m.multi_step([dict(x=x[i:i + 512], cache=c)], want_logits=False)[0]['cache']
            caches.append(c)
        for s in smps:
            s.begin(-1, 1.15, [], a.tokens + 1)
            if can_record and (top >= 0 or getattr(s, '_logprobs_top', -1) >= 0):
                s.set_logprobs(top)
        out = m.round_multi([dict(x=x[-1:], cache=c, sampler=s, sample=True) for x, c, s in zip(ctx, caches, smps)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.tokens):
            out = m.round_multi([dict(x=None, cache=o['cache'], sampler=s, feed=True, sample=True) for o, s in zip(out, smps)])
        dt = (time.perf_counter() - t0) / a.tokens * 1e3
        if can_record and top >= 0:
            assert smps[0].read_logprobs()['logprobs'].shape[0] == a.tokens + 1
        return dt

    response(-1)          # warm-up: arenas mapped, workspaces allocated
    for rep in range(a.reps):
        for name, top in configs:
            times[name].append(response(top))
    res = dict(streams=a.streams, context=a.context, tokens=a.tokens, reps=a.reps,
               ms_per_round={k: sorted(v)[len(v) // 2] for k, v in times.items()}, ms_per_round_all=times)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
