"""How far two accumulation orders of the same logits are apart in the tiny bf16 model: the rows of three streams from shared mmd_frame_step_multi calls (one call per
token, lm_head over the three last rows) against single-row replay calls, as |log_softmax| differences at the generated ids.  The figure is the measured part of the bf16
tolerance of tests/test_gpu_round_logprobs.py (BF16_MEASURED); both routes exist without the rounds' log-probabilities.

    python tools/round_logits_routes.py [--out FILE.json]

The three streams are the test's: plain greedy with a penalty list, constrained greedy, sampled; 12 tokens each, decoded in shared rounds with nothing recorded."""
import argparse, json, os, sys
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import test_gpu_round_logprobs as R
    from test_gpu_logprobs import replay_rows, prompt
    out = {}
    for dtype, name in ((torch.bfloat16, 'bf16'), (torch.float32, 'fp32')):
        m = R.model_of(dtype)
        x = prompt()
        streams = R.three_streams(m, (None, None, None))
        ids, _ = R.run_rounds(m, streams)
        # route 1: the three streams' rows from shared multi-stream steps, teacher-forced on the ids
        res = m.multi_step([dict(x=x[0], cache=None, hidden='last') for _ in ids])
        shared = [[o['logits'][0].float().cpu()] for o in res]
        for step in range(R.N_NEW - 1):
            emb = [m.get_input_embeddings()(torch.tensor([[i[step]]], device=m.device)).view(1, -1) for i in ids]
            res = m.multi_step([dict(x=e, cache=o['cache'], hidden='last') for e, o in zip(emb, res)])
            for s, o in zip(shared, res):
                s.append(o['logits'][0].float().cpu())
        # route 2: single-row replay calls
        worst = 0.0
        for i, s in zip(ids, shared):
            one = torch.log_softmax(replay_rows(m, x, i).double(), dim=-1)
            two = torch.log_softmax(torch.stack(s).double(), dim=-1)
            at = torch.tensor(i)[:, None]
            worst = max(worst, float((one.gather(1, at) - two.gather(1, at)).abs().max()))
        out[name] = dict(ids=ids, max_abs_log_softmax_difference_at_ids=worst)
        print(json.dumps({name: out[name]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
