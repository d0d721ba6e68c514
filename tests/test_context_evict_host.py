"""CPU checks of informative eviction (DESIGN.md section 5 "Eviction"): the policy function against a brute-force reference over random ledgers; the driver over the
duck-typed oracle model with context_evict='informative' -- before every forward each ledger entry denotes exactly the tokens its frame wrote, with that frame's score,
and no forward leaves the context past the window --; and 'oldest' (the default) asks the model for exactly the drops the driver asked for before the policy existed."""
import random

import pytest
import torch

from helpers import oracle_model, make_args, tokenizer_for, stream_cases, stream_frames
from mmduet_amd.inference import LiveInferForBenchmark, context_evict_spans, _p1
from oracle import duet_oracle as O


# ---- the policy ----------------------------------------------------------------------------------------------------------------------------------------------
def reference_spans(frames, need, sink, length, recent):
    """by search: the shortest prefix of the candidates, ordered by (score, start), that frees `need` tokens; then every token of it, as maximal runs"""
    if need <= 0:
        return []
    cand = [f for f in frames if f[0] >= sink and f[1] <= length - recent]
    order = sorted(range(len(cand)), key=lambda i: (cand[i][2], cand[i][0]))
    for k in range(1, len(order) + 1):
        if sum(cand[i][1] - cand[i][0] for i in order[:k]) >= need:
            gone = sorted(t for i in order[:k] for t in range(cand[i][0], cand[i][1]))
            runs = []
            for t in gone:
                if runs and runs[-1][1] == t:
                    runs[-1][1] = t + 1
                else:
                    runs.append([t, t + 1])
            return [tuple(r) for r in runs]
    return None


def random_ledger(rng):
    """frames of 1-7 tokens with text between some of them, scores from a small set (ties)"""
    at, frames = rng.randrange(0, 12), []
    for _ in range(rng.randrange(0, 14)):
        w = rng.randrange(1, 8)
        frames.append((at, at + w, rng.choice([0.0, 0.1, 0.1, 0.25, 0.5, 0.9, rng.random()])))
        at += w + rng.choice([0, 0, 0, 3])
    return frames, at + rng.randrange(0, 9)


def test_policy_against_the_reference():
    rng = random.Random(5)
    seen = dict(none=0, exact=0, ties=0, recent=0, sink=0, merged=0, nothing=0)
    for _ in range(400):
        frames, length = random_ledger(rng)
        sink, recent = rng.choice([0, 5, 12, 20]), rng.choice([0, 0, 4, 10, length])
        cand = [f for f in frames if f[0] >= sink and f[1] <= length - recent]
        room = sum(f[1] - f[0] for f in cand)
        for need in {0, 1, 3, 7, room, room + 1, rng.randrange(0, room + 2)}:
            got = context_evict_spans(frames, need, sink, length, recent)
            want = reference_spans(frames, need, sink, length, recent)
            assert got == want, (frames, need, sink, length, recent, got, want)
            if got is None:
                seen['none'] += 1; assert need > room
                continue
            if need <= 0:
                seen['nothing'] += 1; assert got == []
                continue
            freed = sum(b - a for a, b in got)
            assert freed >= need and all(a >= sink and b <= length - recent for a, b in got)
            assert all(p[1] < q[0] for p, q in zip(got, got[1:]))          # ascending, merged where they touch
            seen['exact'] += freed == need
            seen['ties'] += len({f[2] for f in cand}) < len(cand)
            seen['recent'] += any(f[1] > length - recent for f in frames)
            seen['sink'] += any(f[0] < sink for f in frames)
            seen['merged'] += any(sum(1 for f in cand if a <= f[0] and f[1] <= b) > 1 for a, b in got)
    assert all(v > 10 for v in seen.values()), seen
    # lists work as ledger entries, the lowest score goes first, ties oldest first
    led = [[20, 30, 0.5], [30, 40, 0.1], [45, 55, 0.1], [55, 65, 0.9], [65, 75, 0.05]]
    assert context_evict_spans(led, 10, 20, 100, 20) == [(65, 75)]
    assert context_evict_spans(led, 11, 20, 100, 20) == [(30, 40), (65, 75)]
    assert context_evict_spans(led, 21, 20, 100, 20) == [(30, 40), (45, 55), (65, 75)]
    assert context_evict_spans(led, 31, 20, 100, 20) == [(20, 40), (45, 55), (65, 75)]
    assert context_evict_spans(led, 51, 20, 100, 20) is None and context_evict_spans(led, 10, 20, 100, 30) == [(30, 40)]


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------------------
class Windowed:
    """the oracle model with kv_drop / kv_drop_many by slicing the handle, every call recorded, and the driver's ledger checked before every forward"""

    def __init__(self, m):
        self.__dict__.update(_m=m, drops=[], many=[], lens=[], driver=None, rows={}, forwards=0, checked=0)

    def __getattr__(self, name):
        return getattr(self._m, name)

    def kv_drop(self, handle, start, end, shift=False):
        self.drops.append((int(start), int(end), bool(shift)))
        return O.KVHandle([torch.cat([k[:, :start], k[:, end:]], 1) for k in handle.k], [torch.cat([v[:, :start], v[:, end:]], 1) for v in handle.v])

    def kv_drop_many(self, handle, spans, shift=False):
        spans = [(int(a), int(b)) for a, b in spans]
        assert spans and all(a < b for a, b in spans) and all(p[1] < q[0] for p, q in zip(spans, spans[1:])) and spans[-1][1] <= len(handle)
        self.many.append((spans, bool(shift)))
        for a, b in reversed(spans):
            handle = O.KVHandle([torch.cat([k[:, :a], k[:, b:]], 1) for k in handle.k], [torch.cat([v[:, :a], v[:, b:]], 1) for v in handle.v])
        return handle

    def check_ledger(self, past):
        """every entry: frame_num_tokens consecutive rows of one forward, ending on the row whose informative score the entry carries"""
        d, nt = self.driver, self._m.config.frame_num_tokens
        n = len(past) if past else 0
        led = [e for e in d._frame_ledger if e[1] <= n]          # (entries of a speculative chunk behind the context are cut when the driver next looks)
        assert all(p[1] <= q[0] for p, q in zip(led, led[1:]))
        for start, end, score in led:
            assert end - start == nt
            where = [self.rows[past.v[-1][0, t].numpy().tobytes()] for t in range(start, end)]
            assert all(w[0] == where[0][0] and w[1] == where[0][1] + k for k, w in enumerate(where)), (start, end, where)
            assert where[-1][2] == score
            self.checked += 1

    def __call__(self, inputs_embeds=None, past_key_values=None, **kw):
        if self.driver is not None:
            self.check_ledger(past_key_values)
        n0 = len(past_key_values) if past_key_values else 0
        out = self._m(inputs_embeds=inputs_embeds, past_key_values=past_key_values, **kw)
        self.forwards += 1
        inf = out.informative_logits[0]
        for r in range(inputs_embeds.shape[1]):
            self.rows[out.past_key_values.v[-1][0, n0 + r].numpy().tobytes()] = (self.forwards, r, _p1(float(inf[r, 0]), float(inf[r, 1])))
        self.lens.append(len(out.past_key_values))
        return out


def run_driver(fpf, n_frames=40, **over):
    meta = stream_cases()
    case = meta['cases']['prob_keep']
    opts = case['opts']
    model = oracle_model('A')[0]
    args = make_args(frame_fps=case['fps'], system_prompt=meta['system_prompt'], max_new_tokens=12, stream_end_prob_threshold=opts['stream_end_prob_threshold'],
                     score_heads=opts['score_heads'], frames_per_forward=fpf, **over)
    tok = tokenizer_for(model.config)
    model.config.eos_token_id = meta['eos_token_id']
    wm = Windowed(model)
    d = LiveInferForBenchmark(args, model=wm, tokenizer=tok)
    wm.driver = d
    d.input_video_stream(torch.cat([stream_frames('prob_keep')] * 4)[:n_frames])
    d.input_query_stream(case['conversation'])
    d.inference()
    wm.check_ledger(d.past_key_values)
    return d, wm


def window_for(fpf):
    base, wm = run_driver(fpf)
    nt = base.frame_num_tokens
    assert base.dropped_tokens == 0 and wm.drops == [] and wm.many == [] and base._frame_ledger == []          # the window is off: no ledger is kept
    return base._sink_tokens + (fpf + 5) * nt + 40, max(wm.lens), base


@pytest.mark.parametrize('remove', [False, True], ids=['turns-kept', 'turns-removed'])
@pytest.mark.parametrize('fpf', [1, 3])
def test_informative_driver_keeps_its_ledger_and_the_window(fpf, remove):
    window, longest, base = window_for(fpf)
    assert window < longest
    nt = base.frame_num_tokens
    d, wm = run_driver(fpf, context_window=window, context_evict='informative', context_recent=2 * nt, remove_assistant_turns=remove)
    assert d.context_evict == 'informative' and len(d.debug_data_list) == 40
    assert max(wm.lens) <= window, (max(wm.lens), window)
    assert len(wm.many) >= 3 and d.evicted_frames >= 3 and wm.checked > 100
    assert d.dropped_tokens == sum(b - a for sp, _ in wm.many for a, b in sp) + sum(b - a for a, b, _ in wm.drops)
    assert all(not s for _, s in wm.many)
    # frames left the middle of the context, not only its front
    assert any(sp[0][0] > d._sink_tokens for sp, _ in wm.many)
    # the ledger at the end: every frame still in the context
    assert all(e[1] <= len(d.past_key_values) for e in d._frame_ledger) and len(d._frame_ledger) >= 2
    # shifted positions reach the model
    d2, wm2 = run_driver(fpf, context_window=window, context_evict='informative', context_recent=2 * nt, context_positions='shifted', remove_assistant_turns=remove)
    assert wm2.many and all(s for _, s in wm2.many) and [sp for sp, _ in wm2.many] == [sp for sp, _ in wm.many]
    d.reset()
    assert d._frame_ledger == [] and d.evicted_frames == 0


def test_nothing_evictable_falls_back_to_the_oldest_tokens():
    window, _, base = window_for(2)
    d, wm = run_driver(2, context_window=window, context_evict='informative', context_recent=window)          # every frame is recent
    assert wm.many == [] and wm.drops and max(wm.lens) <= window
    o, wo = run_driver(2, context_window=window)
    assert wm.drops == wo.drops and d.dropped_tokens == o.dropped_tokens and d.debug_data_list == o.debug_data_list
    wm.check_ledger(d.past_key_values)


@pytest.mark.parametrize('fpf', [1, 3])
def test_oldest_makes_the_drops_it_always_made(fpf):
    """the default policy: the kv_drop calls, recorded by the stub, are those the driver made before the policy existed (tests/golden/context_oldest_drops.json: the
    same stub around the driver of the commit before, same stream, same windows), and kv_drop_many is never called"""
    import json, os
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'context_oldest_drops.json')))
    window, _, base = window_for(fpf)
    for name, kw in (('kept', dict()), ('shifted-q16', dict(context_positions='shifted', context_drop_quantum=16)), ('kept', dict(context_evict='oldest'))):
        rec = golden[f'fpf{fpf}-{name}']
        assert rec['window'] == window and len(rec['drops']) >= 3
        d, wm = run_driver(fpf, context_window=window, **kw)
        assert d.context_evict == 'oldest' and wm.many == []
        assert [list(x) for x in wm.drops] == rec['drops']
        assert d.dropped_tokens == sum(b - a for a, b, _ in wm.drops)
        assert d.evicted_frames > 0 and all(e[1] <= len(d.past_key_values) for e in d._frame_ledger)          # the ledger follows these drops too


def test_flags_and_attributes():
    from mmduet_amd.__main__ import cli_extra_args
    ns = cli_extra_args(['--context_window', '4096', '--context_evict', 'informative', '--context_recent', '512'])
    assert (ns.context_evict, ns.context_recent) == ('informative', 512)
    ns = cli_extra_args(['--context_window', '4096'])
    assert (ns.context_evict, ns.context_recent) == ('oldest', None)
    with pytest.raises(SystemExit):
        cli_extra_args(['--context_evict', 'random'])
    model = oracle_model('A')[0]
    with pytest.raises(ValueError, match='context_evict'):
        LiveInferForBenchmark(make_args(stream_end_prob_threshold=0.5, context_evict='newest'), model=model, tokenizer=tokenizer_for(model.config))
    for bad in (-1, 2.5, 'many'):
        with pytest.raises(ValueError, match='context_recent'):
            LiveInferForBenchmark(make_args(stream_end_prob_threshold=0.5, context_recent=bad), model=model, tokenizer=tokenizer_for(model.config))
    d = LiveInferForBenchmark(make_args(stream_end_prob_threshold=0.5, context_window=300), model=model, tokenizer=tokenizer_for(model.config))
    assert (d.context_evict, d.context_recent, d.evicted_frames) == ('oldest', None, 0)
