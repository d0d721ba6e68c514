"""The vision tower on its side stream beside the decoder on the main stream, at true width: running them together changes no bit.

The shipped drivers (mmduet_amd/inference.py `_issue_vit`, mmduet_amd/multistream.py) enqueue tower batches on a lowest-priority side HIP stream of the SAME native context the
decoder steps run in.  That is correct only while the two streams share no scratch memory: tower code touches the context's v_* workspaces (its own split-K slabs v_splitk_ws
and attention partials v_attn_ws among them), decoder code the l_* ones, splitk_ws, attn_ws and the decode / round / sampling / scoring scratch (DESIGN.md section 5 lists both
sets).  Every operator is pinned to an fp32 reference elsewhere in the suite, running alone; here the statement is only that concurrency does not change a bit.

Model: the true-width one of tests/test_gpu_production.py, `_build(2, 2, bf16)` -- 7B decoder widths, so400m tower widths, 2 + 2 layers: the kernels, grids, split-K slabs, key
splits and persistent ring grids of the full-depth model, live on both streams at once.

Part 1, operator pairs.  A tower job (several batches back to back into disjoint slices of one buffer) and a decoder job run serialized once -- tower, synchronize, decoder,
synchronize: the expected bits -- then 10 times concurrently, the tower enqueued exactly as `_issue_vit` does it (side.wait_stream(main), the job, an event behind it) and the
decoder on the current stream with no host synchronisation in between.  Every output (tower rows; head logits, final hidden rows, lm logits, token ids, log-probabilities, NLL, and the K / V rows the job
wrote in both layers as the arena stores them) must equal the serialized bits, and the step / tower / attention plans must be the same (the concurrent run took the same
kernels).  The overlap is a CONDITION: each job is bracketed by timing events on its own stream and at least 8 of the 10 repeats must have intersecting intervals, else the case
fails (10 and 8 bound the case's run time; no measurement stands behind them).

Part 2, the shipped schedules.  LiveInferForBenchmark under the five tower schedules of tests/test_gpu_streams.py and MultiStreamInfer (4 slots, k = 13, tower two batches
ahead, native rounds -- the schedule in which wrong bits were once seen with captured tower graphs, profiles/r06_tower_graph.md) on 60-frame clips with two pinned 16-token
responses per stream, in a context whose tower batch is 13 frames (five batches per clip: the lookahead and burst schedules then really differ, which is asserted): scores as Python floats, response ids, the final KV length and the final KV contents identical across schedules and across five repeats.  Five repeats are
a time budget, not a proof of absence: a hazard rarer than that passes here.
(What the multi-stream test did catch, in its second pass: a new sampler's token slot was zeroed on whichever stream the context was bound to last -- the tower's -- and the
fill landed behind the first drawn token.  DESIGN.md section 5.)

The side stream is chosen, not just created: the runtime deals streams onto a few hardware queues, and one that shares the main stream's queue runs strictly behind it (see
_overlapping_stream) -- two jobs that never run together prove nothing.

Shown once on a scratch copy of the library (not committed): with the tower's GEMMs pointed at the decoder's split-K workspace (gemm_args: c->splitk_ws for tower launches) the
three cases beside 1-frame tower batches -- the only tower shape that leaves split-K slabs -- fail in their first repeat (tower rows, log-probabilities); the others pass."""
import ctypes as C
import random
import pytest
import torch
from mmduet_amd._lib import lib

pytestmark = pytest.mark.gpu
from helpers import _build
from kv_layout import BLK, v_logical

H = 3584
REPEATS, MIN_OVERLAPPED = 10, 8


# ---- models ----------------------------------------------------------------------------------------------------------------------------------------
def _release(m):
    m.release_pooled_arenas()
    torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def width2():
    """true widths, 2 tower layers + 2 decoder layers, bf16: the model of tests/test_gpu_production.py"""
    m, w, _ = _build(2, 2, torch.bfloat16)
    del w
    yield m
    _release(m)


@pytest.fixture(scope='module')
def width2_fp8():
    """the same with fp8-e4m3 decoder weights"""
    m, w, _ = _build(2, 2, torch.bfloat16, weight_dtype='fp8')
    del w
    yield m
    _release(m)


@pytest.fixture(scope='module')
def width2_graph():
    """the same with the captured decode step switched on (MMDUET_GRAPH is read when the native context is created; the default environment decodes by eager launches)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('MMDUET_GRAPH', '1')
        m, w, _ = _build(2, 2, torch.bfloat16)
    del w
    yield m
    _release(m)


MULTI_SLOTS, MULTI_K, DRIVER_VIT_BATCH = 4, 13, 13


@pytest.fixture(scope='module')
def width2_drivers():
    """the same weights in a context for the driver tests: sized for four streams' merged k = 13 chunks, as bench.py sizes its multi-stream leg, and with tower batches of 13
    frames, so that a 60-frame clip is FIVE tower batches -- with the 35-frame batch of the other contexts it would be two, every lookahead schedule would issue both before
    the first forward and no burst would ever find a batch left to issue"""
    m, w, _ = _build(2, 2, torch.bfloat16, max_vit_batch=DRIVER_VIT_BATCH, max_step_tokens=MULTI_SLOTS * (MULTI_K * 49 + 192))
    del w
    yield m
    _release(m)


# ---- reading results -------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    """the raw bits of a tensor (NaNs compare equal to themselves, -0 differs from +0)"""
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b.to(a.device)))
    return a == b


def _first_difference(a, b):
    """where two tensors differ: for the failure message (rows say which operator)"""
    if not torch.is_tensor(a) or not torch.is_tensor(b) or a.shape != b.shape:
        return 'shape / type'
    d = (_bits(a) != _bits(b.to(a.device))).nonzero()
    return f'{d.shape[0]} elements, first at {d[0].tolist()}, last at {d[-1].tolist()}'


def _kv_rows(m, cache, lo, hi=None):
    """K and V of tokens [lo, hi) of every layer, read back as the arena stores them (mmd_kv_debug_read): -> (K [layers, nkv, hi - lo, d], V the same, in token order)"""
    from mmduet_amd._lib import check
    from mmduet_amd.modeling_live import _ptr
    hi = len(cache) if hi is None else hi
    cfg = m.config
    layers, nkv, d = cfg.num_hidden_layers, cfg.num_key_value_heads, cfg.head_dim
    n64 = (hi + BLK - 1) // BLK * BLK
    K = torch.empty(layers, nkv, n64, d, dtype=m.dtype, device=m.device)
    V = torch.empty(layers, nkv, n64 // BLK, d, BLK, dtype=m.dtype, device=m.device)
    m._bind_stream()
    for i in range(layers):
        check(lib().mmd_kv_debug_read(cache.arena.h, i, n64, _ptr(K[i]), _ptr(V[i])), m._ctx, 'mmd_kv_debug_read')
    Vl = torch.stack([v_logical(V[i]) for i in range(layers)])
    return K[:, :, lo:hi].clone(), Vl[:, :, lo:hi].clone()          # (slots behind `hi` in the last 64-token block hold whatever the arena held before)


def _plans(m):
    """what the most recent step, tower run, attention launch and generate call of this context took -- host-side records, read after the run has finished"""
    form = (C.c_int * 2)()
    lib().mmd_op_attention_last_form(m._ctx, form)
    # (decode route: 0 eager launches, else the captured step was replayed -- whether it was also captured in that call, 2, depends on what ran before, not on the schedule)
    return dict(step=m.step_last_plan(), tower=m.tower_last_plan(), attention=list(form), decode_replayed=m.decode_last_route() > 0)


def _context(m, x):
    c = None
    for s0 in range(0, x.shape[0], 1024):
        c = m(inputs_embeds=x[None, s0:s0 + 1024], past_key_values=c).past_key_values
    return c


# ---- tower jobs ------------------------------------------------------------------------------------------------------------------------------------
# name -> (frames per batch, fused uint8 entry?, ring-grid cap of the burst form, batches).  Three 35-frame batches keep the tower busy for the whole decoder job; a 3-frame
# batch (short ring, compact last layer) and a 1-frame batch are launch-bound, so more of them are enqueued for the host to stay ahead of the device.  The 1-frame batch (a
# clip of 35 n + 1 frames, the demo's frame-by-frame input) is the ONE tower shape that leaves split-K slabs in v_splitk_ws: its projector GEMMs have 196 rows and run on the
# weight-streaming kernel with 3 and 8 K slabs + a reduce launch; every GEMM of a larger batch writes its output tile directly (gemm_plan.h; asserted below).
TOWER_JOBS = {'fused35': (35, True, 0, 3), 'pixels35': (35, False, 0, 3), 'burst35': (35, True, 128, 3), 'fused3': (3, True, 0, 24), 'fused1': (1, True, 0, 32)}


class TowerJob:
    def __init__(self, m, name, more=1.0):
        self.m, self.name = m, name
        self.nf, self.fused, self.share, self.batches = TOWER_JOBS[name]
        self.batches = int(-(-self.batches * more // 1))          # (the token loops, one host round trip per token, outlast three batches: they get more)
        g = torch.Generator(device=m.device).manual_seed(100 + self.nf)
        n = self.nf * self.batches
        if self.fused:          # 336-px uint8 frames through the fused preprocess entry (Pillow-exact bicubic resample to 384 inside the patch-embed load)
            self.src = torch.randint(0, 256, (n, 3, 336, 336), dtype=torch.uint8, generator=g, device=m.device)
        else:
            self.src = torch.randn(n, 3, 384, 384, generator=g, device=m.device).to(torch.bfloat16)
        self.out = torch.empty(n * 49, H, dtype=m.dtype, device=m.device)

    def enqueue(self):
        """the batches back to back on the current stream, each into its own slice of the output buffer"""
        m, nf = self.m, self.nf
        if self.share:
            m.set_tower_share(self.share)
        try:
            for b in range(self.batches):
                src, out = self.src[b * nf:(b + 1) * nf], self.out[b * nf * 49:(b + 1) * nf * 49]
                (m.visual_embed_frames if self.fused else m.visual_embed)(src, out=out)
        finally:
            if self.share:
                m.set_tower_share(0)


# ---- decoder jobs ----------------------------------------------------------------------------------------------------------------------------------
def _rnd(m, g, n):
    return (torch.randn(n, H, generator=g, device=m.device) * 0.5).to(torch.bfloat16)


class ChunkStep:
    """(a) a 26-frame chunk with an 8-row text prefix (S = 1282) over 2000 cached keys through frame_step: tile / ring GEMMs, split-K down_proj whose slabs go to the fused
    residual + RMSNorm pass, chunk attention with partials, the chunk RoPE table, the sparse last layer"""
    expect = dict(step=dict(schedule=0, chunk_rope=1, down_slab_norm=1))
    tower_batches = 1.0          # x the tower job's batches, so that the tower is busy for the whole decoder job

    def __init__(self, m):
        g = torch.Generator(device=m.device).manual_seed(21)
        self.m, self.n0 = m, 2000
        self.base = _context(m, _rnd(m, g, self.n0))
        self.x = _rnd(m, g, 8 + 26 * 49)
        self.rows = [8 + 49 * (j + 1) - 1 for j in range(26)]

    def run(self):
        m = self.m
        heads, _ = m.frame_step(self.x[None], m.cache_prefix(self.base, self.n0), self.rows)
        # ... and the same rows once more through the forward that returns every row's final hidden state (no sparse last layer) and the last row's lm logits
        out = m(inputs_embeds=self.x[None], past_key_values=m.cache_prefix(self.base, self.n0))
        self.cache = out.past_key_values
        return dict(heads=heads, hidden=out.hidden_states[0].clone(), logits=out.logits[0, -1].clone())

    def after(self):
        K, V = _kv_rows(self.m, self.cache, self.n0)
        return dict(K=K, V=V, kv_len=len(self.cache))


class FrameStep(ChunkStep):
    """(b) one frame (S = 49) over 4116 keys: the w1 attention form with key splits, the stream GEMM slabs and the slab consumers"""
    expect = dict(step=dict(schedule=1), attention_form=5)

    def __init__(self, m):
        g = torch.Generator(device=m.device).manual_seed(22)
        self.m, self.n0 = m, 4116
        self.base = _context(m, _rnd(m, g, self.n0))
        self.x = _rnd(m, g, 49)
        self.rows = [48]


class Generate:
    """(c) / (f) greedy_generate of 16 tokens behind 1000 keys with a repetition penalty and log-probability records: the decode steps (eager launches, or the replayed captured
    step in a context created for it), the GEMV chain, rope_tab, chain_ssq, the arg-max scratch, the penalty list, the record buffers"""
    expect = dict(step=dict(schedule=2))
    tower_batches = 5 / 3

    def __init__(self, m):
        g = torch.Generator(device=m.device).manual_seed(23)
        self.m, self.n0 = m, 1000
        self.base = _context(m, _rnd(m, g, self.n0))
        self.prompt = _rnd(m, g, 5)

    def run(self):
        m = self.m
        seen = [3, 5]
        m.set_generate_logprobs(2)
        try:
            ids, self.cache = m.greedy_generate(self.prompt, m.cache_prefix(self.base, self.n0), -1, 16, 1.15, seen)
            lp = m.last_generate_logprobs()
        finally:
            m.set_generate_logprobs(-1)
        assert len(ids) == 16
        return dict(ids=ids, seen=seen, **{k: v.clone() for k, v in lp.items()})

    def after(self):
        K, V = _kv_rows(self.m, self.cache, self.n0)
        return dict(K=K, V=V, kv_len=len(self.cache))


class Rounds:
    """(d) round_multi with four streams behind 63 / 257 / 1000 / 1000 rows: a prompt round and eight feed rounds -- the batched decode attention (form 9), the seg_dev slot
    rotation (nine uploads through eight slots), the round_* buffers; sampler 0 penalises, sampler 1 draws with a fixed seed, sampler 2 records log-probabilities"""
    expect = dict(step=dict(run_n=4, run_all=1), attention_form=9)
    tower_batches = 5 / 3
    LENS = (63, 257, 1000, 1000)

    def __init__(self, m):
        g = torch.Generator(device=m.device).manual_seed(24)
        self.m = m
        self.bases = [_context(m, _rnd(m, g, n)) for n in self.LENS]
        self.prompts = [_rnd(m, g, n) for n in (4, 6, 4, 5)]
        self.smp = [m.new_sampler() for _ in self.LENS]

    def run(self):
        m, smp = self.m, self.smp
        smp[0].begin(-1, 1.15, [3, 5], 16)
        smp[1].begin(-1, None, None, 16, sampling=dict(temperature=0.8, top_k=50, top_p=0.9, seed=1234, restart=True))
        smp[2].begin(-1, None, None, 16); smp[2].set_logprobs(2)
        smp[3].begin(-1, None, None, 16)
        caches = [m.cache_prefix(b, n) for b, n in zip(self.bases, self.LENS)]
        toks = []
        for r in range(9):
            if r == 0:
                segs = [dict(x=p, cache=c, sampler=s, sample=True) for p, c, s in zip(self.prompts, caches, smp)]
            else:
                segs = [dict(x=None, cache=c, sampler=s, feed=True, sample=True) for c, s in zip(caches, smp)]
            out = m.round_multi(segs)
            caches = [o['cache'] for o in out]
            toks.append([o['token'] for o in out])
        self.caches = caches
        lp = smp[2].read_logprobs()
        return dict(tokens=toks, **{k: v.clone() for k, v in lp.items()})

    def after(self):
        res = dict(kv_len=[len(c) for c in self.caches])
        for i, (c, n) in enumerate(zip(self.caches, self.LENS)):
            res[f'K{i}'], res[f'V{i}'] = _kv_rows(self.m, c, n)
        return res


class TokenNll:
    """(e) token_nll on 64 hidden rows, in one pass over the vocabulary and in four forced column chunks: nll_ws, the rows' running state and the chunk partials"""
    expect = {}
    tower_batches = 1.0

    def __init__(self, m):
        g = torch.Generator(device=m.device).manual_seed(25)
        self.m = m
        self.hid = _rnd(m, g, 64)
        self.labels = torch.randint(0, m.config.vocab_size, (64,), generator=g, device=m.device)
        self.labels[5] = -100

    def run(self):
        nll, lse = self.m.token_nll(self.hid, self.labels, return_lse=True)
        nll4, lse4 = self.m.token_nll(self.hid, self.labels, return_lse=True, chunk_cols=512)
        return dict(nll=nll, lse=lse, nll4=nll4, lse4=lse4)

    def after(self):
        return {}


DECODER_JOBS = dict(chunk=ChunkStep, frame=FrameStep, generate=Generate, rounds=Rounds, nll=TokenNll)
MODELS = dict(bf16='width2', fp8='width2_fp8', graph='width2_graph')

# every decoder job beside the 35-frame fused tower job; the chunk step and the token loop also beside the other three; the token loop once more on the fp8-weight build and once
# in a context that replays the captured decode step
CASES = [('bf16', d, 'fused35') for d in DECODER_JOBS] + [('bf16', d, t) for d in ('chunk', 'generate') for t in ('pixels35', 'burst35', 'fused3')] + \
        [('fp8', 'generate', 'fused35'), ('graph', 'generate', 'fused35')] + \
        [('bf16', d, 'fused1') for d in ('chunk', 'frame', 'generate')]          # split-K slabs live in both workspaces at once: the decoder's jobs that leave slabs in splitk_ws


def _check_expect(expect, plans):
    for k, v in expect.get('step', {}).items():
        assert plans['step'][k] == v, (k, plans['step'])
    if 'attention_form' in expect:
        assert plans['attention'][0] == expect['attention_form'], plans['attention']


def _beside(main, side, tower_fn, decoder_fn):
    """The tower job enqueued on `side` as LiveInferForBenchmark._issue_vit does it -- side.wait_stream(main), the job, an event behind it -- and the decoder job on `main`, no
    host synchronisation between the two; each bracketed by timing events on its own stream.  -> (what decoder_fn returned, (tower start, tower end, decoder start, decoder end)
    in ms behind one common reference event, whether the two intervals intersect)"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ev[0].record(main)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        ev[1].record(side)
        tower_fn()
        ev[2].record(side)
        done = torch.cuda.Event()
        done.record(side)
    ev[3].record(main)
    got = decoder_fn()
    ev[4].record(main)
    main.wait_event(done)
    torch.cuda.synchronize()
    t0, t1, d0, d1 = (ev[0].elapsed_time(e) for e in ev[1:])
    return got, (round(t0, 3), round(t1, 3), round(d0, 3), round(d1, 3)), t0 < d1 and d0 < t1


def _overlapping_stream(m, priority):
    """A side stream of `priority` whose work really runs beside the current stream's.  The runtime deals streams onto a few hardware queues (four by default); a stream that
    lands on the current stream's queue runs strictly behind it -- measured here: every fourth stream of torch's pool, the whole tower job first and only then the decoder's
    first kernel -- and two jobs that never run together cannot show a shared buffer.  Streams are taken until a tower job and a small kernel on the current stream overlap."""
    main = torch.cuda.current_stream(m.device)
    tj = TowerJob(m, 'fused35')
    x = torch.zeros(1 << 22, device=m.device)
    tj.enqueue()
    torch.cuda.synchronize()
    seen, keep = [], []
    for _ in range(8):
        side = torch.cuda.Stream(device=m.device, priority=priority)
        keep.append(side)
        _, span, ok = _beside(main, side, tj.enqueue, lambda: x.add_(1.0))
        seen.append(span)
        if ok:
            return side
    pytest.fail(f'no stream of priority {priority} overlapped the current stream: {seen}')


@pytest.fixture(scope='module')
def side_stream(width2):
    """the lowest priority, as LiveInferForBenchmark creates its tower stream"""
    return _overlapping_stream(width2, torch.cuda.Stream.priority_range()[0])


@pytest.mark.parametrize('model,decoder,tower', CASES, ids=[f'{d}-beside-{t}' + ('' if mo == 'bf16' else f'-{mo}') for mo, d, t in CASES])
def test_concurrent_pair_equals_serialized_bit_for_bit(request, side_stream, model, decoder, tower):
    m = request.getfixturevalue(MODELS[model])
    dj = DECODER_JOBS[decoder](m)
    tj = TowerJob(m, tower, dj.tower_batches)
    main, side = torch.cuda.current_stream(m.device), side_stream
    # once unobserved: what is allocated at a first use, and the capture of the decode step, happen here (the step and attention records below are written when a step is
    # planned and launched, not when a captured one is replayed)
    dj.run()
    torch.cuda.synchronize()

    # serialized: the expected bits and plans
    tj.out.zero_()
    tj.enqueue()
    torch.cuda.synchronize()
    want_tower = tj.out.clone()
    gemm_plan = (C.c_int * 4)()
    lib().mmd_op_gemm_last_plan(m._ctx, gemm_plan)          # the tower's last GEMM, the projector's second linear: (kernel, tiles, splits, blocks)
    assert (gemm_plan[2] > 1) == (tower == 'fused1'), list(gemm_plan)
    want = dj.run()
    torch.cuda.synchronize()
    want.update(dj.after())
    want_plans = _plans(m)
    assert want_plans['decode_replayed'] == (model == 'graph'), want_plans          # the captured step is replayed exactly where the context was created for it
    if model != 'graph':
        _check_expect(dj.expect, want_plans)
    assert torch.isfinite(want_tower.float()).all()
    nb = tj.nf * 49
    assert all(not torch.equal(want_tower[b * nb:(b + 1) * nb], want_tower[:nb]) for b in range(1, tj.batches))          # every batch has its own frames

    # concurrent
    overlapped, spans = 0, []
    for r in range(REPEATS):
        tj.out.zero_()
        got, span, ok = _beside(main, side, tj.enqueue, dj.run)
        got.update(dj.after())
        plans = _plans(m)
        spans.append(span)
        overlapped += int(ok)
        assert _same(tj.out, want_tower), (r, 'tower output', _first_difference(tj.out, want_tower), span)
        assert sorted(got) == sorted(want)
        for k in want:
            assert _same(got[k], want[k]), (r, k, _first_difference(got[k], want[k]), span)
        assert plans == want_plans, (r, plans, want_plans)
    print(f'\n{decoder} beside {tower} [{model}]: {overlapped} of {REPEATS} repeats overlapped; (tower start, tower end, decoder start, decoder end) in ms: {spans}')
    assert overlapped >= MIN_OVERLAPPED, (overlapped, spans)


# ---- the shipped schedules -------------------------------------------------------------------------------------------------------------------------
QUERY = 'Please narrate the video in real time.'[:24]
T_FRAMES = 60


def _args(k, overlap=True):
    from mmduet_amd.arguments_live import LiveTestArguments
    # threshold 1.0: a score never exceeds it, so the responses are exactly the pinned frames' (the driver class bench.py times: the decision rule runs, the firing frames are fixed)
    return LiveTestArguments(llm_pretrained='synthetic:bench', frame_fps=1.0, bf16=True, stream_end_prob_threshold=1.0, score_heads='informative_score', max_new_tokens=16,
                             frames_per_forward=k, overlap_vision=overlap, system_prompt='A multimodal AI assistant is helping users with some activities.')


def _clip(dev, seed):
    return torch.randint(0, 256, (T_FRAMES, 3, 336, 336), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(dev)


def _stream_result(m, scores, ids, cache):
    K, V = _kv_rows(m, cache, 0)
    return dict(scores=scores, ids=[list(x) for x in ids], kv_len=len(cache), K=K, V=V)


def _assert_same_result(a, b, what):
    assert a['scores'] == b['scores'], (what, 'scores', [i for i, (x, y) in enumerate(zip(a['scores'], b['scores'])) if x != y])
    assert a['ids'] == b['ids'], (what, 'response ids', a['ids'], b['ids'])
    assert a['kv_len'] == b['kv_len'], (what, a['kv_len'], b['kv_len'])
    for k in ('K', 'V'):
        assert _same(a[k], b[k]), (what, k, _first_difference(a[k], b[k]))


N_TOWER_BATCHES = -(-T_FRAMES // DRIVER_VIT_BATCH)


def test_single_stream_tower_schedules_give_identical_results_true_width(width2_drivers):
    """LiveInferForBenchmark, k = 13, under the five tower schedules of tests/test_gpu_streams.py::test_tower_schedule_does_not_change_results: all five batches up front on the
    side stream; one batch ahead with a burst of up to three capped-grid batches (128 workgroups) beside a response; one batch ahead with one capped batch (32 workgroups) per
    response; issued only when needed; on the LLM's own stream.  The responses are pinned to frames 5 and 17, while batches are still unissued, and one burst batch is sized to
    5 expected tokens (the driver's default, 10, would cut a 16-token response's burst to one batch in both burst schedules).  That each schedule really ran is asserted: the
    batches issued before the first forward, and the grid caps the bursts set."""
    import bench as B
    from mmduet_amd.tokenization_live import build_live_tokenizer_and_update_config
    m = width2_drivers
    side = _overlapping_stream(m, torch.cuda.Stream.priority_range()[0])
    tok = build_live_tokenizer_and_update_config('synthetic:bench', m.config)
    frames = _clip(m.device, 1)
    runs, seen = [], []
    scheds = (dict(vit_burst_batches=0), dict(vit_burst_batches=3, vit_burst_blocks=128), dict(vit_burst_batches=1, vit_burst_blocks=32),
              dict(vit_burst_batches=0, vit_lookahead_batches=0), dict(overlap_vision=False))
    real_share = m.set_tower_share
    for sched in scheds:
        caps = []
        m.set_tower_share = lambda blocks, caps=caps: (caps.append(int(blocks)), real_share(blocks))[1]
        try:
            d = B.bench_driver_class()(_args(13), model=m, tokenizer=tok)
            d.forced_frames, d.eos_token_id, d.vit_burst_tokens_per_batch = frozenset((5, 17)), -1, 5
            d._vit_stream = side          # (the driver creates its own lowest-priority stream when it has none: this one is known to run beside the LLM's)
            for key, v in sched.items():
                setattr(d, key, v)
            d.reset()
            d.input_video_stream(frames)
            at_start = len(d._vit_events)
            d.input_query_stream([{'role': 'user', 'content': QUERY, 'time': 0.0}])
            d.inference()
            torch.cuda.synchronize()
        finally:
            del m.set_tower_share          # (the instance attribute: the method is back)
        assert len(d.debug_data_list) == T_FRAMES and [len(x) for x in d.response_token_ids] == [16, 16]
        seen.append((at_start, len(d._vit_events), caps))
        runs.append(_stream_result(m, [(x['informative_score'], x['relevance_score']) for x in d.debug_data_list], d.response_token_ids, d.past_key_values))
        del d
    print(f'\n(batches issued before the first forward, at the end, set_tower_share calls) per schedule: {seen}')
    n = N_TOWER_BATCHES
    assert seen[0] == (n, n, [])                                                      # everything up front, full grids
    assert seen[1][:2] == (2, n) and 128 in seen[1][2] and set(seen[1][2]) == {128, 0} and seen[1][2][-1] == 0          # one ahead; a burst under the 128-workgroup cap, cap lifted behind it
    assert seen[2][:2] == (2, n) and 32 in seen[2][2] and set(seen[2][2]) == {32, 0} and seen[2][2][-1] == 0
    assert seen[3] == (1, n, [])                                                      # only the batch the first forward needs; the rest during the run
    assert seen[4] == (0, 0, [])                                                      # no side stream at all
    for i, r in enumerate(runs[1:], 1):
        _assert_same_result(r, runs[0], f'schedule {i}')


def _multi_pass(m, tok, clips, side, overlap=True, lookahead=2):
    import bench as B
    from mmduet_amd.multistream import MultiStreamInfer
    sink = {}

    class Rec(B.bench_driver_class()):
        def input_video_stream(self, video_frames):
            r = super().input_video_stream(video_frames)
            self.issued_at_start = len(self._vit_events)
            return r

        def inference(self):
            r = super().inference()
            sink[self.sink_key] = self
            return r

    videos = [dict(frames=fr, conversation=[{'role': 'user', 'content': QUERY, 'time': 0.0}],
                   driver_attrs=dict(forced_frames=frozenset(random.Random(s).sample(range(1, T_FRAMES + 1), 2)), eos_token_id=-1, sink_key=s)) for s, fr in enumerate(clips)]
    ms = MultiStreamInfer(_args(MULTI_K, overlap), model=m, tokenizer=tok, n_slots=MULTI_SLOTS, driver_cls=Rec, vit_lookahead_batches=lookahead)
    ms.keep_drivers = True          # the arenas are read below
    ms._vit_stream = side           # (the scheduler creates its one tower stream, priority 0, when it has none: this one is known to run beside the LLM's)
    results = ms.run(videos)
    torch.cuda.synchronize()
    assert ms.rounds < sum(r['forward_calls'] + sum(len(g) for g in r['response_token_ids']) for r in results)          # the forwards really were shared
    out = []
    for s, r in enumerate(results):
        assert len(r['debug_data']) == T_FRAMES and [len(x) for x in r['response_token_ids']] == [16, 16]
        # the schedule really ran: `lookahead` batches beyond the first before the first forward, the others issued between the forwards; none with the tower on the LLM stream
        assert (sink[s].issued_at_start, len(sink[s]._vit_events)) == ((lookahead + 1, N_TOWER_BATCHES) if overlap else (0, 0)), (s, sink[s].issued_at_start, len(sink[s]._vit_events))
        out.append(_stream_result(m, [(x['informative_score'], x['relevance_score']) for x in r['debug_data']], r['response_token_ids'], sink[s].past_key_values))
        assert out[-1]['kv_len'] == r['final_kv_len']
    for d in sink.values():
        d.past_key_values = None
    return out


def test_multi_stream_lookahead_schedule_repeats_bit_identical_true_width(width2_drivers):
    """MultiStreamInfer with 4 slots, k = 13, the tower two batches ahead (three of a clip's five batches issued before its first forward, the others between the forwards of
    the run) on ONE side stream shared by the slots, responses decoding in native rounds: the pass five times over,
    every repeat identical to the first in every stream's scores, response ids and final KV bits; and identical to the pass with the tower on the LLM's stream and to the pass
    with the tower issued only when needed."""
    from mmduet_amd.tokenization_live import build_live_tokenizer_and_update_config
    m = width2_drivers
    tok = build_live_tokenizer_and_update_config('synthetic:bench', m.config)
    clips = [_clip(m.device, 1 + s) for s in range(MULTI_SLOTS)]          # every stream its own frames: rows of two streams mixed up in a shared forward cannot cancel out
    side = _overlapping_stream(m, 0)
    first = _multi_pass(m, tok, clips, side)
    assert all(first[a]['scores'] != first[b]['scores'] for a in range(MULTI_SLOTS) for b in range(a + 1, MULTI_SLOTS))
    for rep in range(1, 5):
        for s, (a, b) in enumerate(zip(_multi_pass(m, tok, clips, side), first)):
            _assert_same_result(a, b, f'repeat {rep}, stream {s}')
    for what, kw in (('tower on the LLM stream', dict(overlap=False)), ('tower issued when needed', dict(lookahead=0))):
        for s, (a, b) in enumerate(zip(_multi_pass(m, tok, clips, side, **kw), first)):
            _assert_same_result(a, b, f'{what}, stream {s}')
