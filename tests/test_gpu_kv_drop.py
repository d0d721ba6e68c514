"""Sliding context window on the device: mmd_kv_drop moves the arena bit for bit (host statement: tests/kv_drop_cases.py), refuses what it must, and every step
afterwards writes slot `len` at RoPE position `len + dropped` -- single steps, both decode routes, several streams per step, truncate / stash, and the drivers.
Arena forms: a stream's arena stores V in transposed 64-token blocks in both dtypes (plain V rows exist only in the operator-level entry points, which own no
stream), so the two forms the library has are the bf16 and the fp32 arena of the models tests/test_gpu_kv_arena.py uses."""
import pytest
import torch

pytestmark = pytest.mark.gpu
import kv_layout as L
import kv_drop_cases as D
from oracle import duet_oracle as O
from mmduet_amd._lib import lib, check, MmduetError
from mmduet_amd.modeling_live import _ptr
from helpers import hip_model, oracle_model, make_args, tokenizer_for, stream_cases, stream_frames

BF = torch.bfloat16
F32_TOL = 3e-4          # tests/test_gpu_model.py: fp32 HIP path vs the fp32 oracle


@pytest.fixture(scope='module')
def bf16_model():
    """the 2-layer true-width bf16 model of tests/test_gpu_kv_arena.py (nkv 4, d 128), captured decode step on"""
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    ocfg = O.OracleConfig(vocab_size=2048, num_hidden_layers=2, vit_layers=1)
    w = O.random_weights(ocfg, seed=3, dtype=BF, scale='unit')
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=2, vit_num_hidden_layers=2, vit_layers_removed=1,
                                        frame_num_tokens=49, frame_resolution=384, v_placeholder='<image>')
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('MMDUET_GRAPH', '1')
        m = VideoHeadLiveLlavaQwenForCausalLM(pcfg, torch_dtype=BF, max_vit_batch=1, max_step_tokens=1024, kv_initial_tokens=1024)
    m.load_state_dict(w)
    return m, w, ocfg


@pytest.fixture(scope='module')
def f32_model():
    """the fp32 tiny model (nkv 2, d 16) and its oracle"""
    m = hip_model('A', torch.float32)[0]
    om, _, w = oracle_model('A')
    return m, om.w, om.cfg


def rand(g, rows, H, dtype):
    return (torch.randn(1, rows, H, generator=g) * 0.5).to(dtype)


def up64(n):
    return -(-n // L.BLK) * L.BLK


def snapshot(m, cache, n):
    """-> (K [layers, nkv, n, d], V as stored [layers, nkv, n / 64, d, 64]) of the first n (a multiple of 64) slots"""
    c = m.config
    layers, nkv, d = c.num_hidden_layers, c.num_key_value_heads, c.head_dim
    K = torch.empty(layers, nkv, n, d, dtype=m.dtype, device=m.device)
    V = torch.empty(layers, nkv, n // L.BLK, d, L.BLK, dtype=m.dtype, device=m.device)
    m._bind_stream()
    for i in range(layers):
        check(lib().mmd_kv_debug_read(cache.arena.h, i, n, _ptr(K[i]), _ptr(V[i])), m._ctx, 'mmd_kv_debug_read')
    return K, V


def ibits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same(a, b):
    return torch.equal(ibits(a), ibits(b))


def assert_arena(m, cache, want_k, want_v, what):
    """the live tokens of every layer equal the host statement exactly"""
    n = want_k[0].shape[1]
    assert len(cache) == n == int(lib().mmd_kv_len(cache.arena.h)), what
    if n == 0:
        return
    K, V = snapshot(m, cache, up64(n))
    for i in range(K.shape[0]):
        assert same(K[i][:, :n], want_k[i]), f'{what}: layer {i} K differs in {int((ibits(K[i][:, :n]) != ibits(want_k[i])).sum())} elements'
        got_v = L.v_logical(V[i])[:, :n]
        assert same(got_v, want_v[i]), f'{what}: layer {i} V differs in {int((ibits(got_v) != ibits(want_v[i])).sum())} elements'


def run_arena_case(m, case):
    frm, to, n = case
    H = m.config.hidden_size
    g = torch.Generator(device='cuda').manual_seed(frm * 31 + to * 7 + n)
    x = (torch.randn(1, n, H, generator=g, device='cuda') * 0.5).to(m.dtype)
    cache = m(inputs_embeds=x).past_key_values          # filled by real steps (max_step_tokens rows each)
    del x
    assert len(cache) == n
    K, V = snapshot(m, cache, up64(n))
    layers = K.shape[0]
    want = [D.expected_arena(K[i], V[i], frm, to, n) for i in range(layers)]
    pos = m.kv_position(cache)
    cache = m.kv_drop(cache, frm, to)
    assert m.kv_position(cache) == pos == n
    wk, wv = [w[0] for w in want], [w[1] for w in want]
    assert_arena(m, cache, wk, wv, f'drop {case}')
    # a second drop composes with the first
    n1 = n - (to - frm)
    if n1 >= 2:
        f2 = n1 // 3; t2 = min(n1, f2 + 65) if n1 > 200 else min(n1 - 1, f2 + 3)
        cache = m.kv_drop(cache, f2, t2)
        assert m.kv_position(cache) == n
        assert_arena(m, cache, [D.drop_rows(k, f2, t2) for k in wk], [D.drop_rows(v, f2, t2) for v in wv], f'drop {case}, then [{f2}, {t2})')


@pytest.mark.parametrize('case', D.CASES, ids=lambda c: '-'.join(map(str, c)))
def test_arena_bf16_bit_for_bit(bf16_model, case):
    run_arena_case(bf16_model[0], case)
    if case[2] >= D.BIG_LEN:
        bf16_model[0].release_pooled_arenas()


@pytest.mark.parametrize('case', [c for c in D.CASES if c[2] < D.BIG_LEN], ids=lambda c: '-'.join(map(str, c)))
def test_arena_fp32_bit_for_bit(f32_model, case):
    run_arena_case(f32_model[0], case)


def test_refusals_change_nothing(f32_model):
    m = f32_model[0]
    H = m.config.hidden_size
    g = torch.Generator().manual_seed(1)
    cache = m(inputs_embeds=rand(g, D.REFUSAL_LEN, H, m.dtype).cuda()).past_key_values
    cache = m.kv_drop(cache, 3, 5)          # a position offset to keep
    cache = m(inputs_embeds=rand(g, 2, H, m.dtype).cuda(), past_key_values=cache).past_key_values
    h = cache.arena.h
    before = snapshot(m, cache, 128)

    def unchanged():
        after = snapshot(m, cache, 128)
        return int(lib().mmd_kv_len(h)) == D.REFUSAL_LEN and int(lib().mmd_kv_position(h)) == D.REFUSAL_LEN + 2 and same(before[0], after[0]) and same(before[1], after[1])
    assert unchanged()
    for (f, t), code in D.REFUSED_RANGES:
        assert lib().mmd_kv_drop(h, f, t) == code, (f, t)
        assert unchanged(), (f, t)
    assert lib().mmd_kv_drop(None, 0, 1) == D.MMD_EINVAL and lib().mmd_kv_position(None) == -1
    with pytest.raises(ValueError):
        m.kv_drop(cache, 5, D.REFUSAL_LEN + 1)
    # while a stash is held: refused, whatever the span; after the unstash: accepted
    stash = m.kv_stash(cache, 60)
    assert lib().mmd_kv_drop(h, 10, 20) == D.MMD_EINVAL and lib().mmd_kv_drop(h, 70, 80) == D.MMD_EINVAL and lib().mmd_kv_drop(h, 4, 4) == D.MMD_EINVAL
    assert unchanged()
    with pytest.raises(MmduetError, match='stash'):
        m.kv_drop(cache, 10, 20)
    cache = m.kv_unstash(stash)
    assert unchanged()
    assert lib().mmd_kv_drop(h, 4, 4) == D.MMD_OK and unchanged()          # from == to: nothing
    assert lib().mmd_kv_drop(h, 10, 20) == D.MMD_OK
    assert int(lib().mmd_kv_len(h)) == D.REFUSAL_LEN - 10 and int(lib().mmd_kv_position(h)) == D.REFUSAL_LEN + 2
    # truncate leaves the offset alone, reset zeroes it
    assert lib().mmd_kv_truncate(h, 50) == 0 and int(lib().mmd_kv_position(h)) == 50 + 12
    assert lib().mmd_stream_reset(h) == 0 and int(lib().mmd_kv_position(h)) == 0 and int(lib().mmd_kv_len(h)) == 0


# ---- positions ---------------------------------------------------------------------------------------------------------------------------------------------
N0, A, B = 150, 10, 110


@pytest.fixture(scope='module')
def dropped_prefix(f32_model):
    """the oracle's handle of a 150-token prefix with [10, 110) sliced out, and the prefix itself"""
    m, w, cfg = f32_model
    x0 = rand(torch.Generator().manual_seed(21), N0, cfg.hidden_size, torch.float32)
    _, kv = O.llm_forward(w, cfg, x0[0], None)
    return x0, D.drop_handle(kv, A, B)


def hip_dropped(m, x0):
    return m.kv_drop(m(inputs_embeds=x0.cuda()).past_key_values, A, B)


def maxerr(a, b):
    return (a.float().cpu() - b.float().cpu()).abs().max().item()


@pytest.mark.parametrize('S', [1, 7, 70])
def test_positions_after_a_drop(f32_model, dropped_prefix, S):
    m, w, cfg = f32_model
    x0, kvd = dropped_prefix
    x = rand(torch.Generator().manual_seed(100 + S), S, cfg.hidden_size, torch.float32)
    want, _ = D.oracle_step_at(w, cfg, x[0], kvd, N0)
    renumbered, _ = D.oracle_step_at(w, cfg, x[0], kvd, N0 - (B - A))
    disc = maxerr(want, renumbered)
    print(f'S {S}: oracle at true positions vs renumbered positions differ by {disc:.4g}')
    assert disc >= 100 * F32_TOL          # the check below can tell the two apart
    cache = hip_dropped(m, x0)
    assert len(cache) == N0 - (B - A) and m.kv_position(cache) == N0
    out = m(inputs_embeds=x.cuda(), past_key_values=cache)
    err = maxerr(out.hidden_states[0], want)
    print(f'S {S}: max |hidden - oracle| = {err:.4g}')
    assert err < F32_TOL
    assert len(out.past_key_values) == N0 - (B - A) + S and m.kv_position(out.past_key_values) == N0 + S


def test_truncate_then_step_after_a_drop(f32_model, dropped_prefix):
    """roll back to a point behind the dropped span, step: the position goes back with the length (offset kept)"""
    m, w, cfg = f32_model
    x0, kvd = dropped_prefix
    H = cfg.hidden_size
    g = torch.Generator().manual_seed(5)
    x1, x2 = rand(g, 9, H, torch.float32), rand(g, 5, H, torch.float32)
    cache = hip_dropped(m, x0)
    base = len(cache)
    longer = m(inputs_embeds=x1.cuda(), past_key_values=cache).past_key_values
    back = m.cache_prefix(longer, base + 4)          # keep 4 of the 9
    out = m(inputs_embeds=x2.cuda(), past_key_values=back)
    _, kv1 = D.oracle_step_at(w, cfg, x1[0, :4], kvd, N0)
    want, _ = D.oracle_step_at(w, cfg, x2[0], kv1, N0 + 4)
    assert m.kv_position(out.past_key_values) == N0 + 4 + 5
    assert maxerr(out.hidden_states[0], want) < F32_TOL


def test_fp32_greedy_after_drops_equals_oracle(f32_model, dropped_prefix):
    """the eager decode of the fp32 model: greedy and top-k-1 sampled ids after a drop, and after a second drop between two responses, equal the oracle's"""
    m, w, cfg = f32_model
    x0, kvd = dropped_prefix
    prompt = rand(torch.Generator().manual_seed(6), 3, cfg.hidden_size, torch.float32)
    want1, gap1, kv1 = D.oracle_greedy_at(w, cfg, prompt[0], kvd, N0, 5)
    want2, gap2, _ = D.oracle_greedy_at(w, cfg, prompt[0], D.drop_handle(kv1, 12, 31), N0 + 3 + 4, 5)
    assert min(gap1, gap2) > 10 * F32_TOL, (gap1, gap2)          # no near-tie in the oracle's own logits
    ids, cache = m.greedy_generate(prompt.cuda(), hip_dropped(m, x0), -1, 5)
    assert ids == want1 and m.kv_position(cache) == N0 + 3 + 4
    ids_s, _, _ = m.sample_generate(prompt.cuda(), hip_dropped(m, x0), -1, 5, temperature=1.0, top_k=1, top_p=1.0, seed=3, offset=0)
    assert ids_s == want1
    ids2, cache = m.greedy_generate(prompt.cuda(), m.kv_drop(cache, 12, 31), -1, 5)
    assert ids2 == want2 and m.kv_position(cache) == N0 + 2 * (3 + 4)


# ---- decode routes (bf16, head_dim 128: the captured step exists) ------------------------------------------------------------------------------------------
def test_decode_routes_agree_after_drops(bf16_model):
    """After a drop: the call-by-call loop, the captured greedy step and the captured sampled step (top-k 1) return the same ids; after a second drop between two
    responses the replayed graph picks the new offset up from device state without a re-capture.  All of them equal the greedy ids of the bf16 oracle composed at the
    true positions.  The seed and the second span were searched on the CPU so that the oracle's own top-2 gap exceeds the bf16 logits bound of
    tests/test_gpu_trueshape.py (2 x 6e-2) in front of every returned token of both responses (asserted below: 0.27 and 0.22), so equality of ids is decided by
    the positions, not by bf16 rounding; the second drop changes the oracle's second response.  The teacher-forced shortfall is printed and held as an extra."""
    from mmduet_amd.modeling_live import fast_greedy_generate
    m, w, ocfg = bf16_model
    H = m.config.hidden_size
    g = torch.Generator().manual_seed(1057)
    ctx, prompt = rand(g, 90, H, BF), rand(g, 5, H, BF)
    n_new, BOUND, SPAN2 = 4, 2 * 6e-2, (5, 50)

    def oracle_scores(past, pos0, ids):
        """teacher-forced: the oracle's logits in front of each returned id -> (worst shortfall of a returned id against the best, handle)"""
        x, worst = prompt[0], 0.0
        for t in ids:
            h, past = D.oracle_step_at(w, ocfg, x, past, pos0)
            pos0 += x.shape[0]
            lg = O.linear(h[-1:], w['lm_head.weight']).float()[0]
            worst = max(worst, float(lg.max() - lg[t]))
            x = w['model.embed_tokens.weight'][t][None]
        return worst, past

    def fresh():
        return m.kv_drop(m(inputs_embeds=ctx.cuda()).past_key_values, 20, 61)
    # eager: one forward per token
    out = torch.zeros(1, n_new, dtype=torch.long, device='cuda')
    m.python_generate_loop = True
    try:
        ids_e, cache_e, _ = fast_greedy_generate(model=m, inputs_embeds=prompt.cuda(), past_key_values=fresh(), eos_token_id=-1, inplace_output_ids=out)
    finally:
        m.python_generate_loop = False
    ids_e = ids_e[0].tolist()
    # captured
    ids_g, cache_g = m.greedy_generate(prompt.cuda(), fresh(), -1, n_new)
    assert m.decode_last_route() in (1, 2)
    ids_s, cache_s, _ = m.sample_generate(prompt.cuda(), fresh(), -1, n_new, temperature=1.0, top_k=1, top_p=1.0, seed=11, offset=0)
    assert m.decode_last_route() in (1, 2)
    assert ids_g == ids_e == ids_s, (ids_e, ids_g, ids_s)
    assert len(cache_g) == 90 - 41 + 5 + n_new - 1 and m.kv_position(cache_g) == 90 + 5 + n_new - 1
    _, kv = O.llm_forward(w, ocfg, ctx[0], None)
    want1, gap1, kv1 = D.oracle_greedy_at(w, ocfg, prompt[0], D.drop_handle(kv, 20, 61), 90, n_new)
    worst, _ = oracle_scores(D.drop_handle(kv, 20, 61), 90, ids_g)
    print(f'first response: oracle ids {want1}, smallest top-2 gap {gap1:.4g}; returned {ids_g}, worst shortfall against the oracle {worst:.4g}')
    assert gap1 > BOUND
    assert ids_g == want1
    assert worst < BOUND
    # drop again between two responses: same graph, new offset
    ids_g2, cache_g2 = m.greedy_generate(prompt.cuda(), m.kv_drop(cache_g, *SPAN2), -1, n_new)
    assert m.decode_last_route() == 1
    ids_s2, _, _ = m.sample_generate(prompt.cuda(), m.kv_drop(cache_s, *SPAN2), -1, n_new, temperature=1.0, top_k=1, top_p=1.0, seed=11, offset=0)
    assert m.decode_last_route() == 1
    m.python_generate_loop = True
    try:
        ids_e2, _, _ = fast_greedy_generate(model=m, inputs_embeds=prompt.cuda(), past_key_values=m.kv_drop(cache_e, *SPAN2), eos_token_id=-1, inplace_output_ids=out)
    finally:
        m.python_generate_loop = False
    assert ids_g2 == ids_e2[0].tolist() == ids_s2, (ids_e2, ids_g2, ids_s2)
    assert m.kv_position(cache_g2) == 90 + 2 * (5 + n_new - 1)
    want2, gap2, _ = D.oracle_greedy_at(w, ocfg, prompt[0], D.drop_handle(kv1, *SPAN2), 90 + 5 + n_new - 1, n_new)
    worst2, _ = oracle_scores(D.drop_handle(kv1, *SPAN2), 90 + 5 + n_new - 1, ids_g2)
    print(f'second response: oracle ids {want2}, smallest top-2 gap {gap2:.4g}; returned {ids_g2}, worst shortfall against the oracle {worst2:.4g}')
    assert gap2 > BOUND and want2 != want1
    assert ids_g2 == want2
    assert worst2 < BOUND


# ---- several streams per step ------------------------------------------------------------------------------------------------------------------------------
def test_multi_step_with_one_dropped_stream(f32_model):
    """mmd_frame_step_multi / mmd_round_multi: a stream with a dropped span and one without share steps; each equals its single-stream run (tolerances of
    tests/test_gpu_multistream.py)"""
    m = f32_model[0]
    H = m.config.hidden_size
    g = torch.Generator().manual_seed(8)
    pa, pb = (torch.randn(n, H, generator=g).cuda() * 0.3 for n in (120, 33))
    xa, xb = (torch.randn(n, H, generator=g).cuda() * 0.3 for n in (7, 12))

    def ctxs():
        return m.kv_drop(m(inputs_embeds=pa[None]).past_key_values, 5, 70), m(inputs_embeds=pb[None]).past_key_values
    ca, cb = ctxs()
    ra = m(inputs_embeds=xa[None], past_key_values=ca); rb = m(inputs_embeds=xb[None], past_key_values=cb)
    ca, cb = ctxs()
    out = m.multi_step([dict(x=xa, cache=ca, hidden='all'), dict(x=xb, cache=cb, hidden='all')])
    torch.testing.assert_close(out[0]['hidden'], ra.hidden_states[0], atol=2e-5, rtol=1e-5)
    torch.testing.assert_close(out[1]['hidden'], rb.hidden_states[0], atol=2e-5, rtol=1e-5)
    assert m.kv_position(out[0]['cache']) == 127 and m.kv_position(out[1]['cache']) == 45 and len(out[0]['cache']) == 62
    # a round: both streams draw a token from their last row, then feed it
    ca, cb = ctxs()
    sa, sb = m.new_sampler(), m.new_sampler()
    sa.begin(-1, None, None, 4); sb.begin(-1, None, None, 4)
    rnd = m.round_multi([dict(x=xa, cache=ca, sampler=sa, sample=True), dict(x=xb, cache=cb, sampler=sb, sample=True)])
    assert rnd[0]['token'] == int(ra.logits[0, -1].argmax()) and rnd[1]['token'] == int(rb.logits[0, -1].argmax())
    nxt = m.round_multi([dict(x=None, cache=rnd[0]['cache'], sampler=sa, feed=True, sample=True), dict(x=None, cache=rnd[1]['cache'], sampler=sb, feed=True, sample=True)])
    for i, r in enumerate((ra, rb)):
        e = m.get_input_embeddings()(torch.tensor([[rnd[i]['token']]], device=m.device)).view(1, 1, H)
        assert nxt[i]['token'] == int(m(inputs_embeds=e, past_key_values=r.past_key_values).logits[0, -1].argmax())
    assert m.kv_position(nxt[0]['cache']) == 128 and len(nxt[0]['cache']) == 63


def test_round_of_talking_streams_bf16_one_dropped(bf16_model):
    """the batched decode attention (one launch for the talking streams' rows, per-stream states on the device): a dropped stream among them draws what it draws alone"""
    m = bf16_model[0]
    H = m.config.hidden_size
    g = torch.Generator().manual_seed(9)
    ctx = [rand(g, n, H, BF).cuda() for n in (200, 64, 130)]
    rows = [rand(g, 1, H, BF).cuda() for _ in ctx]

    def caches():
        cs = [m(inputs_embeds=c).past_key_values for c in ctx]
        cs[0] = m.kv_drop(cs[0], 30, 101)
        return cs
    alone = [m(inputs_embeds=r, past_key_values=c) for r, c in zip(rows, caches())]
    smp = [m.new_sampler() for _ in ctx]
    for s in smp:
        s.begin(-1, None, None, 4)
    out = m.round_multi([dict(x=rows[i], cache=c, sampler=smp[i], sample=True) for i, c in enumerate(caches())])
    assert m.step_last_plan()['run_n'] == 3
    for i in range(3):
        lg = alone[i].logits[0, -1].float()
        assert float(lg.max() - lg[out[i]['token']]) < 2 * 6e-2, i          # (bf16: another attention form may move a near-tie)
    assert m.kv_position(out[0]['cache']) == 201 and len(out[0]['cache']) == 130


# ---- drivers -----------------------------------------------------------------------------------------------------------------------------------------------
class _Watch:
    """the model with the context length recorded behind every forward the driver issues"""

    def __init__(self, m):
        self.__dict__['_m'] = m; self.__dict__['lens'] = []

    def __getattr__(self, name):
        return getattr(self._m, name)

    def __setattr__(self, name, v):
        setattr(self._m, name, v)

    def frame_step(self, *a, **k):
        r = self._m.frame_step(*a, **k); self.lens.append(len(r[1])); return r

    def __call__(self, *a, **k):
        r = self._m(*a, **k); self.lens.append(len(r.past_key_values)); return r

    def greedy_generate(self, *a, **k):
        r = self._m.greedy_generate(*a, **k); self.lens.append(len(r[1])); return r


def run_driver(m, fpf, **window):
    from mmduet_amd.inference import LiveInferForBenchmark
    meta = stream_cases()
    case = meta['cases']['prob_keep']
    opts = case['opts']
    args = make_args(frame_fps=case['fps'], system_prompt=meta['system_prompt'], max_new_tokens=12, stream_end_prob_threshold=opts['stream_end_prob_threshold'],
                     score_heads=opts['score_heads'], frames_per_forward=fpf, **window)
    tok = tokenizer_for(m.config)                        # (the tokenizer builder writes its own eos into the config ...)
    m.config.eos_token_id = meta['eos_token_id']         # ... the fixture's synthetic "eos" goes in afterwards
    wm = _Watch(m)
    d = LiveInferForBenchmark(args, model=wm, tokenizer=tok)
    frames = stream_frames('prob_keep')
    d.input_video_stream(torch.cat([frames] * 4)[:40])
    d.input_query_stream(case['conversation'])
    responses = d.inference()
    return d, wm.lens, responses


@pytest.mark.parametrize('fpf', [1, 3])
def test_driver_holds_the_window(f32_model, fpf):
    m = f32_model[0]
    base, lens0, resp0 = run_driver(m, fpf)
    assert len(base.debug_data_list) == 40 and base.dropped_tokens == 0
    nt, sink = m.config.frame_num_tokens, base._sink_tokens
    # window absent, off, or wider than the whole stream: the same records, bit for bit
    for kw in (dict(context_window=0), dict(context_window=max(lens0) + 1000), dict(context_window=max(lens0) + 1000, context_sink=3)):
        d, lens, resp = run_driver(m, fpf, **kw)
        assert d.dropped_tokens == 0 and lens == lens0 and resp == resp0 and d.debug_data_list == base.debug_data_list and d.response_token_ids == base.response_token_ids
    # a window of the sink, a few chunks and a response: held after every forward
    window = sink + (fpf + 3) * nt + 40
    assert window < max(lens0)
    d, lens, resp = run_driver(m, fpf, context_window=window)
    print(f'fpf {fpf}: window {window}, sink {d._sink_tokens}, longest context {max(lens)} (unbounded run: {max(lens0)}), dropped {d.dropped_tokens}')
    assert d._sink_tokens == sink and d.dropped_tokens > 0
    assert max(lens) <= window, (max(lens), window)
    assert len(d.debug_data_list) == 40
    for rec, rec0 in zip(d.debug_data_list, base.debug_data_list):
        assert set(rec) == set(rec0) and rec['time'] == rec0['time'] and 0.0 <= rec['informative_score'] <= 1.0 and 0.0 <= rec['relevance_score'] <= 1.0
    assert all(set(r) == {'time', 'content', 'role'} for r in resp)
    assert m.kv_position(d.past_key_values) == len(d.past_key_values) + d.dropped_tokens
    d.reset()
    assert d.dropped_tokens == 0 and d._sink_tokens is None and d.past_key_values is None


def test_multistream_slots_hold_the_window(f32_model):
    """two slots of MultiStreamInfer, each driver built from args that carry the window: kv_drop reaches the real model through the slot's proxy, every stream ends
    inside its window and equals the same stream run alone with the same window"""
    from mmduet_amd.multistream import MultiStreamInfer
    m = f32_model[0]
    fpf = 2
    base, lens0, _ = run_driver(m, fpf)
    window = base._sink_tokens + (fpf + 3) * m.config.frame_num_tokens + 40
    alone, lens, _ = run_driver(m, fpf, context_window=window)
    assert alone.dropped_tokens > 0 and max(lens) <= window < max(lens0)
    meta = stream_cases()
    case = meta['cases']['prob_keep']
    opts = case['opts']
    args = make_args(frame_fps=case['fps'], system_prompt=meta['system_prompt'], max_new_tokens=12, stream_end_prob_threshold=opts['stream_end_prob_threshold'],
                     score_heads=opts['score_heads'], frames_per_forward=fpf, context_window=window)
    tok = tokenizer_for(m.config)
    m.config.eos_token_id = meta['eos_token_id']
    frames = torch.cat([stream_frames('prob_keep')] * 4)[:40]
    ms = MultiStreamInfer(args, model=m, tokenizer=tok, n_slots=2)
    results = ms.run([dict(frames=frames, conversation=case['conversation'], args=args) for _ in range(3)])
    for res in results:
        assert 0 < res['final_kv_len'] <= window
        assert res['final_kv_len'] == len(alone.past_key_values)
        assert res['response_token_ids'] == alone.response_token_ids
        assert len(res['debug_data']) == 40
        for got, exp in zip(res['debug_data'], alone.debug_data_list):
            assert got['informative_score'] == pytest.approx(exp['informative_score'], abs=2e-4) and got['relevance_score'] == pytest.approx(exp['relevance_score'], abs=2e-4)


def test_demo_driver_holds_the_window(f32_model):
    """LiveInferForDemo: one frame per call and a query from the side, with a window"""
    from mmduet_amd.liveinfer import LiveInferForDemo
    m = f32_model[0]
    meta = stream_cases()
    case = meta['cases']['prob_keep']
    opts = case['opts']
    nt = m.config.frame_num_tokens
    tok = tokenizer_for(m.config)
    m.config.eos_token_id = meta['eos_token_id']
    probe = LiveInferForDemo(make_args(frame_fps=case['fps'], system_prompt=meta['system_prompt'], max_new_tokens=12, stream_end_prob_threshold=opts['stream_end_prob_threshold'],
                                       score_heads=opts['score_heads']), model=m, tokenizer=tok)
    query = case['conversation'][0]['content']
    q_rows = 64          # (room for the query turn)
    window = int(probe._start_ids.shape[1]) + 5 * nt + q_rows + 40
    d = LiveInferForDemo(make_args(frame_fps=case['fps'], system_prompt=meta['system_prompt'], max_new_tokens=12, stream_end_prob_threshold=opts['stream_end_prob_threshold'],
                                   score_heads=opts['score_heads'], context_window=window), model=m, tokenizer=tok)
    d.input_video_stream(torch.cat([stream_frames('prob_keep')] * 4)[:40])
    seen = []
    for i in range(40):
        if i == 7:
            d.encode_given_query(query)
            seen.append(len(d.past_key_values))
        ret = d.input_one_frame()
        assert set(ret) >= {'frame_idx', 'time', 'informative_score', 'relevance_score', 'response'}
        seen.append(len(d.past_key_values))
    assert d.dropped_tokens > 0 and max(seen) <= window, (max(seen), window)
    assert m.kv_position(d.past_key_values) == len(d.past_key_values) + d.dropped_tokens
