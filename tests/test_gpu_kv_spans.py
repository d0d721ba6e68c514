"""Many spans in one pass on the device: mmd_kv_drop_spans leaves the arena of the host statement (tests/kv_spans_cases.py) bit for bit -- which is also the arena of the
same spans dropped one at a time, last span first --, keeps the position; the shifted form moves V the same way, leaves the keys in front of the first span alone and turns
every retained key back by the tokens dropped in front of it (tests/kv_shift_oracle.py, under its derived bound), gives mmd_kv_drop_shift's bits for one span and shrinks
the position by the total; refusals change nothing; steps and decode rows afterwards equal the oracle over the sliced handle; the driver evicts uninformative frames.
Models and tolerances are those of tests/test_gpu_kv_drop.py and tests/test_gpu_kv_shift.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import kv_layout as L
import kv_drop_cases as D
import kv_shift_oracle as SO
import kv_spans_cases as S
from oracle import duet_oracle as O
from mmduet_amd._lib import lib, check, MmduetError
from mmduet_amd.modeling_live import _ptr
from helpers import hip_model, oracle_model, make_args, tokenizer_for, stream_cases, stream_frames

BF = torch.bfloat16
F32_TOL = 3e-4          # tests/test_gpu_kv_drop.py: fp32 HIP path vs the fp32 oracle
BF16_LOGITS = 2 * 6e-2  # tests/test_gpu_kv_drop.py: the bf16 logits bound under which the oracle's own top-2 gap decides nothing
CASE_IDS = [f'{len(sp)}spans-of-{n}-{i}' for i, (sp, n) in enumerate(S.CASES)]


@pytest.fixture(scope='module')
def bf16_model():
    """the 2-layer true-width bf16 model of tests/test_gpu_kv_drop.py (nkv 4, d 128), captured decode step on"""
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


@pytest.fixture(params=['bf16', 'fp32'])
def model(request):
    return request.param, request.getfixturevalue('bf16_model' if request.param == 'bf16' else 'f32_model')[0]


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


def logical(m, cache, n):
    """the first n live tokens as (K, V) [layers, nkv, n, d], V un-transposed on the host's terms (kv_layout.v_logical)"""
    if n == 0:
        c = m.config
        e = torch.empty(c.num_hidden_layers, c.num_key_value_heads, 0, c.head_dim, dtype=m.dtype, device=m.device)
        return e, e
    K, V = snapshot(m, cache, up64(n))
    return K[:, :, :n], torch.stack([L.v_logical(V[i])[:, :n] for i in range(V.shape[0])])


def ibits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(ibits(a), ibits(b))


def to_np(t):
    return t.detach().cpu().float().numpy().astype(np.float64)


def inv_freq(m):
    return m._rope_inv_freq.detach().cpu().float().numpy()


def context(m, n, seed):
    H = m.config.hidden_size
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = (torch.randn(1, n, H, generator=g, device='cuda') * 0.5).to(m.dtype)
    return m(inputs_embeds=x).past_key_values          # filled by real steps


def spans_on_the_library(m, cache, spans, shift):
    """mmd_kv_drop_spans itself (the Python layer answers an empty list without a call)"""
    import ctypes as C
    flat = (C.c_int64 * max(1, 2 * len(spans)))(*[x for sp in spans for x in sp])
    m._bind_stream()
    return lib().mmd_kv_drop_spans(cache.arena.h, C.cast(flat, C.c_void_p), len(spans), shift)


def launch_deltas(spans, n):
    """for every kept token, in order: the positions each launch that moves it turns it back by (one entry per launch: beyond 64 spans a key behind a group's first span
    is moved, and rounded, once per group at or below its own)"""
    slots = list(range(n))          # the old slot of the token in each slot
    turns = {t: [] for t in range(n)}
    for dst0, len_in, len_end, segs in S.launches(spans, n):
        slots = slots[:len_in]          # (a dropped tail moved nothing)
        new, dst = slots[:dst0], dst0
        for src, count in segs:
            for t in slots[src:src + count]:
                turns[t].append(src - dst)
            new += slots[src:src + count]; dst += count
        slots = new
    keep = S.kept(spans, n)
    assert slots[:len(keep)] == keep
    return [turns[t] for t in keep]


def check_shifted_keys(m, kind, K0, got, spans, n, what):
    """got [layers, nkv, newlen, d] against the oracle: token by token turned back launch by launch (float64, the fp32 angle of each launch), under the oracle's bound.
    One launch: kv_shift_oracle.bound as it stands.  A key moved by g launches was rounded g times: the error of the launches before passes through a rotation, which keeps
    the pair's error norm (so each component's is at most hypot of the pair's two), and the last launch adds its own bound."""
    keep, turns = S.kept(spans, n), launch_deltas(spans, n)
    first = S.normalise(spans)[0][0] if S.normalise(spans) else n
    assert same(got[:, :, :first], K0[:, :, :first]), f'{what}: K below the first span was written'
    inv, K0n, gotn = inv_freq(m), to_np(K0), to_np(got)
    worst = 0.0
    groups = {}
    for j, t in enumerate(keep):
        if turns[j]:
            groups.setdefault(tuple(turns[j]), []).append((j, t))
    for deltas, members in groups.items():
        js, ts = [j for j, _ in members], [t for _, t in members]
        exact, pn = K0n[:, :, ts], SO.pair_norm(K0n[:, :, ts])
        bnd = np.zeros_like(exact)
        for dl in deltas:
            exact = SO.turn_back(exact, dl, inv)
            half = bnd.shape[-1] // 2
            carried = np.hypot(bnd[..., :half], bnd[..., half:])
            bnd = np.concatenate([carried, carried], -1) + SO.bound(exact, pn, kind) * (1 + 2.0 ** -7 if len(deltas) > 1 else 1)          # (the bound is taken at the exact keys, the device's are within 2^-8 of them)
        err = np.abs(gotn[:, :, js] - exact)
        worst = max(worst, float((err / np.maximum(bnd, 1e-300)).max()))
        assert (err <= bnd).all(), f'{what}: deltas {deltas}: {int((err > bnd).sum())} of {err.size} keys outside the bound, worst at {float((err / np.maximum(bnd, 1e-300)).max()):.3g} of it'
    print(f'{what}: worst |got - exact| / bound = {worst:.3g}')


# ---- the arena -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', S.CASES, ids=CASE_IDS)
def test_arena_after_the_spans(model, case):
    kind, m = model
    spans, n = case
    ns = S.normalise(spans)
    total = sum(b - a for a, b in ns)
    newlen, what = n - total, f'{kind} {len(spans)} spans of {n}'
    cache = context(m, n, 7 * n + len(spans))
    assert len(cache) == n
    K0, V0 = logical(m, cache, n)
    want_k, want_v = S.drop_rows(K0, spans), S.drop_rows(V0, spans)
    one_by_one, shifted = m.kv_fork(cache), m.kv_fork(cache)
    # plain: the host statement, bit for bit
    if not spans:
        assert spans_on_the_library(m, cache, spans, 0) == S.MMD_OK
    cache = m.kv_drop_many(cache, spans)
    assert len(cache) == newlen == int(lib().mmd_kv_len(cache.arena.h)), what
    assert m.kv_position(cache) == n == int(lib().mmd_kv_position(cache.arena.h)), what
    gk, gv = logical(m, cache, newlen)
    assert same(gk, want_k), f'{what}: K differs in {int((ibits(gk) != ibits(want_k)).sum())} elements'
    assert same(gv, want_v), f'{what}: V differs in {int((ibits(gv) != ibits(want_v)).sum())} elements'
    # ... and the arena of the spans dropped one at a time, last span first
    for a, b in reversed(spans):
        one_by_one = m.kv_drop(one_by_one, a, b)
    assert len(one_by_one) == newlen and m.kv_position(one_by_one) == n
    ok, ov = logical(m, one_by_one, newlen)
    assert same(gk, ok) and same(gv, ov), what
    if newlen:
        Ks, Vs = snapshot(m, cache, up64(newlen))          # every slot up to the end of the last V block is finite
        assert bool(torch.isfinite(Ks.float()).all()) and bool(torch.isfinite(Vs.float()).all()), what
    # shifted: V as the plain form's, K turned back, the position shrinks by the total
    shifted = m.kv_drop_many(shifted, spans, shift=True)
    assert len(shifted) == newlen == int(lib().mmd_kv_len(shifted.arena.h)), what
    assert m.kv_position(shifted) == newlen == int(lib().mmd_kv_position(shifted.arena.h)), what
    sk, sv = logical(m, shifted, newlen)
    assert same(sv, gv), f'{what}: V of the plain and the shifted form differ'
    check_shifted_keys(m, kind, K0, sk, spans, n, what)
    if newlen:
        Ks, Vs = snapshot(m, shifted, up64(newlen))
        assert bool(torch.isfinite(Ks.float()).all()) and bool(torch.isfinite(Vs.float()).all()), what
    if n >= 4000:
        m.release_pooled_arenas()


@pytest.mark.parametrize('span', D.REQUIRED + [(3, 4, 1500), (100, 149, 700)], ids=lambda c: '-'.join(map(str, c)))
def test_one_span_has_the_bits_of_kv_drop_shift(model, span):
    kind, m = model
    frm, to, n = span
    cache = context(m, n, 11 * n + frm)
    twin = m.kv_fork(cache)
    a = m.kv_drop(cache, frm, to, shift=True)
    b = m.kv_drop_many(twin, [(frm, to)], shift=True)
    assert len(a) == len(b) == n - (to - frm) and m.kv_position(a) == m.kv_position(b)
    (ak, av), (bk, bv) = logical(m, a, len(a)), logical(m, b, len(b))
    assert same(ak, bk) and same(av, bv), (kind, span)


def test_a_position_offset_stays(f32_model):
    """after an earlier plain drop: the plain form adds to the offset, the shifted form leaves it"""
    m = f32_model[0]
    cache = m.kv_drop(context(m, 150, 5), 3, 8)
    twin = m.kv_fork(cache)
    assert m.kv_position(cache) == 150 and len(cache) == 145
    cache = m.kv_drop_many(cache, [(10, 20), (30, 31), (100, 120)])
    assert len(cache) == 114 and m.kv_position(cache) == 150
    twin = m.kv_drop_many(twin, [(10, 20), (30, 31), (100, 120)], shift=True)
    assert len(twin) == 114 and m.kv_position(twin) == 119


def test_refusals_change_nothing(f32_model):
    m = f32_model[0]
    H = m.config.hidden_size
    g = torch.Generator().manual_seed(1)
    cache = m(inputs_embeds=rand(g, S.REFUSAL_LEN, H, m.dtype).cuda()).past_key_values
    cache = m.kv_drop(cache, 3, 5)          # a position offset to keep
    cache = m(inputs_embeds=rand(g, 2, H, m.dtype).cuda(), past_key_values=cache).past_key_values
    h = cache.arena.h
    before = snapshot(m, cache, 128)

    def unchanged():
        after = snapshot(m, cache, 128)
        return int(lib().mmd_kv_len(h)) == S.REFUSAL_LEN and int(lib().mmd_kv_position(h)) == S.REFUSAL_LEN + 2 and same(before[0], after[0]) and same(before[1], after[1])
    assert unchanged()
    for shift in (0, 1):
        for spans, code in S.REFUSED:
            assert spans_on_the_library(m, cache, spans, shift) == code, (spans, shift)
            assert unchanged(), (spans, shift)
        assert lib().mmd_kv_drop_spans(None, None, 0, shift) == S.MMD_EINVAL          # the null stream
        assert lib().mmd_kv_drop_spans(h, None, 2, shift) == S.MMD_EINVAL and lib().mmd_kv_drop_spans(h, None, -1, shift) == S.MMD_EINVAL
        assert lib().mmd_kv_drop_spans(h, None, 0, shift) == S.MMD_OK and unchanged()
    with pytest.raises(ValueError):
        m.kv_drop_many(cache, [(5, 6), (90, S.REFUSAL_LEN + 1)])
    with pytest.raises(MmduetError, match='ascend'):
        m.kv_drop_many(cache, [(30, 40), (10, 20)])
    assert unchanged()
    # while a stash is held: refused, whatever the spans; after the unstash: accepted
    stash = m.kv_stash(cache, 60)
    for shift in (0, 1):
        assert spans_on_the_library(m, cache, [(10, 20), (30, 40)], shift) == S.MMD_EINVAL and spans_on_the_library(m, cache, [(4, 4)], shift) == S.MMD_EINVAL
    with pytest.raises(MmduetError, match='stash'):
        m.kv_drop_many(cache, [(10, 20), (30, 40)])
    cache = m.kv_unstash(stash)
    assert unchanged()
    assert spans_on_the_library(m, cache, [(4, 4), (9, 9)], 0) == S.MMD_OK and unchanged()          # only empty spans: nothing
    assert spans_on_the_library(m, cache, [(10, 20), (30, 40)], 0) == S.MMD_OK
    assert int(lib().mmd_kv_len(h)) == S.REFUSAL_LEN - 20 and int(lib().mmd_kv_position(h)) == S.REFUSAL_LEN + 2


# ---- steps afterwards ------------------------------------------------------------------------------------------------------------------------------------------
N0, THREE = 150, [(10, 40), (41, 60), (100, 121)]          # a one-token segment between the first two
GONE = sum(b - a for a, b in THREE)


def maxerr(a, b):
    return (a.float().cpu() - b.float().cpu()).abs().max().item()


def oracle_greedy_with_gaps(w, cfg, x, past, pos0, n_new):
    """kv_drop_cases.oracle_greedy_at, the gap in front of every token kept"""
    ids, gaps = [], []
    for _ in range(n_new):
        h, past = D.oracle_step_at(w, cfg, x, past, pos0)
        pos0 += x.shape[0]
        top = O.linear(h[-1:], w['lm_head.weight']).float()[0].topk(2)
        gaps.append(float(top.values[0] - top.values[1])); ids.append(int(top.indices[0]))
        x = w['model.embed_tokens.weight'][ids[-1]][None]
    return ids, gaps


def test_fp32_steps_after_three_spans_equal_the_oracle(f32_model):
    m, w, cfg = f32_model
    H = cfg.hidden_size
    g = torch.Generator().manual_seed(21)
    x0, x, prompt = rand(g, N0, H, torch.float32), rand(g, 7, H, torch.float32), rand(g, 3, H, torch.float32)
    _, kv = O.llm_forward(w, cfg, x0[0], None)
    kvd = S.drop_handle(kv, THREE)
    # a chunk step at the stream's position
    want, kv1 = D.oracle_step_at(w, cfg, x[0], kvd, N0)
    cache = m.kv_drop_many(m(inputs_embeds=x0.cuda()).past_key_values, THREE)
    assert len(cache) == N0 - GONE and m.kv_position(cache) == N0
    out = m(inputs_embeds=x.cuda(), past_key_values=cache)
    err = maxerr(out.hidden_states[0], want)
    print(f'chunk step after three spans: max |hidden - oracle| = {err:.4g}')
    assert err < F32_TOL
    assert m.kv_position(out.past_key_values) == N0 + 7 and len(out.past_key_values) == N0 - GONE + 7
    # 8 greedy decode steps
    ids_w, gaps = oracle_greedy_with_gaps(w, cfg, prompt[0], kv1, N0 + 7, 8)
    assert min(gaps) > 10 * F32_TOL, gaps          # no near-tie in the oracle's own logits
    ids, after = m.greedy_generate(prompt.cuda(), out.past_key_values, -1, 8)
    assert ids == ids_w and m.kv_position(after) == N0 + 7 + 3 + 7


@pytest.mark.parametrize('captured', [True, False], ids=['captured', 'call-by-call'])
def test_bf16_decode_after_three_spans_equals_the_oracle(bf16_model, captured):
    """ids equal the bf16 oracle's over the sliced handle up to the first token in front of which the oracle's own top-2 gap is below the bf16 logits bound"""
    from mmduet_amd.modeling_live import fast_greedy_generate
    m, w, ocfg = bf16_model
    H = m.config.hidden_size
    g = torch.Generator().manual_seed(1057)
    ctx, x, prompt = rand(g, N0, H, BF), rand(g, 49, H, BF), rand(g, 5, H, BF)
    _, kv = O.llm_forward(w, ocfg, ctx[0], None)
    want_h, kv1 = D.oracle_step_at(w, ocfg, x[0], S.drop_handle(kv, THREE), N0)
    ids_w, gaps = oracle_greedy_with_gaps(w, ocfg, prompt[0], kv1, N0 + 49, 8)
    cache = m.kv_drop_many(m(inputs_embeds=ctx.cuda()).past_key_values, THREE)
    out = m(inputs_embeds=x.cuda(), past_key_values=cache)
    lg_w = O.linear(want_h[-1:], w['lm_head.weight']).float()[0]
    err = maxerr(out.logits[0, -1], lg_w)
    print(f'chunk step after three spans: max |logits - oracle| = {err:.4g}')
    assert err < BF16_LOGITS
    if captured:
        ids, after = m.greedy_generate(prompt.cuda(), out.past_key_values, -1, 8)
        assert m.decode_last_route() in (1, 2)
    else:
        buf = torch.zeros(1, 8, dtype=torch.long, device='cuda')
        m.python_generate_loop = True
        try:
            ids, after, _ = fast_greedy_generate(model=m, inputs_embeds=prompt.cuda(), past_key_values=out.past_key_values, eos_token_id=-1, inplace_output_ids=buf)
        finally:
            m.python_generate_loop = False
        ids = ids[0].tolist()
    sure = next((i for i, gp in enumerate(gaps) if gp < BF16_LOGITS), len(gaps))
    print(f'oracle ids {ids_w}, gaps {[round(x, 3) for x in gaps]}; device {ids}; compared: the first {sure}')
    assert len(ids) == 8 and ids[:sure] == ids_w[:sure]
    assert m.kv_position(after) == N0 + 49 + 5 + 7 and len(after) == N0 - GONE + 49 + 5 + 7


def shifted_context(m, K0, V0, spans):
    """the oracle's canonical K / V [layers, nkv, n, d] after a shifted drop of the spans: every retained segment turned back by its own delta (float64, rounded once)"""
    n = K0.shape[2]
    first = S.normalise(spans)[0][0]
    ks, vs = [K0[:, :, :first]], [V0[:, :, :first]]
    for src, count, _, delta in S.segments(spans, n):
        ks.append(torch.from_numpy(SO.turn_back(to_np(K0[:, :, src:src + count]), delta, inv_freq(m)).astype(np.float32)).to(K0.dtype))
        vs.append(V0[:, :, src:src + count])
    return torch.cat(ks, 2), torch.cat(vs, 2)


def test_steps_behind_shifted_spans_equal_the_oracle_context(model):
    """tests/test_gpu_kv_shift.py's sink test for three spans.  Stream X: a device kv_drop_many(THREE, shift=True).  Stream Y: a fresh stream that receives the oracle's
    K / V, computed on the CPU from X's export before the drop, and the new length as its position.  A chunk step and six decode rows agree in hidden states and logits
    (that file's tolerances); then the native decode loop behind the shifted drop -- the captured step in bf16 -- returns ids that the call-by-call logits of the same
    context place within the logits tolerance of the best, and the bookkeeping follows."""
    from mmduet_amd.modeling_live import KVSnapshot
    kind, m = model
    H = m.config.hidden_size
    c = m.config
    layers, nkv, d = c.num_hidden_layers, c.num_key_value_heads, c.head_dim
    g = torch.Generator().manual_seed(41)
    x0 = rand(g, N0, H, m.dtype).cuda()
    cx = m(inputs_embeds=x0).past_key_values
    snap = m.kv_save(cx, pin=False)
    K0, V0 = snap.K, snap.V
    cx = m.kv_drop_many(cx, THREE, shift=True)
    Kn, Vn = shifted_context(m, K0, V0, THREE)
    cy = m.kv_load(KVSnapshot(Kn, Vn, N0 - GONE, m.dtype, layers, nkv, d, m._rope_inv_freq))
    assert m.kv_position(cx) == m.kv_position(cy) == N0 - GONE == len(cx) == len(cy)
    tol_h, tol_l = (F32_TOL, F32_TOL) if kind == 'fp32' else (6e-2, BF16_LOGITS)          # tests/test_gpu_kv_shift.py: bf16 lm_head logits under 2 TOL, the rest under TOL
    x = rand(g, 49 if kind == 'bf16' else 9, H, m.dtype).cuda()
    for step in range(7):
        oa, ob = m(inputs_embeds=x, past_key_values=cx), m(inputs_embeds=x, past_key_values=cy)
        cx, cy = oa.past_key_values, ob.past_key_values
        eh, el = maxerr(oa.hidden_states[0], ob.hidden_states[0]), maxerr(oa.logits[0, -1], ob.logits[0, -1])
        print(f'{kind} step {step} ({x.shape[1]} rows): hidden {eh:.4g}, logits {el:.4g}')
        assert eh < tol_h and el < tol_l, (kind, step, eh, el)
        assert bool(torch.isfinite(oa.logits[0, -1]).all())
        x = m.get_input_embeddings()(torch.tensor([[int(oa.logits[0, -1].argmax())]], device=m.device)).view(1, 1, H)
    n1 = len(cx)
    assert m.kv_position(cx) == n1 == len(cy)
    # the native loop (bf16: the captured decode step) behind the shifted drop, held against call-by-call logits of a fork of the same context
    prompt = rand(g, 5, H, m.dtype).cuda()
    twin = m.kv_fork(cx)
    ids, after = m.greedy_generate(prompt, cx, -1, 6)
    if kind == 'bf16':
        assert m.decode_last_route() in (1, 2)
    assert len(ids) == 6 and len(after) == n1 + 5 + 5 == m.kv_position(after)
    xin, worst = prompt, 0.0
    for t in ids:
        out = m(inputs_embeds=xin, past_key_values=twin)
        twin, lg = out.past_key_values, out.logits[0, -1].float()
        worst = max(worst, float(lg.max() - lg[t]))
        xin = m.get_input_embeddings()(torch.tensor([[t]], device=m.device)).view(1, 1, H)
    print(f'{kind}: native loop ids {ids}, worst shortfall against call-by-call logits {worst:.4g}')
    assert worst < tol_l


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------------------------
class _Watch:
    """the model with the context length behind every forward the driver issues, and every eviction it asks for"""

    def __init__(self, m):
        self.__dict__.update(_m=m, lens=[], many=[], drops=[], calls=[])          # calls: every drop in order, ([spans], shift)

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

    def kv_drop(self, handle, start, end, **k):
        self.drops.append((int(start), int(end))); self.calls.append(([(int(start), int(end))], bool(k.get('shift', False))))
        return self._m.kv_drop(handle, start, end, **k)

    def kv_drop_many(self, handle, spans, **k):
        self.many.append(([(int(a), int(b)) for a, b in spans], bool(k.get('shift', False)))); self.calls.append(self.many[-1])
        return self._m.kv_drop_many(handle, spans, **k)


def run_driver(m, fpf, **window):
    from mmduet_amd.inference import LiveInferForBenchmark
    meta = stream_cases()
    case = meta['cases']['prob_keep']
    opts = case['opts']
    args = make_args(frame_fps=case['fps'], system_prompt=meta['system_prompt'], max_new_tokens=12, stream_end_prob_threshold=opts['stream_end_prob_threshold'],
                     score_heads=opts['score_heads'], frames_per_forward=fpf, **window)
    tok = tokenizer_for(m.config)
    m.config.eos_token_id = meta['eos_token_id']
    wm = _Watch(m)
    d = LiveInferForBenchmark(args, model=wm, tokenizer=tok)
    d.input_video_stream(torch.cat([stream_frames('prob_keep')] * 4)[:40])
    d.input_query_stream(case['conversation'])
    d.inference()
    return d, wm


class _PosHandle(O.KVHandle):
    """the oracle's functional handle with the RoPE position of the next token beside it"""
    __slots__ = ('pos',)

    def __init__(self, k, v, pos):
        super().__init__(k, v)
        self.pos = pos


class _OracleAt:
    """The oracle model under the same driver: every step rotates its new rows at the position the handle carries (kv_drop_cases.oracle_step_at), a drop slices the
    handle (kv_spans_cases.drop_handle) and keeps the position, a shifted drop also turns the retained keys back (kv_shift_oracle.turn_back per segment, rounded once to
    the handle's dtype) and takes the total off the position.  Every drop the oracle driver asks for must be the one the device driver asked for at the same point
    (`script`, in order): the two drivers slice the same spans."""

    def __init__(self, om, inv, script):
        self.__dict__.update(_m=om, inv=inv, script=list(script), at=0)

    def __getattr__(self, name):
        return getattr(self._m, name)

    def __call__(self, inputs_embeds=None, past_key_values=None, **kw):
        w, cfg, past = self._m.w, self._m.cfg, past_key_values
        h, kv = D.oracle_step_at(w, cfg, inputs_embeds[0].to(self._m.dtype), past, past.pos if past else 0)
        cache = _PosHandle(kv.k, kv.v, (past.pos if past else 0) + inputs_embeds.shape[1])
        return O.OracleOutput(logits=O.linear(h, w['lm_head.weight']).float()[None], informative_logits=O.linear(h, w['informative_head.weight']).float()[None],
                              relevance_logits=O.linear(h, w['relevance_head.weight']).float()[None], past_key_values=cache, hidden_states=h[None])

    def cache_prefix(self, handle, length):
        return _PosHandle([k[:, :length] for k in handle.k], [v[:, :length] for v in handle.v], handle.pos - (len(handle) - length))

    def _drop(self, handle, spans, shift):
        want = self.script[self.at] if self.at < len(self.script) else None
        assert want == (spans, shift), f'drop {self.at}: the oracle driver asks for {(spans, shift)}, the device driver asked for {want}'
        self.__dict__['at'] = self.at + 1
        cut = S.drop_handle(handle, spans)
        total = sum(b - a for a, b in spans)
        if not shift:
            return _PosHandle(cut.k, cut.v, handle.pos)
        ks = []
        for k in handle.k:
            parts = [k[:, :spans[0][0]]]
            for src, count, _, delta in S.segments(spans, k.shape[1]):
                parts.append(torch.from_numpy(SO.turn_back(to_np(k[:, src:src + count]), delta, self.inv).astype(np.float32)).to(k.dtype))
            ks.append(torch.cat(parts, 1))
        return _PosHandle(ks, cut.v, handle.pos - total)

    def kv_drop(self, handle, start, end, shift=False):
        return self._drop(handle, [(int(start), int(end))], bool(shift))

    def kv_drop_many(self, handle, spans, shift=False):
        return self._drop(handle, [(int(a), int(b)) for a, b in spans], bool(shift))


STREAM_TOL = 2e-4          # tests/test_gpu_streams.py: the fp32 device stream against the reference's scores


@pytest.mark.parametrize('positions', ['kept', 'shifted'])
def test_driver_evicts_uninformative_frames(f32_model, positions):
    """a 40-frame stream under a window that forces evictions, on the device and -- the same driver, the same arguments -- over the oracle model stepping at the
    device's positions and slicing the same spans (_OracleAt): every score of every frame agrees under the stream tolerance of tests/test_gpu_streams.py, the responses
    are the same tokens, the context ends at the same length and position.  On the device: the driver asks for the evictions through kv_drop_many, every forward stays
    inside the window, the ledger at the end denotes whole frames of the context, and the position is the length plus what plain evictions took out (shifted: the length)."""
    from mmduet_amd.inference import LiveInferForBenchmark
    m = f32_model[0]
    fpf, nt = 2, m.config.frame_num_tokens
    base, w0 = run_driver(m, fpf)
    window = base._sink_tokens + (fpf + 5) * nt + 40
    assert window < max(w0.lens) and base.evicted_frames == 0 and w0.many == []
    kw = dict(context_window=window, context_evict='informative', context_recent=2 * nt, context_positions=positions)
    d, wm = run_driver(m, fpf, **kw)
    shift = positions == 'shifted'
    print(f'{positions}: window {window}, {len(wm.many)} evictions of {[len(sp) for sp, _ in wm.many]} spans, {d.evicted_frames} frames, {len(wm.drops)} oldest-first drops')
    assert len(wm.many) >= 3 and d.evicted_frames >= 3 and all(s == shift for _, s in wm.many)
    assert max(wm.lens) <= window, (max(wm.lens), window)
    assert any(sp[0][0] > d._sink_tokens for sp, _ in wm.many)          # frames left the middle of the context
    assert d.dropped_tokens == sum(b - a for sp, _ in wm.many for a, b in sp) + sum(b - a for a, b in wm.drops)
    assert m.kv_position(d.past_key_values) == len(d.past_key_values) + (0 if shift else d.dropped_tokens)
    assert all(e[1] - e[0] == nt and e[1] <= len(d.past_key_values) for e in d._frame_ledger)
    assert len(d.debug_data_list) == 40
    # the oracle driver
    meta = stream_cases()
    case = meta['cases']['prob_keep']
    opts = case['opts']
    om = oracle_model('A')[0]
    otok = tokenizer_for(om.config)                       # (the tokenizer builder writes its own eos into the config ...)
    om.config.eos_token_id = meta['eos_token_id']         # ... the fixture's synthetic "eos" goes in afterwards
    args = make_args(frame_fps=case['fps'], system_prompt=meta['system_prompt'], max_new_tokens=12, stream_end_prob_threshold=opts['stream_end_prob_threshold'],
                     score_heads=opts['score_heads'], frames_per_forward=fpf, **kw)
    oa = _OracleAt(om, inv_freq(m), wm.calls)
    od = LiveInferForBenchmark(args, model=oa, tokenizer=otok)
    od.input_video_stream(torch.cat([stream_frames('prob_keep')] * 4)[:40])
    od.input_query_stream(case['conversation'])
    od.inference()
    assert oa.at == len(wm.calls) >= 3          # every drop of the device driver was replayed
    worst = 0.0
    for got, exp in zip(d.debug_data_list, od.debug_data_list):
        assert got['time'] == pytest.approx(exp['time'])
        worst = max(worst, abs(got['informative_score'] - exp['informative_score']), abs(got['relevance_score'] - exp['relevance_score']))
        assert got['informative_score'] == pytest.approx(exp['informative_score'], abs=STREAM_TOL)
        assert got['relevance_score'] == pytest.approx(exp['relevance_score'], abs=STREAM_TOL)
    print(f'{positions}: worst |score - oracle driver| over 40 frames = {worst:.3g}')
    assert len(od.debug_data_list) == 40 and d.response_token_ids == od.response_token_ids
    assert len(d.past_key_values) == len(od.past_key_values) and m.kv_position(d.past_key_values) == od.past_key_values.pos
    assert (d.dropped_tokens, d.evicted_frames, d._frame_ledger) == (od.dropped_tokens, od.evicted_frames, [[a, b, pytest.approx(sc, abs=STREAM_TOL)] for a, b, sc in od._frame_ledger])
