"""What the model's steps leave in a stream's KV arena, read back as stored (mmd_kv_debug_read) and compared bit for bit.

Twin streams: stream A first holds a 400-token random context and is rolled back, so every slot above its length is stale but plausible; stream B receives the same
live tokens by the same calls.  Both take the same step.  Then, exactly:
  * footprint: A's arena outside [L, L + S) is unchanged by the step (raw contents, so the neighbours inside partly written V blocks are covered);
  * A and B agree on [0, L + S): same kernels on the same inputs, so a slot nobody wrote shows up as stale against fresh;
  * every new K row and V column of A differs from what the slot held before.
One anchor to the truth per schedule: layer-0 K and V of the new slots against a float64 reference from the model's own weights, at assert_close's bf16 bound.
Further: stash / unstash and arena growth (both mechanisms) keep every live slot's bits."""
import ctypes as C
import pytest
import torch

pytestmark = pytest.mark.gpu
import kv_layout as L
from oracle import duet_oracle as O
from mmduet_amd._lib import lib, check
from mmduet_amd.modeling_live import _ptr
from test_gpu_ops import assert_close

BF = torch.bfloat16
STALE = 400


@pytest.fixture(scope='module')
def model():
    """the 2-layer true-width bf16 model (tests/test_gpu_trueshape.py), with the captured decode step switched on for mmd_greedy_generate"""
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


def rand(g, rows, H, dtype=BF):
    return (torch.randn(1, rows, H, generator=g) * 0.5).to(dtype).cuda()


def snapshot(m, cache, n=None):
    """-> (K [layers, nkv, n, d], V in token order [layers, nkv, n, d]) of the first n tokens of the handle's arena, as stored (V through the layout's permute only)"""
    h = cache.arena.h
    if n is None:
        n = min(1024, int(lib().mmd_kv_capacity(h)))
    c = m.config
    layers, nkv, d = c.num_hidden_layers, c.num_key_value_heads, c.head_dim
    K = torch.empty(layers, nkv, n, d, dtype=m.dtype, device=m.device)
    V = torch.empty(layers, nkv, n // L.BLK, d, L.BLK, dtype=m.dtype, device=m.device)
    m._bind_stream()
    for i in range(layers):
        check(lib().mmd_kv_debug_read(h, i, n, _ptr(K[i]), _ptr(V[i])), m._ctx, 'mmd_kv_debug_read')
    return K, torch.stack([L.v_logical(V[i]) for i in range(layers)])


def ibits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same(a, b):
    return torch.equal(ibits(a), ibits(b))


def assert_step_footprint(before, after, lo, hi, what):
    """the arena changed at tokens [lo, hi) only, and every row there is new"""
    for name, b, a in (('K', before[0], after[0]), ('V', before[1], after[1])):
        assert same(b[:, :, :lo], a[:, :, :lo]), f'{what}: {name} below token {lo} changed'
        assert same(b[:, :, hi:], a[:, :, hi:]), f'{what}: {name} at or above token {hi} changed'
        fresh = (ibits(b[:, :, lo:hi]) != ibits(a[:, :, lo:hi])).any(-1)
        assert bool(fresh.all()), f'{what}: {int((~fresh).sum())} {name} rows inside [{lo}, {hi}) still hold their stale contents'


def assert_twins_agree(a, b, upto, what):
    for name, x, y in (('K', a[0], b[0]), ('V', a[1], b[1])):
        assert same(x[:, :, :upto], y[:, :, :upto]), f'{what}: {name} of the stale and the fresh stream differ below token {upto} in {int((ibits(x[:, :, :upto]) != ibits(y[:, :, :upto])).sum())} elements'


def twins(m, g, length, H):
    """-> (handle of A, handle of B), both holding the same `length` tokens; A's slots above are stale"""
    stale = rand(g, STALE, H, m.dtype); live = rand(g, length, H, m.dtype)
    a0 = m(inputs_embeds=stale).past_key_values
    a = m(inputs_embeds=live, past_key_values=m.cache_prefix(a0, 0)).past_key_values if length else m.cache_prefix(a0, 0)
    b = m(inputs_embeds=live).past_key_values if length else m.new_cache()
    assert a.arena is not b.arena
    return a, b


def anchor_layer0(m, w, x, pos0, snap, what):
    """layer-0 K / V of tokens [pos0, pos0 + S) against float64 math on the model's weights: rms_norm -> k / v projection + bias -> rotate-half RoPE of k"""
    c = m.config
    nkv, d, eps = c.num_key_value_heads, c.head_dim, c.rms_norm_eps
    xs = x.reshape(-1, c.hidden_size).double().cpu()
    S = xs.shape[0]
    p = 'model.layers.0.'
    xn = xs * torch.rsqrt(xs.pow(2).mean(-1, keepdim=True) + eps) * w[p + 'input_layernorm.weight'].double()
    k = (xn @ w[p + 'self_attn.k_proj.weight'].double().T + w[p + 'self_attn.k_proj.bias'].double()).view(S, nkv, d).transpose(0, 1)
    v = (xn @ w[p + 'self_attn.v_proj.weight'].double().T + w[p + 'self_attn.v_proj.bias'].double()).view(S, nkv, d).transpose(0, 1)
    fr = torch.arange(pos0, pos0 + S).float()[:, None] * L.inv_freq(d, c.rope_theta)[None, :]
    emb = torch.cat([fr, fr], -1).double()
    k = O.apply_rope(k, emb.cos(), emb.sin())
    assert_close(snap[0][0][:, pos0:pos0 + S], k, BF, what=what + ' layer-0 K')
    assert_close(snap[1][0][:, pos0:pos0 + S], v, BF, what=what + ' layer-0 V')


def run_twin_step(m, w, length, S, step, what, anchor_x=None):
    """step(handle) -> handle S tokens longer; run on the stale and on the fresh twin"""
    H = m.config.hidden_size
    g = torch.Generator().manual_seed(length * 1000 + S)
    a, b = twins(m, g, length, H)
    before = snapshot(m, a)
    a1 = step(a)
    plan = m.step_last_plan()
    after = snapshot(m, a)
    b1 = step(b)
    fresh = snapshot(m, b)
    assert len(a1) == len(b1) == length + S
    assert_step_footprint(before, after, length, length + S, what)
    assert_twins_agree(after, fresh, length + S, what)
    if anchor_x is not None:
        anchor_layer0(m, w, anchor_x() if callable(anchor_x) else anchor_x, length, after, what)
    return plan


def test_tile_step_with_chunk_rope(model):
    """the tile schedule starts above STEP_FUSED_MAX_ROWS = 256 rows (step_plan.h): 290 rows at 57 end at 347, ragged against the 8-token groups at both ends"""
    m, w, _ = model
    x = rand(torch.Generator().manual_seed(1), 290, m.config.hidden_size)
    plan = run_twin_step(m, w, 57, 290, lambda h: m(inputs_embeds=x, past_key_values=h).past_key_values, 'tile step S 290 at 57', x)
    assert plan['schedule'] == 0 and plan['chunk_rope'] == 1, plan


def test_130_row_step_over_two_block_edges(model):
    """S = 130 at 57: up to 256 rows a step of this model takes the fused-slab schedule (slab_rope_append_kernel), here across two block edges"""
    m, w, _ = model
    x = rand(torch.Generator().manual_seed(1), 130, m.config.hidden_size)
    plan = run_twin_step(m, w, 57, 130, lambda h: m(inputs_embeds=x, past_key_values=h).past_key_values, 'S 130 at 57', x)
    assert plan['schedule'] == 1 and plan['chunk_rope'] == 0, plan


def test_fused_slab_step(model):
    m, w, _ = model
    x = rand(torch.Generator().manual_seed(2), 49, m.config.hidden_size)
    plan = run_twin_step(m, w, 63, 49, lambda h: m(inputs_embeds=x, past_key_values=h).past_key_values, 'fused slabs S 49 at 63', x)
    assert plan['schedule'] == 1, plan


@pytest.mark.parametrize('length', [63, 64, 127])
def test_decode_chain_step(model, length):
    m, w, _ = model
    x = rand(torch.Generator().manual_seed(3 + length), 1, m.config.hidden_size)
    plan = run_twin_step(m, w, length, 1, lambda h: m(inputs_embeds=x, past_key_values=h).past_key_values, f'decode chain at {length}', x)
    assert plan['schedule'] == 2 and plan['rope_fused'] == 1, plan


def test_graph_replayed_generate_across_a_block_edge(model):
    m, w, _ = model
    H = m.config.hidden_size
    x = rand(torch.Generator().manual_seed(9), 1, H)
    ids_seen, routes = [], []

    def step(h):
        ids, cache = m.greedy_generate(x, h, -1, 6)
        routes.append(m.decode_last_route()); ids_seen.append(ids)
        return cache

    def fed():          # the prompt row, then the embeddings of the first five tokens (the sixth is returned, not fed back)
        e = m.get_input_embeddings()(torch.tensor([ids_seen[0][:5]], device=m.device)).view(1, 5, H)
        return torch.cat([x, e.to(m.dtype)], 1)
    run_twin_step(m, w, 61, 6, step, 'greedy_generate from 61', fed)
    assert all(r in (1, 2) for r in routes), routes
    assert ids_seen[0] == ids_seen[1] and len(ids_seen[0]) == 6


@pytest.mark.parametrize('watcher', [False, True], ids=['talking', 'talking+chunk'])
def test_round_of_three_talking_streams(model, watcher):
    """mmd_round_multi: the decode rows of three streams in ONE attention launch (form 9) whose blocks prepare their own stream's k / v from per-stream offsets into the
    slabs and the table -- each arena changes at its own slot only and equals its fresh twin; optionally a 98-row chunk of a fourth stream rides in the same round"""
    m, w, _ = model
    H = m.config.hidden_size
    lengths = [63, 64, 200]
    g = torch.Generator().manual_seed(77)
    pairs = [twins(m, g, n, H) for n in lengths]
    rows = [rand(g, 1, H) for _ in lengths]
    wx = rand(g, 98, H)
    wpair = twins(m, g, 30, H) if watcher else None
    snaps = {}
    for side in (0, 1):
        samplers = [m.new_sampler() for _ in lengths]
        for s in samplers:
            s.begin(-1, None, None, 4)
        segs = [dict(x=rows[i], cache=pairs[i][side], sampler=samplers[i], sample=True) for i in range(3)]
        if watcher:
            segs.append(dict(x=wx, cache=wpair[side], head_rows=[48, 97]))
        handles = [sg['cache'] for sg in segs]
        before = [snapshot(m, h) for h in handles]
        out = m.round_multi(segs)
        plan = m.step_last_plan()
        form = (C.c_int * 2)()
        check(lib().mmd_op_attention_last_form(m._ctx, form), m._ctx)
        assert plan['run_n'] == 3, plan
        assert [len(o['cache']) for o in out[:3]] == [n + 1 for n in lengths]
        snaps[side] = (before, [snapshot(m, h) for h in handles], [o['token'] for o in out[:3]], form[0])
    if not watcher:          # (with a watcher the step's last attention launch is the chunk's: the plan's run_n above is the witness)
        assert snaps[0][3] == 9 and snaps[1][3] == 9
    assert snaps[0][2] == snaps[1][2]
    spans = [(n, n + 1) for n in lengths] + ([(30, 128)] if watcher else [])
    for i, (lo, hi) in enumerate(spans):
        what = f'round_multi stream {i} at {lo}'
        assert_step_footprint(snaps[0][0][i], snaps[0][1][i], lo, hi, what)
        assert_twins_agree(snaps[0][1][i], snaps[1][1][i], hi, what)
    anchor_layer0(m, w, rows[1], 64, snaps[0][1][1], 'round_multi stream 1')
    if watcher:
        anchor_layer0(m, w, wx, 30, snaps[0][1][3], 'round_multi watching chunk')


def test_scalar_transposed_writer_in_the_fp32_model():
    """rope_append_kernel with v_tr = 1 as the fp32 model runs it, across token 64"""
    from helpers import hip_model
    m = hip_model('A', torch.float32)[0]
    H = m.config.hidden_size
    g = torch.Generator().manual_seed(4)
    x = rand(g, 9, H, torch.float32)
    a, b = twins(m, g, 60, H)
    before = snapshot(m, a, 512)
    a1 = m(inputs_embeds=x, past_key_values=a).past_key_values
    after = snapshot(m, a, 512)
    m(inputs_embeds=x, past_key_values=b)
    fresh = snapshot(m, b, 512)
    assert len(a1) == 69
    assert_step_footprint(before, after, 60, 69, 'fp32 step S 9 at 60')
    assert_twins_agree(after, fresh, 69, 'fp32 step S 9 at 60')


@pytest.mark.parametrize('start,end', [(64, 128), (65, 300), (127, 129), (100, 320), (0, 70)])
def test_stash_and_unstash_keep_every_live_bit(model, start, end):
    m, w, _ = model
    H = m.config.hidden_size
    g = torch.Generator().manual_seed(start * 7 + end)
    ctx = m(inputs_embeds=rand(g, end, H)).past_key_values
    s0 = snapshot(m, ctx)
    stash = m.kv_stash(ctx, start)
    other = m(inputs_embeds=rand(g, 40, H), past_key_values=m.cache_prefix(ctx, start)).past_key_values
    assert len(other) == start + 40
    mid = snapshot(m, other)
    assert not same(mid[0][:, :, start:start + 40], s0[0][:, :, start:start + 40])          # the slots really were overwritten
    back = m.kv_unstash(stash)
    assert len(back) == end
    s1 = snapshot(m, back)
    up = -(-end // L.BLK) * L.BLK
    for name, x0, xm, x1 in (('K', s0[0], mid[0], s1[0]), ('V', s0[1], mid[1], s1[1])):
        assert same(x0[:, :, :end], x1[:, :, :end]), f'{name} of [0, {end}) after unstash differs in {int((ibits(x0[:, :, :end]) != ibits(x1[:, :, :end])).sum())} elements'
        assert same(xm[:, :, up:], x1[:, :, up:]), f'{name} at or above token {up} was touched by the unstash'


@pytest.mark.parametrize('vmm', [True, False], ids=['virtual-memory', 'realloc'])
def test_growth_keeps_every_live_bit(model, vmm, monkeypatch):
    """An arena that starts at 256 tokens: 100-row steps up to 700 tokens; whenever a step grows the arena the old contents [0, len) are bit-equal before and after
    (realloc: every (layer, head) row is re-pitched; virtual memory: pages are mapped behind the same addresses).  The virtual-memory arena maps whole chunks of at
    least 2 MiB per row -- thousands of tokens at this width -- so its first growth comes later: the run goes on in 1000-row steps until the capacity has changed once."""
    m, w, _ = model
    H = m.config.hidden_size
    monkeypatch.setenv('MMDUET_KV_NO_VMM', '0' if vmm else '1')
    m.release_pooled_arenas()
    g = torch.Generator().manual_seed(11)
    cache = m.new_cache(256)
    cap0 = int(lib().mmd_kv_capacity(cache.arena.h))
    stride = int(lib().mmd_kv_stride(cache.arena.h))
    assert (stride > cap0) if vmm else (stride == cap0 == 256)          # the mode asked for is the mode in use
    grown, n = 0, 0
    try:
        while n < 700 or (grown == 0 and n < 40000):
            S = 100 if n < 700 else 1000
            cap = int(lib().mmd_kv_capacity(cache.arena.h))
            will_grow = n + S > cap
            live = -(-n // L.BLK) * L.BLK
            before = snapshot(m, cache, live) if will_grow and n else None
            cache = m(inputs_embeds=rand(g, S, H), past_key_values=cache).past_key_values
            if will_grow:
                assert int(lib().mmd_kv_capacity(cache.arena.h)) > cap
                grown += 1
                if before is not None:
                    after = snapshot(m, cache, live)
                    assert same(before[0][:, :, :n], after[0][:, :, :n]) and same(before[1][:, :, :n], after[1][:, :, :n]), f'growth past {cap} tokens changed live slots below {n}'
            n += S
        assert grown >= (1 if vmm else 2), (grown, n)
    finally:
        del cache
        m.release_pooled_arenas()
