"""Stream snapshots on the device: mmd_kv_export / mmd_kv_import convert between the arena and the canonical form bit for bit (host statement:
tests/kv_snapshot_cases.py over tests/kv_layout.py), mmd_kv_fork copies an arena into another of a different capacity and pitch, the refusals change nothing, and
a context that went through kv_save + kv_load or kv_fork continues exactly as the original does -- after a drop, in chunks, over both decode routes and in another
model instance.  Copies are exact: no tolerance appears anywhere.  The models are the two of tests/test_gpu_kv_drop.py."""
import ctypes as C
import pytest
import torch

pytestmark = pytest.mark.gpu
import kv_layout as L
import kv_snapshot_cases as S
from oracle import duet_oracle as O
from rawops import guarded, sentinel_intact
from mmduet_amd._lib import lib, check
from mmduet_amd.modeling_live import _ptr, KVSnapshot
from helpers import hip_model

BF = torch.bfloat16
N = S.CTX_LEN


def build_bf16(graph):
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    ocfg = O.OracleConfig(vocab_size=2048, num_hidden_layers=2, vit_layers=1)
    w = O.random_weights(ocfg, seed=3, dtype=BF, scale='unit')
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=2, vit_num_hidden_layers=2, vit_layers_removed=1,
                                        frame_num_tokens=49, frame_resolution=384, v_placeholder='<image>')
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('MMDUET_GRAPH', '1' if graph else '0')
        m = VideoHeadLiveLlavaQwenForCausalLM(pcfg, torch_dtype=BF, max_vit_batch=1, max_step_tokens=1024, kv_initial_tokens=1024)
    m.load_state_dict(w)
    return m


@pytest.fixture(scope='module')
def bf16_model():
    """the 2-layer true-width bf16 model of tests/test_gpu_kv_drop.py (nkv 4, d 128, vocab 2048), captured decode step on"""
    return build_bf16(True)


@pytest.fixture(scope='module')
def bf16_eager_model():
    """a second instance from the same weights whose decode steps are launched one by one"""
    return build_bf16(False)


@pytest.fixture(scope='module')
def f32_model():
    """the fp32 tiny model (nkv 2, d 16)"""
    return hip_model('A', torch.float32)[0]


@pytest.fixture(params=['bf16', 'fp32'])
def model(request):
    return request.getfixturevalue('bf16_model' if request.param == 'bf16' else 'f32_model')


def geometry(m):
    c = m.config
    return c.num_hidden_layers, c.num_key_value_heads, c.head_dim


def rand_rows(seed, rows, m):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, rows, m.config.hidden_size, generator=g) * 0.5).to(m.dtype).cuda()


def filled(m, n=N, seed=11):
    """a context of n tokens written by real steps"""
    cache = m(inputs_embeds=rand_rows(seed, n, m)).past_key_values
    assert len(cache) == n
    return cache


def arena_image(m, h, n64):
    """the first n64 slots of every layer AS STORED -> (K [layers, nkv, n64, d], V_raw [layers, nkv, n64 / 64, d, 64])"""
    layers, nkv, d = geometry(m)
    K = torch.empty(layers, nkv, n64, d, dtype=m.dtype, device=m.device)
    V = torch.empty(layers, nkv, n64 // L.BLK, d, L.BLK, dtype=m.dtype, device=m.device)
    m._bind_stream()
    for i in range(layers):
        check(lib().mmd_kv_debug_read(h, i, n64, _ptr(K[i]), _ptr(V[i])), m._ctx, 'mmd_kv_debug_read')
    return K, V


def ibits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(ibits(a), ibits(b))


def where(a, b):
    """for a failing comparison: how many elements differ, and the first few indices"""
    bad = (ibits(a) != ibits(b)).nonzero()
    return f'{bad.shape[0]} of {a.numel()} elements differ, the first at {bad[:8].tolist()}'


def same_image(a, b):
    return same(a[0], b[0]) and same(a[1], b[1])


def canonical_of(image, frm, to):
    """the host statement over every layer: -> (K, V) [layers, nkv, to - frm, d]"""
    per = [S.canonical(image[0][i], image[1][i], frm, to) for i in range(image[0].shape[0])]
    return torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per])


def imported_into(image, at, Kc, Vc):
    per = [S.imported(image[0][i], image[1][i], at, Kc[i], Vc[i]) for i in range(image[0].shape[0])]
    return torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per])


class RawStream:
    """an arena of the model driven through the C ABI alone: made by model.new_cache (taken from the model's arena pool, or created when the pool has none that fits)
    and given back to the pool, which resets what it hands out.  No test of this module destroys an arena before the module ends (DESIGN.md section 5 "Snapshots")."""

    def __init__(self, m, initial_tokens=256):
        self.m, self.cache = m, m.new_cache(initial_tokens)
        self.h = self.cache.arena.h
        assert self.len() == 0 and self.position() == 0

    def len(self):
        return int(lib().mmd_kv_len(self.h))

    def position(self):
        return int(lib().mmd_kv_position(self.h))

    def capacity(self):
        return int(lib().mmd_kv_capacity(self.h))

    def imp(self, Kc, Vc):
        self.m._bind_stream()
        Kc, Vc = Kc.contiguous(), Vc.contiguous()
        rc = lib().mmd_kv_import(self.h, _ptr(Kc), _ptr(Vc), Kc.shape[2])
        torch.cuda.synchronize()
        return rc

    def close(self):
        self.cache = self.h = None


@pytest.fixture
def raw_streams():
    made = []

    def make(m, initial_tokens=256):
        made.append(RawStream(m, initial_tokens))
        return made[-1]
    yield make
    torch.cuda.synchronize()
    for s in made:
        s.close()


def random_canonical(m, n, seed):
    layers, nkv, d = geometry(m)
    g = torch.Generator(device='cuda').manual_seed(seed)
    return tuple((torch.randn(layers, nkv, n, d, generator=g, device='cuda') + 3.0).to(m.dtype) for _ in range(2))


# ---- export --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('span', S.EXPORT_SPANS, ids=lambda c: '-'.join(map(str, c)))
def test_export_equals_the_canonical_form_of_the_arena(model, span):
    m = model
    frm, to = span
    layers, nkv, d = geometry(m)
    cache = filled(m)
    want_k, want_v = canonical_of(arena_image(m, cache.arena.h, S.up64(N)), frm, to)
    rows = layers * nkv * (to - frm)
    kbuf, kview = guarded(rows, d, m.dtype, m.device)
    vbuf, vview = guarded(rows, d, m.dtype, m.device)
    m._bind_stream()
    check(lib().mmd_kv_export(cache.arena.h, frm, to, _ptr(kview), _ptr(vview)), m._ctx, 'mmd_kv_export')
    torch.cuda.synchronize()
    assert same(kview.view(layers, nkv, to - frm, d), want_k), f'K differs in {int((ibits(kview.view_as(want_k)) != ibits(want_k)).sum())} elements'
    assert same(vview.view(layers, nkv, to - frm, d), want_v), f'V differs in {int((ibits(vview.view_as(want_v)) != ibits(want_v)).sum())} elements'
    for buf in (kbuf, vbuf):
        assert sentinel_intact(buf[:16]) and sentinel_intact(buf[16 + rows:])
    assert len(cache) == N == int(lib().mmd_kv_len(cache.arena.h))


# ---- import --------------------------------------------------------------------------------------------------------------------------------------------------
def dirty_stream(m, raw_streams):
    """a fresh stream of length 0 whose first 256 slots hold finite values that are not zero, and that image"""
    s = raw_streams(m)
    assert s.imp(*random_canonical(m, 256, 5)) == S.MMD_OK and s.len() == 256
    check(lib().mmd_kv_truncate(s.h, 0), m._ctx, 'mmd_kv_truncate')
    image = arena_image(m, s.h, 256)
    assert bool((image[1].float() != 0).all())
    return s, image


def test_import_reproduces_the_source_arena(model, raw_streams):
    m = model
    cache = filled(m)
    src = arena_image(m, cache.arena.h, S.up64(N))
    Kc, Vc = canonical_of(src, 0, N)
    s, before = dirty_stream(m, raw_streams)
    assert s.imp(Kc, Vc) == S.MMD_OK
    assert s.len() == N and s.position() == N
    after = arena_image(m, s.h, 256)
    assert same(after[0][:, :, :N], src[0][:, :, :N]), where(after[0][:, :, :N], src[0][:, :, :N])
    for i in range(after[1].shape[0]):
        assert same(L.v_logical(after[1][i])[:, :N], L.v_logical(src[1][i])[:, :N]), where(L.v_logical(after[1][i])[:, :N], L.v_logical(src[1][i])[:, :N])
    assert same_image(after, imported_into(before, 0, Kc, Vc))          # ... and slots [N, 256) kept what they held


@pytest.mark.parametrize('split', S.IMPORT_SPLITS)
def test_import_in_two_pieces(model, raw_streams, split):
    m = model
    cache = filled(m)
    Kc, Vc = canonical_of(arena_image(m, cache.arena.h, S.up64(N)), 0, N)
    s, before = dirty_stream(m, raw_streams)
    whole = imported_into(before, 0, Kc, Vc)
    assert s.imp(Kc[:, :, :split], Vc[:, :, :split]) == S.MMD_OK and s.len() == split
    first = arena_image(m, s.h, 256)
    assert same_image(first, imported_into(before, 0, Kc[:, :, :split], Vc[:, :, :split]))
    assert s.imp(Kc[:, :, split:], Vc[:, :, split:]) == S.MMD_OK and s.len() == N
    both = arena_image(m, s.h, 256)
    assert same_image(both, imported_into(first, split, Kc[:, :, split:], Vc[:, :, split:]))          # the older tokens of the shared V block are untouched
    assert same_image(both, whole)


def test_import_grows_the_arena(model, raw_streams):
    m = model
    s = raw_streams(m)
    cap0 = s.capacity()
    head = random_canonical(m, 70, 7)
    assert s.imp(*head) == S.MMD_OK
    n = cap0                    # 70 tokens are in: the import ends 70 tokens beyond what is backed by memory (which is at least kv_initial_tokens: whole mapping chunks)
    tail = random_canonical(m, n, 8)
    assert s.imp(*tail) == S.MMD_OK
    assert s.len() == cap0 + 70 and s.capacity() > cap0
    K, V = arena_image(m, s.h, S.up64(cap0 + 70))
    want_k, want_v = torch.cat([head[0], tail[0]], 2), torch.cat([head[1], tail[1]], 2)
    assert same(K[:, :, :cap0 + 70], want_k)
    for i in range(V.shape[0]):
        assert same(L.v_logical(V[i])[:, :cap0 + 70], want_v[i])


def test_refusals_change_nothing(f32_model, bf16_model, raw_streams):
    m = f32_model
    cache = m.kv_drop(filled(m, N + 2), 3, 5)          # a position offset to keep
    h = cache.arena.h
    layers, nkv, d = geometry(m)
    before = arena_image(m, h, 256)

    def unchanged():
        return int(lib().mmd_kv_len(h)) == N and int(lib().mmd_kv_position(h)) == N + 2 and same_image(before, arena_image(m, h, 256))
    assert unchanged()
    kbuf, kview = guarded(layers * nkv * 8, d, m.dtype, m.device)
    vbuf, vview = guarded(layers * nkv * 8, d, m.dtype, m.device)
    m._bind_stream()
    for (f, t), code in S.REFUSED_EXPORTS:
        assert lib().mmd_kv_export(h, f, t, _ptr(kview), _ptr(vview)) == code, (f, t)
        torch.cuda.synchronize()
        assert sentinel_intact(kbuf) and sentinel_intact(vbuf) and unchanged(), (f, t)
    assert 'kv_export' in lib().mmd_last_error(m._ctx).decode()
    # the position may not fall below the length; at or above it is taken
    assert lib().mmd_kv_set_position(h, N - 1) == S.MMD_ERANGE and lib().mmd_kv_set_position(h, -1) == S.MMD_ERANGE and unchanged()
    assert lib().mmd_kv_set_position(h, N + 50) == S.MMD_OK and int(lib().mmd_kv_position(h)) == N + 50
    assert lib().mmd_kv_set_position(h, N + 2) == S.MMD_OK and unchanged()
    # import while a stash is held: refused; export: allowed (it only reads)
    Kc, Vc = random_canonical(m, 8, 9)
    stash = m.kv_stash(cache, 60)
    assert lib().mmd_kv_import(h, _ptr(Kc), _ptr(Vc), 8) == S.MMD_EINVAL and unchanged()
    assert 'stash' in lib().mmd_last_error(m._ctx).decode()
    assert lib().mmd_kv_export(h, 56, 64, _ptr(kview), _ptr(vview)) == S.MMD_OK
    torch.cuda.synchronize()
    want = canonical_of(before, 56, 64)
    assert same(kview.view_as(want[0]), want[0]) and same(vview.view_as(want[1]), want[1])
    cache = m.kv_unstash(stash)
    assert unchanged()
    assert lib().mmd_kv_import(h, _ptr(Kc), _ptr(Vc), -1) == S.MMD_ERANGE and unchanged()
    # fork onto itself, across contexts, onto a stream that holds a stash, of more tokens than the source has
    other = raw_streams(bf16_model)
    mine = raw_streams(m)
    assert lib().mmd_kv_fork(h, h, 10) == S.MMD_EINVAL and unchanged()
    assert lib().mmd_kv_fork(other.h, h, 10) == S.MMD_EINVAL and other.len() == 0 and unchanged()
    assert lib().mmd_kv_fork(h, other.h, 0) == S.MMD_EINVAL and unchanged()
    assert lib().mmd_kv_fork(mine.h, h, N + 1) == S.MMD_ERANGE and lib().mmd_kv_fork(mine.h, h, -1) == S.MMD_ERANGE and mine.len() == 0 and unchanged()
    assert mine.imp(*random_canonical(m, 30, 10)) == S.MMD_OK
    check(lib().mmd_kv_stash(mine.h, 10, 30), m._ctx, 'mmd_kv_stash')
    held = arena_image(m, mine.h, 64)
    assert lib().mmd_kv_fork(mine.h, h, 10) == S.MMD_EINVAL and mine.len() == 30 and same_image(held, arena_image(m, mine.h, 64)) and unchanged()
    # the Python surface: a stale handle raises, a foreign one too
    longer = m(inputs_embeds=rand_rows(3, 4, m), past_key_values=cache).past_key_values
    m(inputs_embeds=rand_rows(4, 2, m), past_key_values=cache)
    assert longer.stale
    for call in (m.kv_save, m.kv_fork):
        with pytest.raises(RuntimeError, match='stale'):
            call(longer)
        with pytest.raises(TypeError):
            call(bf16_model.new_cache())


# ---- fork ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fork_destinations():
    """per model, one stream made for the fork tests with another capacity AND another row pitch than the model's own arenas; reset between uses, destroyed at the end"""
    made = {}

    def get(m, cap):
        if id(m) not in made:
            h = C.c_void_p()
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv('MMDUET_KV_VIRTUAL_TOKENS', str(4 * cap))
                check(lib().mmd_stream_create(m._ctx, 3 * cap + 1, C.byref(h)), m._ctx, 'mmd_stream_create')          # (no pooled arena has grown that far)
            made[id(m)] = h
        check(lib().mmd_stream_reset(made[id(m)]), m._ctx, 'mmd_stream_reset')
        return made[id(m)]
    yield get
    torch.cuda.synchronize()
    for h in made.values():
        lib().mmd_stream_destroy(h)


@pytest.mark.parametrize('n', S.FORK_LENGTHS)
def test_fork_copies_the_arena_and_leaves_the_source(model, fork_destinations, n):
    m = model
    cache = m.kv_drop(filled(m, N + 10), 3, 13)
    src = cache.arena.h
    assert int(lib().mmd_kv_len(src)) == N and int(lib().mmd_kv_position(src)) == N + 10
    cap = int(lib().mmd_kv_capacity(src))
    whole = arena_image(m, src, cap)                       # every mapped byte of the source
    dh = fork_destinations(m, cap)
    dst_cap, dst_stride = int(lib().mmd_kv_capacity(dh)), int(lib().mmd_kv_stride(dh))
    assert dst_cap != cap and dst_stride != int(lib().mmd_kv_stride(src))
    print(f'source: capacity {cap}, row stride {int(lib().mmd_kv_stride(src))}; destination: capacity {dst_cap}, row stride {dst_stride}')
    m._bind_stream()
    check(lib().mmd_kv_fork(dh, src, n), m._ctx, 'mmd_kv_fork')
    torch.cuda.synchronize()
    assert int(lib().mmd_kv_len(dh)) == n and int(lib().mmd_kv_position(dh)) == n + 10
    got = arena_image(m, dh, S.up64(n))
    assert same(got[0][:, :, :n], whole[0][:, :, :n])
    for i in range(got[1].shape[0]):
        assert same(L.v_logical(got[1][i])[:, :n], L.v_logical(whole[1][i])[:, :n])
    assert bool(torch.isfinite(got[1].float()).all())
    assert same_image(whole, arena_image(m, src, cap)) and int(lib().mmd_kv_len(src)) == N and int(lib().mmd_kv_position(src)) == N + 10


# ---- continuation --------------------------------------------------------------------------------------------------------------------------------------------
def continuation(m, cache, route=None):
    """one chunk step of 50 rows, then a greedy response of 8 tokens -> (hidden rows [50, H], ids, position behind the response)"""
    out = m(inputs_embeds=rand_rows(21, 50, m), past_key_values=cache)
    ids, after = m.greedy_generate(rand_rows(22, 3, m), out.past_key_values, -1, 8)
    if route is not None:
        assert m.decode_last_route() in route, m.decode_last_route()
    assert len(ids) == 8
    return out.hidden_states[0].clone(), ids, m.kv_position(after)


def hidden_gap(a, b):
    return float((a[0].float() - b[0].float()).abs().max())


def assert_continues_like(m, original, others, route=None):
    """The control: the original continued twice from the same handle.  A bit-identical control pair demands bit identity of every other run; a control pair that
    differs would allow the others its own largest difference in the hidden rows -- and ids equal to one of the pair's."""
    ref, again = continuation(m, original, route), continuation(m, original, route)
    control = hidden_gap(ref, again)
    print(f'control pair: max |hidden difference| {control:.4g}, ids {ref[1]} / {again[1]}')
    for name, cache in others.items():
        got = continuation(m, cache, route)
        print(f'{name}: max |hidden difference| to the original {hidden_gap(ref, got):.4g}, ids {got[1]}')
        assert got[2] == ref[2], name
        if control == 0.0 and ref[1] == again[1]:
            assert same(got[0], ref[0]) and got[1] == ref[1], name
        else:
            assert hidden_gap(ref, got) <= control and got[1] in (ref[1], again[1]), name


def routes_of(name):
    return {'bf16': (1, 2), 'bf16_eager': (0,), 'fp32': (0,)}[name]


@pytest.fixture(params=['bf16', 'bf16_eager', 'fp32'])
def routed_model(request):
    return request.getfixturevalue({'bf16': 'bf16_model', 'bf16_eager': 'bf16_eager_model', 'fp32': 'f32_model'}[request.param]), routes_of(request.param)


def test_loaded_and_forked_contexts_continue_like_the_original(routed_model):
    """The control pair measured bit-identical on every model and route here, so the loaded and the forked runs are held to bit identity."""
    m, route = routed_model
    c = filled(m)
    snap = m.kv_save(c)
    assert snap.length == N and snap.position == N and snap.K.is_pinned()
    assert_continues_like(m, c, {'loaded': m.kv_load(snap), 'forked': m.kv_fork(c)}, route)
    assert not c.stale and len(c) == N


def test_continuation_after_a_drop_carries_the_position(routed_model):
    m, route = routed_model
    c = m.kv_drop(filled(m), 40, 90)
    assert len(c) == N - 50 and m.kv_position(c) == N
    snap = m.kv_save(c, pin=False)
    assert snap.length == N - 50 and snap.position == N and not snap.K.is_pinned()
    loaded, forked = m.kv_load(snap), m.kv_fork(c)
    assert m.kv_position(loaded) == N == m.kv_position(forked) and len(loaded) == N - 50 == len(forked)
    assert_continues_like(m, c, {'loaded': loaded, 'forked': forked}, route)


def test_chunked_save_and_load(model, tmp_path):
    """staging budgets that force 3 and more chunks on either side, and the file round trip in between"""
    m = model
    layers, nkv, d = geometry(m)
    token_bytes = 2 * layers * nkv * d * (2 if m.dtype == BF else 4)
    c = filled(m)
    one = m.kv_save(c)
    from mmduet_amd.modeling_live import snapshot_chunks
    for budget in (token_bytes * 70, token_bytes * 7 + 5, 1):
        assert len(snapshot_chunks(N, token_bytes, budget)) >= 3
        snap = m.kv_save(c, staging_bytes=budget)
        assert same(snap.K, one.K) and same(snap.V, one.V) and snap.position == one.position
    want = canonical_of(arena_image(m, c.arena.h, S.up64(N)), 0, N)
    assert same(one.K.cuda(), want[0]) and same(one.V.cuda(), want[1])
    p = str(tmp_path / 'ctx.pt')
    one.save(p)
    loaded = m.kv_load(KVSnapshot.load(p), staging_bytes=token_bytes * 70)
    assert same_image(arena_image(m, loaded.arena.h, 192), arena_image(m, c.arena.h, 192))
    assert_continues_like(m, c, {'loaded in 3 chunks': loaded, 'loaded token by token': m.kv_load(one, staging_bytes=1)})


def test_snapshot_moves_between_model_instances(bf16_model, bf16_eager_model, f32_model):
    """saved from one instance, loaded into a second one built from the same weights: it continues as the second instance's own context of the same inputs does"""
    a, b = bf16_model, bf16_eager_model
    snap = KVSnapshot.from_state_dict(a.kv_save(a.kv_drop(filled(a), 40, 90)).state_dict())
    own = b.kv_drop(filled(b), 40, 90)
    mine = b.kv_save(own)
    assert same(mine.K, snap.K) and same(mine.V, snap.V) and mine.position == snap.position == N          # (the two instances wrote the same context)
    assert_continues_like(b, own, {'loaded from the other instance': b.kv_load(snap)}, (0,))
    # and back, onto the captured decode step
    assert_continues_like(a, a.kv_drop(filled(a), 40, 90), {'loaded from the other instance': a.kv_load(mine)}, (1, 2))
    # a model of another geometry or dtype refuses it, naming the field
    with pytest.raises(ValueError, match='dtype'):
        f32_model.kv_load(snap)
    wrong = KVSnapshot(snap.K.float(), snap.V.float(), snap.position, torch.float32, snap.layers, snap.kv_heads, snap.head_dim, snap.inv_freq)
    with pytest.raises(ValueError, match='layers|kv_heads|head_dim'):
        f32_model.kv_load(wrong)
    # empty and None contexts give empty snapshots, which load as empty contexts
    for empty in (a.kv_save(None), a.kv_save(a.new_cache())):
        assert empty.length == 0 and empty.position == 0
        got = a.kv_load(empty)
        assert len(got) == 0 and not got and a.kv_position(got) == 0
    assert len(a.kv_fork(None)) == 0


# ---- isolation -----------------------------------------------------------------------------------------------------------------------------------------------
def mutate(m, cache):
    """extend, truncate and drop: everything that rewrites an arena in place"""
    longer = m(inputs_embeds=rand_rows(31, 30, m), past_key_values=cache).past_key_values
    back = m(inputs_embeds=rand_rows(32, 5, m), past_key_values=m.cache_prefix(longer, 100)).past_key_values
    stash = m.kv_stash(back, 60)
    m(inputs_embeds=rand_rows(33, 70, m), past_key_values=m.cache_prefix(back, 60))
    back = m.kv_unstash(stash)
    return m.kv_drop(back, 10, 50)


@pytest.mark.parametrize('touched', ['fork', 'original'])
def test_fork_and_original_do_not_see_each_other(model, touched):
    m = model
    c = filled(m)
    f = m.kv_fork(c)
    assert f.arena is not c.arena and f.arena.h.value != c.arena.h.value
    watch, work = (c, f) if touched == 'fork' else (f, c)
    x = rand_rows(41, 9, m)
    before_step = m(inputs_embeds=x, past_key_values=watch).hidden_states[0].clone()
    image = arena_image(m, watch.arena.h, 256)
    done = mutate(m, work)
    assert len(done) == 65 and m.kv_position(done) == 105
    assert not watch.stale and len(watch) == N and m.kv_position(watch) == N
    assert same_image(image, arena_image(m, watch.arena.h, 256))
    assert same(m(inputs_embeds=x, past_key_values=watch).hidden_states[0], before_step)
    assert same_image(image, arena_image(m, watch.arena.h, 256))


# ---- ranking candidate answers -------------------------------------------------------------------------------------------------------------------------------
def test_ranking_by_fork_equals_truncate_and_rerun(model):
    """3 candidates of different lengths scored with forward(labels=...): once per fork of the context, and one after the other on the one arena.  The control pair
    (the sequential route twice) measured bit-identical, so the forks are held to bit identity."""
    m = model
    c = filled(m)
    g = torch.Generator().manual_seed(51)
    cands = [torch.randint(0, m.config.vocab_size, (1, n), generator=g).cuda() for n in (3, 7, 12)]

    def score(ids, cache):
        e = m.get_input_embeddings()(ids).view(1, ids.shape[1], -1)
        labels = torch.cat([ids[:, 1:], torch.full((1, 1), -100, device=ids.device)], 1)
        out = m(inputs_embeds=e, past_key_values=cache, labels=labels)
        return out.lm_loss.float().reshape(1).clone()
    seq, seq2 = ([score(ids, c) for ids in cands] for _ in range(2))
    forks = [m.kv_fork(c) for _ in cands]
    forked = [score(ids, f) for ids, f in zip(cands, forks)]
    control = max(float((a - b).abs()) for a, b in zip(seq, seq2))
    print(f'sequential NLLs {[float(s) for s in seq]}, control difference {control:.4g}; forked {[float(s) for s in forked]}')
    assert all(bool(torch.isfinite(s)) for s in seq) and len({float(s) for s in seq}) == 3
    for a, b in zip(seq, forked):
        if control == 0.0:
            assert same(a, b)
        else:
            assert float((a - b).abs()) <= control
    assert not c.stale and all(not f.stale and len(f) == N for f in forks)
