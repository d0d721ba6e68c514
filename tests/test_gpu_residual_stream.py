"""Every writer of the residual stream h and of its RMSNorm image, at operator level (tests/residual_stream.py states the rounding points and holds the case lists).

The tile schedule's writers (EPI_RESID epilogues, rmsnorm kernels) have their parity tests in tests/test_gpu_ops.py and tests/test_gpu_stress_gemm.py.  Here:

  slab consumer   mmd_op_slab_resid_rmsnorm: slab_resid_rmsnorm_kernel<4 / 8 / 16>.  h_out equals residual_stream.slab_resid BIT FOR BIT on slabs whose sum depends on the
                  order of the adds; xn_out is inside rms_image's rule applied to the device's own h_out; in place and apart, with and without wscale.
  chain producer  mmd_op_gemv_chain role 2: h inside the element-wise `resid` bound of the stress GEMM tests, ssq[m][t] within 2^-19 of the tile sums of the device's own new
                  h, nothing else touched; and with operands whose dot products are exact in fp32, h bit for bit (the two roundings).
  chain consumer  mmd_op_gemv_chain role 1, both forms (fp32 slabs as layer_qkv, SwiGLU as layer_tail_chain's gate_up): inside the bound for a float64 product with
                  xn_ref = rnd(gamma * rnd(h * inv)); rows of h at scales 1e-2, 1, 30, 1e3; X is NaN and never read; ssq spread over all 256 entries gives the same result.

Case table of the consumer (residual_stream.CONSUMER_CASES; read back from mmd_op_gemm_last_plan and asserted in test_chain_consumer):
  case                   epi     N      K     weights  K splits  k per wave  prologue passes     ragged
  qkv, qkv_w8            slabs   4608   3584  bf16/fp8     2        448      one (< 512)           no
  qkv_k4096              slabs    512   4096  bf16         2        512      one, full             no
  qkv_k4096_one_slab     slabs    512   4096  bf16         1       1024      two, full (limit)     no
  qkv_k96                slabs     16     96  bf16         2         32      one                   yes (3 k-tiles over 2 x 4 waves)
  gate_up, gate_up_w8    SwiGLU  37888  3584  bf16/fp8     1        896      two, second partly    no
  gate_up_k4096          SwiGLU     64  4096  bf16         1       1024      two, full (limit)     no
  gate_up_k1056          SwiGLU     32  1056  bf16         1        288      one                   yes (33 k-tiles over 4 waves)
Slab consumer: last_plan reports the instantiation: <4> for 1, 2, 4 slabs, <8> for 5, 8, <16> for 9, 16 (residual_stream.SLAB_MAXS).

Mutants (throw-away builds, never committed, one run each on an MI355X; all of them compute wrong numbers inside their own buffers).  "new" is this file (93 tests); "old" is
tests/test_gpu_trueshape.py::test_fused_and_unfused_schedules_agree, ::test_llm_steps_true_shape and tests/test_gpu_step_regimes.py (52 tests) -- the rest of the old suite was
not run against the mutants:
  (a) the consumer's chain_prologue takes row 0's ssq (hence its 1/rms) for every row.
      new: 18 fail -- every case of test_chain_consumer at M = 3 and 4 (M = 1 has only row 0).  old: all 52 pass.
  (b) chain_prologue stores only its first pass of 512 k.
      new: 12 fail -- the test_chain_consumer cases whose waves hold more than 512 k: qkv_k4096_one_slab, gate_up, gate_up_w8, gate_up_k4096, at every M.
      old: 10 fail -- both true-shape tests and 8 rows of test_step_takes_the_plan_of_the_table (its isfinite check: the unwritten LDS reaches the logits).
  (c) the producer rounds once, rnd(gemm + h).
      new: 3 fail -- test_chain_producer_rounds_twice (every M); the bound of test_chain_producer cannot see it (one rounding is closer to float64 than two).  old: all 52 pass.
  (d) slab_resid_rmsnorm_kernel adds its slabs last to first.
      new: 25 fail -- test_slab_consumer at 4, 5, 8, 9 and 16 slabs, every H (1 and 2 slabs have one order).  old: test_fused_and_unfused_schedules_agree fails, 51 pass.
  (e) wscale multiplies rnd(sum) -- rnd(rnd(rnd(sum) * wscale) + resid) -- instead of the fp32 sum.
      new: all 35 cases of test_slab_consumer fail.  old: all 52 pass.
  (f) the <8> instantiation is launched up to 9 slabs.
      new: 5 fail -- test_slab_consumer at 9 slabs, every H (the first assertion to fail is the instantiation read from last_plan).  old: both true-shape tests fail, 50 pass.
With the unmodified kernels every test of this file passes: none exposed a bug in a writer.  Worst |Y - ref| / bound seen: producer 0.98, consumer SwiGLU 0.66, consumer slabs
0.015; ssq relative error 1.2e-7 against 2^-19.
"""
import zlib
import pytest
import torch

pytestmark = pytest.mark.gpu
import gemm_regimes as T
import residual_stream as RS
import stress_inputs as SI
from rawops import RawOps, SENTINEL_BITS, _INT_OF, guarded, sentinel_intact

BF = torch.bfloat16
EPS = 1e-6
C_ACC = SI.C_ACC


@pytest.fixture(scope='module')
def ops():
    return RawOps(BF)


@pytest.fixture(scope='module')
def ops_f32():
    return RawOps(torch.float32)


@pytest.fixture(scope='module')
def env():
    e = {}
    yield e
    e.clear()
    torch.cuda.empty_cache()


def sentinel(shape, dtype, dev):
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(_INT_OF[dtype]).fill_(SENTINEL_BITS[dtype])
    return t


def bits(t):
    return t.contiguous().view(_INT_OF[t.dtype])


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def guards_intact(buf, rows, before=16):
    return sentinel_intact(buf[:before]) and sentinel_intact(buf[before + rows:])


def check(name, Y, ref, tol):
    """every element finite and inside its own bound; prints the worst |Y - ref| / bound"""
    assert torch.isfinite(Y.float()).all(), (name, 'not finite')
    d = (Y.double() - ref).abs()
    bad = ~(d <= tol)
    if int(bad.sum()):
        i = int(torch.argmax(torch.where(bad, d / tol.clamp_min(1e-30), torch.zeros_like(d))))
        m, n = divmod(i, ref.shape[1])
        pytest.fail(f'{name}: {int(bad.sum())} of {ref.numel()} elements outside the bound; worst at ({m}, {n}): Y {float(Y[m, n])} ref {float(ref[m, n])} tol {float(tol[m, n]):.3e}')
    print(f'{name}: worst |Y - ref| / bound {float((d / tol.clamp_min(1e-30)).max()):.3f}')


def weights(env, ops, N, K, fp8, swiglu):
    """one matrix per (shape, format), made once per module: W as the entry takes it, q8 / scale for fp8, and its float64 image (fp8: bf16(q) x scale, what the kernel multiplies by)"""
    key = (N, K, fp8, swiglu)
    if key not in env:
        W = SI.weights(N, K, seed=zlib.crc32(repr(key).encode()), device=ops.dev)
        if swiglu:
            W = SI.swiglu_interleave(W)
        if fp8:
            Wq, q8, sc = ops.quantize_fp8(W)
            env[key] = dict(W=Wq, q8=q8, sc=sc, Wd=Wq.double() * sc.double()[:, None])
        else:
            env[key] = dict(W=W, q8=None, sc=None, Wd=W.double())
    return env[key]


# ---- slab consumer ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', RS.SLAB_HS)
@pytest.mark.parametrize('splits', RS.SLAB_SPLITS)
def test_slab_consumer(ops, splits, H):
    dev = ops.dev
    for M in RS.SLAB_MS:
        slabs, resid, gamma, wscale = RS.slab_inputs(splits, M, H, seed=splits * 8192 + H + M, device=dev)
        for ws in (None, wscale):
            what = f'splits {splits} M {M} H {H} wscale {ws is not None}'
            want = RS.slab_resid(slabs, resid, ws)
            out = []
            for mode in ('apart', 'again', 'in_place'):
                hbuf, h = guarded(M, H, BF, dev, after=16)
                xbuf, xn = guarded(M, H, BF, dev, after=16)
                r = resid
                if mode == 'in_place':          # as the model passes it: h_out is the residual itself
                    h.copy_(resid); r = h
                assert ops.slab_resid_rmsnorm(slabs, r, h, gamma, EPS, xn, ws) == 0, what
                assert ops.last_plan() == (RS.OP_PLAN_SLAB_RESID, RS.SLAB_MAXS[splits], splits, M), (what, ops.last_plan())
                assert guards_intact(hbuf, M) and guards_intact(xbuf, M), (what, mode)
                out.append((h, xn))
            h, xn = out[0]
            diff = int((bits(h) != bits(want)).sum())
            assert diff == 0, f'{what}: {diff} of {h.numel()} elements of h_out differ from rnd(rnd(sum * wscale) + resid)'
            exc = RS.rms_image_excess(xn, h, gamma, EPS)
            assert torch.isfinite(xn.float()).all() and exc.max().item() <= 0, (what, exc.max().item(), int(exc.argmax()) // H)
            if M >= 3:
                assert float(h[1].float().abs().max()) >= 9e3 and bool((h[2] == 0).all()) and bool((xn[2] == 0).all()), what
            for mode, (h2, xn2) in zip(('again', 'in_place'), out[1:]):
                assert same_bits(h2, h) and same_bits(xn2, xn), (what, mode)


@pytest.mark.parametrize('bad', RS.SLAB_REFUSED, ids=[f'{k}_{v}' for d in RS.SLAB_REFUSED for k, v in d.items()])
def test_slab_consumer_refusals(ops, bad):
    dev = ops.dev
    M, H, splits = 3, bad.get('H', 1024), bad.get('splits', 4)
    slabs = torch.zeros(max(splits, 1), M, H + 4, device=dev)          # (room for what is asked: nothing may be launched anyway)
    resid = torch.zeros(M, H + 4, dtype=BF, device=dev); gamma = torch.ones(H + 4, dtype=BF, device=dev)
    hbuf, h = guarded(M, H + 4, BF, dev, after=16); xbuf, xn = guarded(M, H + 4, BF, dev, after=16)
    assert ops.slab_resid_rmsnorm(slabs, resid, h, gamma, EPS, xn, None, splits=splits, M=M, H=H) != 0
    assert sentinel_intact(hbuf) and sentinel_intact(xbuf)


def test_slab_consumer_refuses_an_fp32_context_and_missing_operands(ops, ops_f32):
    for o, missing in ((ops_f32, None), (ops, 'slabs'), (ops, 'resid'), (ops, 'gamma'), (ops, 'xn')):
        dev = o.dev
        slabs = torch.zeros(2, 3, 1024, device=dev); resid = torch.zeros(3, 1024, dtype=BF, device=dev); gamma = torch.ones(1024, dtype=BF, device=dev)
        hbuf, h = guarded(3, 1024, BF, dev, after=16); xbuf, xn = guarded(3, 1024, BF, dev, after=16)
        rc = o.slab_resid_rmsnorm(None if missing == 'slabs' else slabs, None if missing == 'resid' else resid, h, None if missing == 'gamma' else gamma, EPS,
                                  None if missing == 'xn' else xn, None, splits=2, M=3, H=1024)
        assert rc != 0 and sentinel_intact(hbuf) and sentinel_intact(xbuf), missing


# ---- chain producer ----------------------------------------------------------------------------------------------------------------------------------------
def run_producer(ops, X, wt, h0, M, N, K):
    """-> (h buffer, h, ssq buffer, ssq) after one producer launch on fresh guarded buffers holding h0"""
    hbuf, h = guarded(M, N, BF, ops.dev, after=16)
    sbuf, ssq = guarded(M, RS.SSQ_STRIDE, torch.float32, ops.dev, after=16)
    h.copy_(h0)
    rc, _ = ops.gemv_chain(2, X, wt['W'], h, ssq, M, N, K, q8=wt['q8'], scale=wt['sc'])
    assert rc == 0, (rc, M, N, K)
    assert ops.last_plan() == (T.GEMV16, N // 16, 1, N // 16), ops.last_plan()          # one 16-wave block per n-tile over all of K
    return hbuf, h, sbuf, ssq


def check_producer_footprint(name, hbuf, h, sbuf, ssq, M, N):
    nt = N // 16
    assert guards_intact(hbuf, M), f'{name}: rows of h outside [0, {M}) changed'
    assert guards_intact(sbuf, M), f'{name}: rows of ssq outside [0, {M}) changed'
    assert nt == RS.SSQ_STRIDE or sentinel_intact(ssq[:, nt:]), f'{name}: ssq entries past n-tile {nt} changed'
    want = RS.tile_ssq(h).double(); got = ssq[:, :nt].double()
    rel = ((got - want).abs() / want.clamp_min(1e-300)).masked_fill(want == 0, 0.0)
    print(f'{name}: ssq worst relative error {float(rel.max()):.3e} (bound {RS.SSQ_REL:.3e})')
    assert torch.isfinite(got).all() and bool(((got - want).abs() <= RS.SSQ_REL * want).all()), (name, float(rel.max()))


@pytest.mark.parametrize('M', RS.PRODUCER_MS)
@pytest.mark.parametrize('case', RS.PRODUCER_CASES, ids=[c[0] for c in RS.PRODUCER_CASES])
def test_chain_producer(ops, env, case, M):
    name, N, K, fp8, xkind = case
    dev = ops.dev
    wt = weights(env, ops, N, K, fp8, False)
    seed = zlib.crc32(name.encode()) + M
    g = torch.Generator(device=dev).manual_seed(seed)
    X = SI.outlier_x(M, K, seed=seed, device=dev)[0] if xkind == 'outlier' else (0.7 * torch.randn(M, K, generator=g, device=dev)).to(BF)
    h0 = (3 * torch.randn(M, N, generator=g, device=dev)).to(BF)
    hbuf, h, sbuf, ssq = run_producer(ops, X, wt, h0, M, N, K)
    what = f'producer {name} M {M}'
    check_producer_footprint(what, hbuf, h, sbuf, ssq, M, N)
    Xd = X.double()
    ref, tol = SI.epilogue_bound('resid', Xd @ wt['Wd'].T, SI.acc_floor(Xd, wt['Wd'], C_ACC), h0)
    check(what, h, ref, tol)
    _, h2, _, ssq2 = run_producer(ops, X, wt, h0, M, N, K)
    assert same_bits(h2, h) and same_bits(ssq2[:, :N // 16], ssq[:, :N // 16]), what


@pytest.mark.parametrize('M', RS.PRODUCER_MS)
def test_chain_producer_rounds_twice(ops, M):
    """Integer operands (|x| <= 8, |w| <= 2, K = 2048): every partial sum is an integer below 2^24, so the fp32 dot product is exact in any order and h must equal
    rnd(rnd(gemm) + h) bit for bit.  Most |gemm| exceed 256 -- beyond bf16's 8 bits -- so the first rounding changes the result: a single rounding rnd(gemm + h) gives other bits."""
    dev = ops.dev
    N, K = 64, 2048
    g = torch.Generator(device=dev).manual_seed(M)
    X = torch.randint(-8, 9, (M, K), generator=g, device=dev).to(BF)
    W = torch.randint(-2, 3, (N, K), generator=g, device=dev).to(BF)
    h0 = (3 * torch.randn(M, N, generator=g, device=dev)).to(BF)
    lin = (X.double() @ W.double().T)
    assert float(lin.abs().max()) < 2 ** 24
    want = RS.slab_resid(lin.float()[None], h0)
    once = (lin + h0.double()).to(BF)
    assert int((bits(once) != bits(want)).sum()) > 0          # the inputs tell the two apart
    hbuf, h, sbuf, ssq = run_producer(ops, X, dict(W=W, q8=None, sc=None), h0, M, N, K)
    diff = int((bits(h) != bits(want)).sum())
    assert diff == 0, f'{diff} of {h.numel()} elements differ from rnd(rnd(gemm) + h) ({int((bits(h) != bits(once)).sum())} from rnd(gemm + h))'
    check_producer_footprint(f'producer exact M {M}', hbuf, h, sbuf, ssq, M, N)


# ---- chain consumer ----------------------------------------------------------------------------------------------------------------------------------------
def run_consumer(ops, wt, h, gamma, ssq, X, M, N, K, epi, room):
    """-> (buffer, view, rows the kernel may write) after one consumer launch into a fresh guarded buffer: fp32 slabs [room * M, N] or the SwiGLU product [M, N / 2]"""
    if epi == 'none':
        buf, Y = guarded(room * M, N, torch.float32, ops.dev, after=16)
    else:
        buf, Y = guarded(M, N // 2, BF, ops.dev, after=16)
    rc, n = ops.gemv_chain(1, X, wt['W'], h, ssq, M, N, K, gamma=gamma, eps=EPS, Y=Y, q8=wt['q8'], scale=wt['sc'], epi=epi, max_splits=room)
    assert rc == 0, (rc, M, N, K, epi)
    return buf, Y, n


@pytest.mark.parametrize('M', RS.CONSUMER_MS)
@pytest.mark.parametrize('case', list(RS.CONSUMER_CASES), ids=[c[0] for c in RS.CONSUMER_CASES])
def test_chain_consumer(ops, env, case, M):
    name, epi, N, K, fp8, room = case
    splits, kw, rag = RS.CONSUMER_CASES[case]
    dev = ops.dev
    wt = weights(env, ops, N, K, fp8, epi == 'swiglu')
    h, gamma = RS.chain_h(M, K, seed=zlib.crc32(name.encode()) + M, device=dev)
    X = sentinel((M, K), BF, dev)                                   # l_xn as the step passes it: a chain consumer never reads it (NaN: one read shows)
    q = RS.tile_ssq(h)
    ssq_a = torch.zeros(M, RS.SSQ_STRIDE, device=dev); ssq_a[:, :K // 16] = q          # what a producer leaves: the tiles of h, zeros behind them
    ssq_b = (q.sum(-1) / RS.SSQ_STRIDE)[:, None].expand(M, RS.SSQ_STRIDE).contiguous()          # the same row totals over all 256 entries (224 .. 255 carry an eighth)
    # float64 reference on xn_ref = rnd(gamma * rnd(h * inv)), inv in float64.  Where h * inv lies within 2^-20 of a rounding tie (rms_ties) the kernel's fp32 inv may round to
    # the other neighbour, and its x differs from xn_ref there: those k add 2^-8 |w_nk xn_ref_k| to the uncertainty of the linear result, per output element (added to the
    # accumulation floor, so that the SwiGLU bound carries it through the activation; for fp32 slabs the bound IS that floor).
    ref_img, _ = RS.rms_image(h, gamma, EPS)
    xn_ref = ref_img.to(BF).double()
    ties = RS.rms_ties(h, gamma, EPS)
    Wd = wt['Wd']
    Wabs = Wd.abs()
    a = SI.acc_floor(xn_ref, Wd, C_ACC) + SI.U_BF16 * ((xn_ref.abs() * ties) @ Wabs.T)
    del Wabs
    ref, tol = SI.epilogue_bound(epi, xn_ref @ Wd.T, a, r=0 if epi == 'none' else 1)
    first = None
    for tag, ssq in (('tiles', ssq_a), ('spread', ssq_b), ('tiles again', ssq_a)):
        what = f'consumer {name} M {M} ssq {tag}'
        buf, Y, n = run_consumer(ops, wt, h, gamma, ssq, X, M, N, K, epi, room)
        plan = ops.last_plan()
        tiles = N // 16
        assert plan == (T.GEMV16, tiles, splits, (tiles // 2 if epi == 'swiglu' else tiles) * splits), (what, plan)
        assert (RS.wave_k(K, plan[2], fp8), RS.ragged(K, plan[2], fp8)) == (kw, rag), what
        rows = M if epi == 'swiglu' else n * M
        assert n == (0 if epi == 'swiglu' else splits), (what, n)
        assert guards_intact(buf, Y.shape[0]) and sentinel_intact(Y[rows:]), f'{what}: rows behind the output changed'
        out = Y if epi == 'swiglu' else Y[:rows].view(n, M, N).double().sum(0)
        check(what, out, ref, tol)
        if first is None:
            first = Y[:rows].clone()
        elif tag == 'tiles again':
            assert same_bits(Y[:rows], first), what


# ---- refusals: nothing is launched ---------------------------------------------------------------------------------------------------------------------------
def chain_operands(dev, role, M, N, K, room):
    W = SI.weights(N, K, seed=N + K, device=dev)
    ssq_buf, ssq = guarded(M, RS.SSQ_STRIDE, torch.float32, dev, after=16)
    if role == 2:
        X = torch.zeros(M, K, dtype=BF, device=dev)
        hbuf, h = guarded(M, N, BF, dev, after=16)
        return dict(X=X, W=W, h=h, ssq=ssq, gamma=None, Y=None), [hbuf, ssq_buf]
    X = torch.zeros(M, K, dtype=BF, device=dev); h = torch.ones(M, K, dtype=BF, device=dev); gamma = torch.ones(K, dtype=BF, device=dev)
    ssq.fill_(1.0)
    ybuf, Y = guarded(max(room, 1) * M, N, torch.float32, dev, after=16)
    return dict(X=X, W=W, h=h, ssq=ssq, gamma=gamma, Y=Y), [ybuf]


@pytest.mark.parametrize('name', list(RS.CHAIN_REFUSED))
def test_chain_shapes_the_planner_refuses(ops, name):
    role, M, N, K, room = RS.CHAIN_REFUSED[name]
    o, watched = chain_operands(ops.dev, role, M, N, K, room)
    rc, _ = ops.gemv_chain(role, o['X'], o['W'], o['h'], o['ssq'], M, N, K, gamma=o['gamma'], eps=EPS, Y=o['Y'], max_splits=room)
    assert rc != 0
    assert all(sentinel_intact(b) for b in watched)


def test_chain_role_and_operands_that_disagree(ops, ops_f32):
    dev = ops.dev
    M, N, K = 2, 512, 3584
    p, pw = chain_operands(dev, 2, M, N, K, 0)
    c, cw = chain_operands(dev, 1, M, N, K, 2)

    def call(o_, role, d, **kw):
        a = dict(gamma=d['gamma'], eps=EPS, Y=d['Y'], max_splits=2 if role == 1 else 0); a.update(kw)
        return o_.gemv_chain(role, d['X'], d['W'], d['h'], d['ssq'], M, N, K, **a)[0]
    assert call(ops, 3, c) != 0 and call(ops, 0, p) != 0                                   # no such role
    assert call(ops, 2, c) != 0                                                            # a producer with a consumer's gamma and output
    assert call(ops, 2, p, epi='swiglu') != 0                                              # ... with an epilogue
    assert call(ops, 1, p, max_splits=2) != 0                                              # a consumer without gamma / output
    assert call(ops, 1, c, gamma=None) != 0 and call(ops, 1, c, max_splits=0) != 0
    assert call(ops, 1, c, epi='resid') != 0
    assert call(ops, 1, c, q8=torch.zeros(N, K, dtype=torch.uint8, device=dev)) != 0       # fp8 bytes without their scales
    assert ops.gemv_chain(1, c['X'], c['W'], c['h'], c['ssq'], M, N + 8, K, gamma=c['gamma'], eps=EPS, Y=c['Y'], max_splits=2)[0] != 0          # N % 16
    assert ops.gemv_chain(1, c['X'], c['W'], c['h'], c['ssq'], M, N, K - 16, gamma=c['gamma'], eps=EPS, Y=c['Y'], max_splits=2)[0] != 0         # K % 32
    assert ops.gemv_chain(1, c['X'], c['W'], c['h'], c['ssq'], 17, N, K, gamma=c['gamma'], eps=EPS, Y=c['Y'], max_splits=2)[0] != 0             # M > 16
    assert ops.gemv_chain(1, c['X'], c['W'], c['h'], c['ssq'], M, 528, K, gamma=c['gamma'], eps=EPS, Y=c['Y'], epi='swiglu')[0] != 0            # SwiGLU with N % 32
    assert all(sentinel_intact(b) for b in pw + cw)
    # an fp32 context has no chain
    p, pw = chain_operands(ops_f32.dev, 2, M, N, K, 0)
    c, cw = chain_operands(ops_f32.dev, 1, M, N, K, 2)
    assert call(ops_f32, 2, p) != 0 and call(ops_f32, 1, c) != 0
    assert all(sentinel_intact(b) for b in pw + cw)
