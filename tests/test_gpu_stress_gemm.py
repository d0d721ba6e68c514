"""GEMM regimes, epilogues and norms on the inputs real checkpoints produce (tests/stress_inputs.py): six activation channels at 10^3 .. 10^4 among K - 6
of size 0.7, pre-activations far into the saturation of SiLU / GELU, norm rows that carry one element at 1e4.

Why an element-wise bound.  The older GEMM tests measure max|err| / max(1, max|ref|).  With outlier channels max|ref| is ~900 while the median |ref| is
~170 and a correct bf16 result is within ~0.7 of it: 2.4e-2 relative allows 21 absolute on EVERY element, and a kernel that dropped the whole non-outlier
part of the sum would pass (tests/test_stress_inputs.py shows exactly that on the host).  Here every element is held to

    |Y - ref| <= 2^-8 sum_p (|p| + a) + a,      a = C_ACC sqrt(K) 2^-24 (|X| |W|^T)

against the float64 product of the bf16 operands.  2^-8 is bf16's relative rounding error; p runs over the exact images of the values the kernel rounds to
bf16 on its way to Y: the result alone for none / bias / out_f32 (r = 1), the linear result and then the sum for `resid` (r = 2; where |lin| ~ |ref| this is
2 2^-8 (|ref| + a) + a, and it stays sound where the residual cancels the linear part), none for the fp32 dtype and for fp32 slabs (r = 0).  For GELU and
SwiGLU the pre-activation's budget e = 2^-8 (|lin| + a) + a goes through the activation's Lipschitz factor (1.13 GELU, 1.1 SiLU), the rounding of s =
silu(gate) and of the product follow, and the fast forms get the 2^-20 |ref| + 1e-6 of tests/test_gpu_gemm_regimes.py.  sqrt(K) 2^-24 A is the standard
probabilistic bound of an fp32 summation.

C_ACC = 3.04 is defined in tests/stress_inputs.py, next to the measurements it comes from; test_c_acc_is_four_times_the_measured_fp32_error prints the device's.
No kernel bug was found by these cases.

Not here: the tower's fp16 GEMM epilogues past 65504.  mmd_op_gemm runs in the context dtype only (the fp16 GEMMs are set inside the tower's own forward);
tests/test_gpu_tower_stress.py reaches them through the tower itself (half_range: an fc2 output at 45 056, half_overflow: past 65 520, where fp16 is inf)."""
import math, zlib
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
import gemm_regimes as T
import stress_inputs as SI
import residual_stream as RS

C_ACC = SI.C_ACC
U = SI.U_BF16


@pytest.fixture(scope='module')
def env():
    e = {}
    yield e
    e.clear()
    torch.cuda.empty_cache()


def _ops(env, dtype=torch.bfloat16, mst=1024):
    if (dtype, mst) not in env:
        from rawops import RawOps
        env[(dtype, mst)] = RawOps(dtype, max_step_tokens=mst)
    return env[(dtype, mst)]


_split, _bound = SI.swiglu_split, SI.epilogue_bound          # (shared with tests/test_gpu_residual_stream.py)


def _check(name, Y, ref, tol):
    assert torch.isfinite(Y.float()).all(), (name, 'not finite')
    d = (Y.double() - ref).abs()
    bad = ~(d <= tol)
    if int(bad.sum()):
        i = int(torch.argmax(torch.where(bad, d / tol.clamp_min(1e-30), torch.zeros_like(d))))
        m, n = divmod(i, ref.shape[1])
        pytest.fail(f'{name}: {int(bad.sum())} of {ref.numel()} elements outside the bound; worst at ({m}, {n}): Y {float(Y[m, n])} ref {float(ref[m, n])} tol {float(tol[m, n]):.3e}')
    worst = float((d / tol.clamp_min(1e-30)).max())
    print(f'{name}: worst |Y - ref| / bound {worst:.3f}, median bound {float(tol.median()):.3e}, max|ref| {float(ref.abs().max()):.1f}')
    return worst


@pytest.mark.parametrize('M,N,K', [(49, 512, 3584), (49, 256, 18944), (130, 384, 1152), (1274, 512, 3584)])
def test_c_acc_is_four_times_the_measured_fp32_error(env, M, N, K):
    """Prints the device library's fp32 matmul error in units of sqrt(K) 2^-24 A (what C_ACC was chosen from) and holds it to C_ACC itself: a library whose fp32
    product left the bound would make the bound's premise false, a heuristic change inside the library does not fail this suite."""
    dev = _ops(env).dev
    X, _ = SI.outlier_x(M, K, seed=M + K, device=dev); W = SI.weights(N, K, seed=N, device=dev)
    ref = X.double() @ W.double().T
    a1 = SI.acc_floor(X.double(), W.double(), 1.0)
    ratio = (((X.float() @ W.float().T).double() - ref).abs() / a1).max().item()
    print(f'c_acc {M}x{N}x{K}: device torch fp32 matmul error / (sqrt(K) 2^-24 A) = {ratio:.3f}')
    assert ratio <= C_ACC


# ---- one outlier_x case per dispatch regime ---------------------------------------------------------------------------------------------------------------
REGIME_ROWS = ['gemm_qkv_16', 'gemm_gate_up_2', 'gemm_down_17', 'gemm_lm_head_33', 'gemm_qkv_64', 'gemm_down_129', 'gemm_gate_up_128', 'gemm_lm_head_65', 'gemm_lm_head_256',
               'gemm_o_257', 'gemm_gate_up_257', 'gemm_down_257', 'gemm_gate_up_513', 'gemm_down_512', 'gemm_qkv_1281', 'gemm_fc1_257', 'gemm_proj0_129', 'gemm_fc2_33',
               'w8_qkv_16', 'w8_down_33', 'w8_gate_up_64', 'w8_o_128', 'w8_o_257', 'w8_gate_up_257', 'w8_down_512', 'w8_gate_up_513', 'w8_qkv_1281',
               'slabs_qkv_16', 'slabs_down_32', 'slabs_o_64', 'slabs_down_256']


def test_every_kernel_of_the_regime_table_has_a_stress_row():
    rows = T.rows_by_name()
    for mode in ('gemm', 'w8', 'slabs'):
        assert {r.plan[0] for r in T.ROWS if r.mode == mode} == {rows[n].plan[0] for n in REGIME_ROWS if rows[n].mode == mode}, mode


def _weights(env, width, w8):
    key = ('w', width, w8)
    if key not in env:
        N, K, epi = T.WIDTHS[width]
        ops = _ops(env)
        W = SI.weights(N, K, seed=zlib.crc32(width.encode()), device=ops.dev)
        if w8:
            W[5, K // 3] = W[5].abs().max() * 100          # one row's scale is set by a single 100 x outlier column
        if epi == 'swiglu':
            W = SI.swiglu_interleave(W)
        if w8:
            from rawops import quantize_ref
            Wq, q8, sc = ops.quantize_fp8(W)
            q_ref, s_ref = quantize_ref(W.cpu())
            assert torch.equal(sc.cpu(), s_ref), width
            env[key] = dict(W=Wq, q8=q8, sc=sc, Wd=(q_ref.double() * s_ref.double()[:, None]).to(ops.dev))
        else:
            env[key] = dict(W=W, Wd=W.double())
    return env[key]


@pytest.mark.parametrize('name', REGIME_ROWS)
def test_gemm_regime_with_outlier_channels(env, name):
    row = T.rows_by_name()[name]
    N, K, epi = T.shape(row)
    M = row.M
    ops = _ops(env, mst=row.max_step_tokens)
    dev = ops.dev
    wt = _weights(env, row.width, row.mode == 'w8')
    X, _ = SI.outlier_x(M, K, seed=zlib.crc32(name.encode()), device=dev)
    g = torch.Generator(device=dev).manual_seed(M + N)
    b = (0.1 * torch.randn(N, generator=g, device=dev)).to(torch.bfloat16) if epi in ('bias', 'gelu_tanh', 'gelu_erf') else None
    NO = N // 2 if epi == 'swiglu' else N
    R = torch.randn(M, NO, generator=g, device=dev).to(torch.bfloat16) if epi == 'resid' else None
    lin = X.double() @ wt['Wd'].T
    a = SI.acc_floor(X.double(), wt['Wd'], C_ACC)
    if row.mode == 'slabs':
        slabs = torch.zeros(T.SLAB_MAX_SPLITS * M * N, dtype=torch.float32, device=dev)
        n = ops.gemm_slabs_into(slabs, X, wt['W'], T.SLAB_MAX_SPLITS)
        assert ops.last_plan() == row.plan and n == row.plan[2], (name, ops.last_plan(), n)
        _check(name, slabs[:n * M * N].view(n, M, N).double().sum(0), lin, a)
        return
    if b is not None:
        lin = lin + b.double()
    out_f32 = epi == 'out_f32'
    kepi = {'bias': 'none', 'out_f32': 'none'}.get(epi, epi)
    Y = torch.empty(M, NO, dtype=torch.float32 if out_f32 else torch.bfloat16, device=dev)
    if row.mode == 'w8':
        ops.gemm_w8_into(Y, X, wt['W'], wt['q8'], wt['sc'], b, R, kepi)
    else:
        ops.gemm_into(Y, X, wt['W'], b, R, kepi, out_f32)
    assert ops.last_plan() == row.plan, (name, ops.last_plan(), row.plan)
    ref, tol = _bound(kepi, lin, a, R)
    _check(name, Y, ref, tol)


# ---- the production shapes where the outliers travel the furthest ------------------------------------------------------------------------------------------
PROD = [('qkv_frame', 49, 4608, 3584, 'none', (T.STREAM,), 1), ('down_frame', 49, 3584, 18944, 'resid', (T.STREAM,), 2), ('down_chunk', 1274, 3584, 18944, 'resid', (T.RING256, T.RING128X2), 2),
        ('gate_up_chunk', 1274, 37888, 3584, 'swiglu', (T.RING256, T.RING128X2), 1), ('fc1_tower', 25515, 4352, 1152, 'gelu_tanh', (T.RING256, T.RING128X2), 1)]


@pytest.mark.parametrize('name,M,N,K,epi,kernels,min_splits', PROD, ids=[p[0] for p in PROD])
def test_production_gemm_shapes_with_outlier_channels(env, name, M, N, K, epi, kernels, min_splits):
    ops = _ops(env)
    dev = ops.dev
    X, _ = SI.outlier_x(M, K, seed=M + N, device=dev)
    W = SI.weights(N, K, seed=N + K, device=dev)
    if epi == 'swiglu':
        W = SI.swiglu_interleave(W)
    g = torch.Generator(device=dev).manual_seed(M)
    b = (0.1 * torch.randn(N, generator=g, device=dev)).to(torch.bfloat16) if epi in ('none', 'gelu_tanh') else None
    R = torch.randn(M, N, generator=g, device=dev).to(torch.bfloat16) if epi == 'resid' else None
    Y = torch.empty(M, N // 2 if epi == 'swiglu' else N, dtype=torch.bfloat16, device=dev)
    ops.gemm_into(Y, X, W, b, R, epi)
    plan = ops.last_plan()
    assert plan[0] in kernels and plan[2] >= min_splits, (name, plan)
    Xd, Wd = X.double(), W.double()
    lin = Xd @ Wd.T
    if b is not None:
        lin += b.double()
    a = SI.acc_floor(Xd, Wd, C_ACC)
    del Xd, Wd
    ref, tol = _bound(epi, lin, a, R)
    _check(f'{name} plan {plan}', Y, ref, tol)


# ---- epilogue saturation --------------------------------------------------------------------------------------------------------------------------------------
SAT = [('swiglu', 50.0), ('swiglu', 120.0), ('gelu_tanh', 8.0), ('gelu_tanh', 40.0), ('gelu_erf', 8.0), ('gelu_erf', 40.0)]
SAT_FORMS = ([(v, dt, 70, 192, 136) for v in (1, 2, 3) for dt in (torch.float32, torch.bfloat16)] +
             [(v, torch.bfloat16, 300, 320, 192) for v in (4, 6, 7, 32, 33, 36, 37)] + [(8, torch.bfloat16, 130, 320, 256)])
SAT_KERNELS = {1: (T.TILE64,), 2: (T.TILE64,), 3: (T.TILE128,), 4: (T.BIG64, T.BIG128), 6: (T.RING256,), 7: (T.RING256,), 32: (T.RING256,), 33: (T.RING128X2,), 36: (T.RING256,), 37: (T.RING128X2,), 8: (T.STREAM,)}


@pytest.mark.parametrize('epi,amp', SAT, ids=[f'{e}_{int(a)}' for e, a in SAT])
@pytest.mark.parametrize('variant,dtype,M,N,K', SAT_FORMS, ids=[f'v{f[0]}_{"f32" if f[1] == torch.float32 else "bf16"}' for f in SAT_FORMS])
def test_epilogues_far_into_saturation(env, variant, dtype, M, N, K, epi, amp):
    """|gate| to 50 and 120 (exp2 overflows to inf past 88.7 / log2 e: the result must be -0 or gate x up, never NaN), GELU arguments to 8 and 40.  Besides the
    bound: where the (gate) pre-activation is <= -41 the output is +-0 or vanishing (|Y| <= 1e-12 max(1, |up|)), never NaN, never a large value."""
    ops = _ops(env, dtype)
    X, W = SI.saturating(M, K, N, amp, seed=int(amp) + variant, device=ops.dev)
    if epi == 'swiglu':
        W = SI.swiglu_interleave(W)
    Y = ops.gemm(X, W, None, epi=epi, variant=variant)
    assert ops.last_plan()[0] in SAT_KERNELS[variant], (variant, ops.last_plan())
    Xd, Wd = X.double(), W.double()
    lin = Xd @ Wd.T
    ref, tol = _bound(epi, lin, SI.acc_floor(Xd, Wd, C_ACC), r=0 if dtype == torch.float32 else 1)
    pre, up = _split(lin) if epi == 'swiglu' else (lin, torch.ones_like(lin))
    assert pre.min().item() <= -amp and pre.max().item() >= amp
    _check(f'{epi} amp {amp} v{variant} {dtype}', Y, ref, tol)
    dead = pre <= -41.0
    if amp >= 40:
        assert int(dead.sum()) > 0
        assert bool((Y.double()[dead].abs() <= 1e-12 * up[dead].abs().clamp_min(1.0)).all()), Y.double()[dead].abs().max().item()


# ---- norms ------------------------------------------------------------------------------------------------------------------------------------------------------
def _norm_rows(H, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(6, H, generator=g, device=dev) * 3
    for r in range(4):
        x[r, (r * 977 + 5) % H] = 1e4 * (-1) ** r          # one element at 1e4
    x[4] = 1e4                                              # a whole row at 1e4
    x[5] = 0                                                # an all-zero row: eps decides
    w = 1 + 0.1 * torch.randn(H, generator=g, device=dev); b = 0.1 * torch.randn(H, generator=g, device=dev)
    return x.to(torch.bfloat16), w.to(torch.bfloat16), b.to(torch.bfloat16)


@pytest.mark.parametrize('H', [3584, 1152, 72])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_norms_with_an_element_at_1e4(env, dtype, H):
    """rmsnorm / layernorm against float64 on the rounded inputs, element-wise 2^-8 |ref| + 2^-20 max|w| (bf16) and 1e-5 (|ref| + max|w|) (fp32).  RMSNorm rounds the normalised
    value to the model dtype BEFORE the gain (as Qwen2RMSNorm does): the reference rounds there too, and where the float64 value sits within 2^-20 of a rounding tie either
    neighbour is right."""
    ops = _ops(env, dtype)
    x, w, b = _norm_rows(H, ops.dev, H)
    xd, wd, bd = x.double(), w.double(), b.double()
    bf = dtype == torch.bfloat16
    floor = (2.0 ** -20 if bf else 1e-5) * wd.abs().max().item()
    rel = U if bf else 1e-5
    # RMSNorm
    y = ops.rmsnorm(x, w, 1e-6).double()
    err = RS.rms_excess(y, RS.rms_candidates(x, w, 1e-6, rounded=bf), rel, floor)          # (the rule lives in tests/residual_stream.py: the slab and chain tests apply it too)
    assert torch.isfinite(y).all() and err.max().item() <= 0, ('rmsnorm', H, err.max().item())
    assert bool((y[5] == 0).all())
    # LayerNorm
    y = ops.layernorm(x, w, b, 1e-6).double()
    mu = xd.mean(-1, keepdim=True); var = (xd - mu).pow(2).mean(-1, keepdim=True)
    ref = (xd - mu) * torch.rsqrt(var + 1e-6) * wd + bd
    err = (y - ref).abs() - (rel * ref.abs() + floor)
    assert torch.isfinite(y).all() and err.max().item() <= 0, ('layernorm', H, err.max().item(), int(err.argmax()) // H)
    tb = rel * bd.abs() + floor          # a constant row and the zero row are the bias: eps decides
    assert bool(((y[4] - bd).abs() <= tb).all()) and bool(((y[5] - bd).abs() <= tb).all())


def test_resid32_layernorm_near_the_fp16_maximum(env):
    """y16 at +-60000 added to an fp32 stream at 1e4: the fp32 stream and the bf16 image bit-exact, LayerNorm to fp16 rounding; and with a gain of 5e4 the LayerNorm result
    passes 65504: the fp16 output is inf exactly where torch's .half() of the float64 result is."""
    from rawops import _ptr
    from mmduet_amd._lib import lib, check
    ops = _ops(env)
    dev = ops.dev
    M, H = 37, 1152
    g = torch.Generator(device=dev).manual_seed(9)
    y = (60000.0 * torch.sign(torch.randn(M, H, generator=g, device=dev)) * (1 - 0.05 * torch.rand(M, H, generator=g, device=dev))).to(torch.float16)
    h = torch.randn(M, H, generator=g, device=dev) * 1e4
    b = (0.1 * torch.randn(H, generator=g, device=dev)).to(torch.float16)
    ref_h = h + y.float()
    ops.m._bind_stream()
    for gain, overflow in ((1.0, False), (5e4, True)):
        w = (gain * (1 + 0.05 * torch.randn(H, generator=g, device=dev))).to(torch.float16)
        h1, y1 = h.clone(), y.clone()
        check(lib().mmd_op_resid32_layernorm(ops.ctx, _ptr(y1), _ptr(h1), None, 0, _ptr(w), _ptr(b), _ptr(y1), None, M, H, 1e-6), ops.ctx)
        torch.cuda.synchronize()
        assert torch.equal(h1, ref_h)
        ref_ln = F.layer_norm(ref_h.double(), (H,), w.double(), b.double(), 1e-6)
        want = ref_ln.to(torch.float16)
        assert bool(torch.isinf(want).any()) == overflow
        assert torch.equal(torch.isinf(y1), torch.isinf(want)) and not torch.isnan(y1).any()
        fin = ~torch.isinf(want)
        assert bool(((y1.double() - ref_ln).abs()[fin] <= 2.0 ** -10 * ref_ln.abs()[fin].clamp_min(gain)).all())
        assert bool((torch.sign(y1[~fin].float()) == torch.sign(ref_ln[~fin].float())).all())
    h2 = h.clone(); out = torch.empty(M, H, dtype=torch.bfloat16, device=dev)
    check(lib().mmd_op_resid32_layernorm(ops.ctx, _ptr(y), _ptr(h2), None, 0, None, None, None, _ptr(out), M, H, 1e-6), ops.ctx)
    torch.cuda.synchronize()
    assert torch.equal(out, ref_h.to(torch.bfloat16)) and torch.equal(h2, h)
