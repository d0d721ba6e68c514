"""Every row of the GEMM regime table (tests/gemm_regimes.py) on the device, through the C ABI:

  * plan -- mmd_op_gemm_last_plan reports the row's (kernel, tiles, splits, blocks): the intended kernel and instantiation really ran;
  * parity -- element by element against a float64 reference computed on the device from the same bf16 operands (fp8 rows: the weights
    dequantised with quantize_ref), with the kernels' bf16 rounding points emulated; the max-norm bounds of the older tests are kept too;
  * out-of-range writes -- Y sits inside a buffer with guard rows before it and 256 rows after it, all holding a sentinel NaN; after the call
    every guard still holds it (slab rows: guards around the slab buffer, and the slabs past `*splits_out` untouched);
  * determinism -- a second identical call gives identical bits (and the same plan).

Element bound.  With u = 2^-24 and ulp(v) the bf16 spacing at |v| (2^(e-8) for |v| in [2^(e-1), 2^e)):
  fl[m, n] = u sqrt(K) |x_m| |w_n|   -- the fp32 accumulation: K roundings, each at most u times a partial sum, and every partial sum at most
      sum_k |x_mk w_nk| <= |x_m| |w_n| (Cauchy-Schwarz).  Random-signed, K of them stay within sqrt(K) times one in all but astronomically rare
      cases; their real size is far smaller (the partial sums grow like sqrt(k), not like the bound), so fl is a floor, not an estimate.
  bias / out_f32:  |Y - ref| <= ulp(ref) + 2 fl        (one bf16 rounding: half an ulp of Y, at most one ulp of ref across a binade)
  resid:           ... + (1 + 2^-7) ulp(lin)            (rnd(acc) may land on the other neighbour than rnd(lin): one ulp of lin; the final rounding
                                                          then costs at most half an ulp of ref plus 2^-8 of that neighbour step -- a tight bound: 0.98 of it is reached)
  gelu:            ulp(ref) + 1.13 (ulp(lin) + 2 fl) + 2^-20 |ref| + 1e-6   (|gelu'| <= 1.13; the fast forms: 2e-7 absolute + a few fp32 ulps)
  swiglu:          ulp(ref) + |u| (1.1 (ulp(g) + 2 fl_g) + ulp(s)) + |s| (ulp(u) + 2 fl_u) + 2^-20 |ref|   (s = rnd(silu(rnd(g))), |silu'| <= 1.1)
  slabs:           |sum of the fp32 slabs - ref| <= 2 fl  (nothing is rounded to bf16)
Each term is at most a couple of bf16 ulps; a missing bias (0.1), a dropped 32-deep K step (~0.04 at these scales) or the neighbour
channel's fp8 scale (~10 % of the value) are each many ulps on most elements.

Inputs are built on the device with seeded generators; each width's weights (the lm_head: 1.1 GB in bf16) and their float64 image are built once
per module.  Each row prints its plan and its largest error as a fraction of the bound (pytest -s shows them)."""
import math, zlib
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
import gemm_regimes as T

U = 2.0 ** -24


class _Env:
    """One context per workspace class, and each width's operands built once"""
    def __init__(self):
        self.ctx, self.w = {}, {}

    def ops(self, mst):
        if mst not in self.ctx:
            from rawops import RawOps
            self.ctx[mst] = RawOps(torch.bfloat16, max_step_tokens=mst)
        return self.ctx[mst]

    def weights(self, width, w8):
        key = (width, w8)
        if key in self.w:
            return self.w[key]
        N, K, epi = T.WIDTHS[width]
        ops = self.ops(1024)
        g = torch.Generator(device=ops.dev).manual_seed(zlib.crc32(width.encode()))
        W = (torch.randn(N, K, generator=g, device=ops.dev) / math.sqrt(K)).to(torch.bfloat16)
        if epi == 'swiglu':          # gate / up rows interleaved in blocks of 16 (the layout mmd_finalize_weights builds)
            W = torch.stack([W[:N // 2].view(-1, 16, K), W[N // 2:].view(-1, 16, K)], 1).reshape(N, K).contiguous()
        if w8:
            from rawops import quantize_ref
            Wq, q8, sc = ops.quantize_fp8(W)
            q_ref, s_ref = quantize_ref(W.cpu())          # (on the host, as test_gpu_fp8 states the scheme: bit-exact there)
            assert torch.equal(sc.cpu(), s_ref), width
            Wd = (q_ref.double() * s_ref.double()[:, None]).to(ops.dev)
            ent = dict(W=Wq, q8=q8, sc=sc, Wd=Wd)
            del W
        else:
            ent = dict(W=W, Wd=W.double())
        ent['wn'] = ent['Wd'].norm(dim=1)
        self.w[key] = ent
        return ent


@pytest.fixture(scope='module')
def env():
    e = _Env()
    yield e
    e.w.clear(); e.ctx.clear()
    torch.cuda.empty_cache()


def ulp(v):
    """bf16 spacing at |v| (0 at 0: the floor terms cover it)"""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 8))


def _rnd(v):
    return v.to(torch.bfloat16).double()


def _swiglu_split(t, M):
    """[M, N] in the interleaved column order -> (gate [M, N/2], up [M, N/2])"""
    v = t.reshape(M, -1, 2, 16)
    return v[:, :, 0].reshape(M, -1), v[:, :, 1].reshape(M, -1)


def _reference(epi, lin, fl, M, b=None, R=None):
    """-> (ref, per-element tolerance, max-norm factor of the older tests) for the kernel's output"""
    if epi == 'swiglu':
        lg, lu = _swiglu_split(lin, M)
        flg, flu = _swiglu_split(fl, M)
        gg, uu = _rnd(lg), _rnd(lu)
        s = _rnd(F.silu(gg))
        ref = s * uu
        tol = ulp(ref) + uu.abs() * (1.1 * (ulp(lg) + 2 * flg) + ulp(s)) + s.abs() * (ulp(lu) + 2 * flu) + 2.0 ** -20 * ref.abs()
        return ref, tol, 2.0
    if b is not None:
        lin = lin + b.double()
    if epi == 'resid':
        ref = _rnd(lin) + R.double()
        return ref, ulp(ref) + (1 + 2.0 ** -7) * ulp(lin) + 2 * fl, 2.0
    if epi in ('gelu_tanh', 'gelu_erf'):
        ref = F.gelu(_rnd(lin), approximate='tanh' if epi == 'gelu_tanh' else 'none')
        return ref, ulp(ref) + 1.13 * (ulp(lin) + 2 * fl) + 2.0 ** -20 * ref.abs() + 1e-6, 2.0
    return lin, ulp(lin) + 2 * fl, 1.0          # bias / out_f32


def _check_elements(name, Y, ref, tol):
    d = (Y.double() - ref).abs()
    bad = ~(d <= tol)                         # (NaN fails)
    nbad = int(bad.sum())
    if nbad:
        i = int(torch.argmax(torch.where(bad, d / tol.clamp_min(1e-30), torch.zeros_like(d))))
        m, n = divmod(i, ref.shape[1])
        pytest.fail(f'{name}: {nbad} of {ref.numel()} elements outside the bound; worst at ({m}, {n}): Y {float(Y[m, n])} ref {float(ref[m, n])} '
                    f'tol {float(tol[m, n]):.3e}')
    return float((d / tol.clamp_min(1e-30)).max())


@pytest.mark.parametrize('row', T.ROWS, ids=[r.name for r in T.ROWS])
def test_gemm_regime(env, row):
    N, K, epi = T.shape(row)
    M = row.M
    ops = env.ops(row.max_step_tokens)
    dev = ops.dev
    wt = env.weights(row.width, row.mode == 'w8')
    W = wt['W']
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(row.name.encode()))
    X = (torch.randn(M, K, generator=g, device=dev) * 0.7).to(torch.bfloat16)
    b = (0.1 * torch.randn(N, generator=g, device=dev)).to(torch.bfloat16) if epi in ('bias', 'gelu_tanh', 'gelu_erf') else None
    NO = N // 2 if epi == 'swiglu' else N
    R = torch.randn(M, NO, generator=g, device=dev).to(torch.bfloat16) if epi == 'resid' else None
    lin = X.double() @ wt['Wd'].T
    fl = U * math.sqrt(K) * X.double().norm(dim=1)[:, None] * wt['wn'][None, :]
    from rawops import guarded, sentinel_intact

    if row.mode == 'slabs':
        S, G = T.SLAB_MAX_SPLITS, 16 * N
        outs = []
        for _ in range(2):
            buf = torch.empty(G + S * M * N + G, dtype=torch.float32, device=dev)
            buf.view(torch.int32).fill_(0x7FA5A5A5)
            n = ops.gemm_slabs_into(buf[G:], X, W, S)
            plan = ops.last_plan()
            assert plan == row.plan, (row.name, 'plan', plan, row.plan)
            assert n == row.plan[2], (row.name, n)
            assert sentinel_intact(buf[:G]) and sentinel_intact(buf[G + S * M * N:]), (row.name, 'write outside the slab buffer')
            assert sentinel_intact(buf[G + n * M * N:G + S * M * N]), (row.name, f'slabs past the {n} reported were written')
            outs.append(buf[G:G + n * M * N].clone())
            del buf
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), (row.name, 'second call differs')
        Y = outs[0].view(n, M, N).double().sum(0)
        ref = lin
        worst = _check_elements(row.name, Y, ref, 2 * fl)
        err = (Y - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        assert err <= 2e-5 * max(1.0, math.sqrt(K / 3584)), (row.name, err)          # test_stream_gemm_slabs_equal_fp32_math's bound
    else:
        out_f32 = epi == 'out_f32'
        kepi = {'bias': 'none', 'out_f32': 'none'}.get(epi, epi)
        ydt = torch.float32 if out_f32 else torch.bfloat16
        outs = []
        for _ in range(2):
            buf, Y = guarded(M, NO, ydt, dev)
            if row.mode == 'w8':
                ops.gemm_w8_into(Y, X, W, wt['q8'], wt['sc'], b, R, kepi)
            else:
                ops.gemm_into(Y, X, W, b, R, kepi, out_f32)
            plan = ops.last_plan()
            assert plan == row.plan, (row.name, 'plan', plan, row.plan)
            assert sentinel_intact(buf[:16]) and sentinel_intact(buf[16 + M:]), (row.name, 'write outside Y')
            outs.append(Y.clone())
            del buf, Y
        Y = outs[0]
        assert torch.equal(Y.view(torch.int16 if ydt == torch.bfloat16 else torch.int32), outs[1].view(torch.int16 if ydt == torch.bfloat16 else torch.int32)), \
            (row.name, 'second call differs')
        if out_f32:
            assert torch.equal(Y, Y.to(torch.bfloat16).float()), (row.name, 'fp32 output not rounded through bf16')
        ref, tol, scale = _reference(epi, lin, fl, M, b, R)
        worst = _check_elements(row.name, Y, ref, tol)
        err = (Y.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        assert torch.isfinite(Y).all() and err <= 1.2e-2 * scale, (row.name, err)        # the max-norm bound of test_gpu_production / test_gpu_fp8
    print(f'{row.name}: plan {plan}, worst |Y - ref| / bound {worst:.3f}, max-norm error {err:.2e}')
