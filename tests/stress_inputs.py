"""Stress inputs for the parity tests: the structure real checkpoints have and `randn` data does not -- an attention sink, one-hot softmax rows, a running
max that keeps rising, a few residual channels at 10^3 .. 10^4, MLP pre-activations far into saturation.  Plain torch, seeded, bf16-rounded; imports and
runs without a GPU (tests/test_stress_inputs.py checks on the host that every builder has the property its name claims).

Attention builders return (q [S, nh * d], K [nkv, cap, d], V [nkv, cap, d], n_ctx, hot) in the layouts RawOps.attention takes, K / V poisoned with 1e4
past n_ctx + S as in the benign tests (with q at 200 .. 1000 a poisoned key scores ~10^8: it must still never reach the result).  `hot` is the key that
owns every row's softmax (None where no single key does).  With c = d ** -0.5 and "score" the scaled score q.k c:

  sink            q[.., j] = 200; K[.., j] *= 0.02; K[0, j] = 60 / (200 c): key 0 scores +60, all others O(1)
  rising          q[.., j] = 200; K[t, j] = (t / n) 400 / (200 c): the running max rises on every key tile
  last_hot        as sink, hot key at n_ctx - 1 (non-causal: n_tot - 1; n_ctx = 0: key 0), +150
  huge            q *= 30; K *= 30: scores of magnitude 3000 .. 4500
  outlier_dims    three q channels at 300, -700, 1000 (x (1 + 0.05 randn)), the same K channels at 0.3 randn
  first_row_only  sink with n_ctx = 0: row 0 sees exactly one key

GEMM builders: outlier_x (six channels of X at 10^3 .. 10^4), weights (randn / sqrt(K)), saturating (pre-activations of standard deviation amp / 3), and
the element-wise bound the stress GEMM tests use (acc_floor / rounding_tol / epilogue_bound)."""
import math
from collections import namedtuple
import torch
import torch.nn.functional as F

AttnCase = namedtuple('AttnCase', 'q K V n_ctx hot')
BF = torch.bfloat16


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def _base(S, nh, nkv, d, n_ctx, seed, device):
    g = _gen(seed, device)
    cap = (n_ctx + S + 100 + 63) // 64 * 64
    q = torch.randn(S, nh, d, generator=g, device=device)
    K = torch.randn(nkv, cap, d, generator=g, device=device)
    V = torch.randn(nkv, cap, d, generator=g, device=device)
    return g, q, K, V


def _finish(q, K, V, S, n_ctx, hot):
    n_tot = n_ctx + S
    K[:, n_tot:] = 1e4; V[:, n_tot:] = 1e4            # beyond the valid range: must never reach the result
    return AttnCase(q.reshape(S, -1).to(BF), K.to(BF), V.to(BF), n_ctx, hot)


def _one_hot(S, nh, nkv, d, n_ctx, j, seed, device, hot, lift):
    g, q, K, V = _base(S, nh, nkv, d, n_ctx, seed, device)
    c = d ** -0.5
    q[:, :, j] = 200.0
    K[:, :, j] *= 0.02
    K[:, hot, j] = lift / (200.0 * c)
    return _finish(q, K, V, S, n_ctx, hot)


def sink(S, nh, nkv, d, n_ctx, causal=True, j=None, seed=0, device='cpu'):
    return _one_hot(S, nh, nkv, d, n_ctx, d // 3 if j is None else j, seed, device, 0, 60.0)


def last_hot(S, nh, nkv, d, n_ctx, causal=True, j=None, seed=0, device='cpu'):
    hot = max(n_ctx - 1, 0) if causal else n_ctx + S - 1
    return _one_hot(S, nh, nkv, d, n_ctx, d // 3 if j is None else j, seed, device, hot, 150.0)


def first_row_only(S, nh, nkv, d, n_ctx, causal=True, j=None, seed=0, device='cpu'):
    return sink(S, nh, nkv, d, 0, causal, j, seed, device)


def rising(S, nh, nkv, d, n_ctx, causal=True, j=None, seed=0, device='cpu'):
    j = d // 3 if j is None else j
    g, q, K, V = _base(S, nh, nkv, d, n_ctx, seed, device)
    n = n_ctx + S
    q[:, :, j] = 200.0
    K[:, :n, j] = (torch.arange(n, device=device, dtype=torch.float32) / n) * (400.0 / (200.0 * d ** -0.5))
    return _finish(q, K, V, S, n_ctx, None)


def huge(S, nh, nkv, d, n_ctx, causal=True, j=None, seed=0, device='cpu'):
    g, q, K, V = _base(S, nh, nkv, d, n_ctx, seed, device)
    return _finish(q * 30.0, K * 30.0, V, S, n_ctx, None)


def outlier_channels(d, j=None):
    j = d // 3 if j is None else j
    return [j, (j + 7) % d, (j + d // 2) % d]


def outlier_dims(S, nh, nkv, d, n_ctx, causal=True, j=None, seed=0, device='cpu'):
    g, q, K, V = _base(S, nh, nkv, d, n_ctx, seed, device)
    for ch, amp in zip(outlier_channels(d, j), (300.0, -700.0, 1000.0)):
        q[:, :, ch] = amp * (1.0 + 0.05 * torch.randn(S, nh, generator=g, device=device))
        K[:, :, ch] = 0.3 * torch.randn(K.shape[0], K.shape[1], generator=g, device=device)
    return _finish(q, K, V, S, n_ctx, None)


ATTN_PATTERNS = {'sink': sink, 'rising': rising, 'last_hot': last_hot, 'huge': huge, 'outlier_dims': outlier_dims, 'first_row_only': first_row_only}


# ---- GEMM operands ----------------------------------------------------------------------------------------------------------------------------------
OUTLIER_AMPS = (1e3, -2e3, 4e3, -6e3, 8e3, 1e4)


def outlier_x(M, K, seed=0, device='cpu'):
    """-> (X [M, K] bf16: 0.7 randn with six random channels at OUTLIER_AMPS x (1 + 0.1 randn) per row, the six channel indices)"""
    g = _gen(seed, device)
    X = 0.7 * torch.randn(M, K, generator=g, device=device)
    ch = torch.randperm(K, generator=g, device=device)[:6]
    amps = torch.tensor(OUTLIER_AMPS, device=device)
    X[:, ch] = amps[None, :] * (1.0 + 0.1 * torch.randn(M, 6, generator=g, device=device))
    return X.to(BF), ch


def weights(N, K, seed=1, device='cpu'):
    return (torch.randn(N, K, generator=_gen(seed, device), device=device) / math.sqrt(K)).to(BF)


def saturating(M, K, N, amp, seed=0, device='cpu'):
    """-> (X [M, K], W [N, K]) bf16 whose product has standard deviation amp / 3, so that |pre-activation| reaches amp (and passes it on a few elements)"""
    g = _gen(seed, device)
    X = torch.randn(M, K, generator=g, device=device)
    W = torch.randn(N, K, generator=g, device=device) * (amp / 3.0 / math.sqrt(K))
    return X.to(BF), W.to(BF)


def swiglu_interleave(W):
    """[gate; up] rows -> blocks of 16 gate rows, 16 up rows, ... (the layout the SwiGLU epilogues read)"""
    N, K = W.shape
    return torch.stack([W[:N // 2].view(-1, 16, K), W[N // 2:].view(-1, 16, K)], 1).reshape(N, K).contiguous()


# ---- the element-wise GEMM bound ----------------------------------------------------------------------------------------------------------------------
U_BF16 = 2.0 ** -8          # bf16's relative rounding error (half an ulp)

# C_ACC of acc_floor.  Measured ratio max |fp32 matmul - float64| / (sqrt(K) 2^-24 |X| |W|^T) of torch's own fp32 matmul on the outlier_x operands: on the host
# 0.37 (49 x 512 x 3584), 0.07 (49 x 256 x 18944), 0.58 (130 x 384 x 1152), and 0.11 .. 0.76 over the three shapes the bound was first tried at; on an MI355X
# 0.48, 0.25, 0.51 at the same three shapes (tests/test_gpu_stress_gemm.py prints them; at 1274 x 512 x 3584 the device library measured 1.72 -- another of its
# kernels, a coarser summation -- and the constant was NOT raised for it).  C_ACC = 4 x the largest = 4 x 0.76; every GEMM kernel of this repository stays inside the
# bound with it (worst |Y - ref| / bound: 0.94 on the GELU epilogues, 0.76 SwiGLU).
LARGEST_MEASURED_ACC_RATIO = 0.76
C_ACC = 4 * LARGEST_MEASURED_ACC_RATIO


def acc_floor(Xd, Wd, c_acc):
    """a = c_acc sqrt(K) 2^-24 (|X| |W|^T): the probabilistic fp32 summation bound, per element.  Xd [M, K], Wd [N, K] in float64."""
    return c_acc * math.sqrt(Xd.shape[1]) * 2.0 ** -24 * (Xd.abs() @ Wd.abs().T)


def rounding_tol(points, a):
    """|Y - ref| <= 2^-8 sum_p (|p| + a) + a over the values p that the kernel rounds to bf16 on the way to Y (the exact images of them: the computed
    ones lie within a).  With one point (p = ref) this is r 2^-8 (|ref| + a) + a at r = 1; with none (fp32 output) it is a."""
    t = a.clone()
    for p in points:
        t = t + U_BF16 * (p.abs() + a)
    return t


def swiglu_split(t):
    """[M, N] in the interleaved SwiGLU column order -> (gate [M, N/2], up [M, N/2])"""
    v = t.reshape(t.shape[0], -1, 2, 16)
    return v[:, :, 0].reshape(t.shape[0], -1), v[:, :, 1].reshape(t.shape[0], -1)


def epilogue_bound(epi, lin, a, R=None, r=1):
    """-> (ref, tol) for a kernel output; lin = X W^T (+ bias) in float64, a = acc_floor, r = 1 bf16 output / 0 fp32"""
    u = U_BF16 * r
    act = 2.0 ** -20
    if epi == 'swiglu':
        g, up = swiglu_split(lin); ag, au = swiglu_split(a)
        eg = u * (g.abs() + ag) + ag; eu = u * (up.abs() + au) + au
        s = F.silu(g)
        es = 1.1 * eg + u * (s.abs() + 1.1 * eg) + act * s.abs() + 1e-6
        ref = s * up
        t = up.abs() * es + s.abs() * eu + es * eu
        return ref, t + u * (ref.abs() + t)
    if epi == 'resid':
        ref = lin + R.double()
        return ref, u * (lin.abs() + a) + u * (ref.abs() + a + u * lin.abs()) + a
    if epi in ('gelu_tanh', 'gelu_erf'):
        ref = F.gelu(lin, approximate='tanh' if epi == 'gelu_tanh' else 'none')
        e = u * (lin.abs() + a) + a
        return ref, 1.13 * e + u * (ref.abs() + 1.13 * e) + act * ref.abs() + 1e-6
    return lin, u * (lin.abs() + a) + a


def old_max_norm_err(Y, ref):
    """the measure of assert_close (tests/test_gpu_ops.py) and _rel_err (tests/test_gpu_production.py)"""
    return (Y.double() - ref.double()).abs().max().item() / max(1.0, ref.double().abs().max().item())
