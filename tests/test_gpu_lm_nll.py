"""mmd_op_lm_nll: per-row cross entropy of labels under X . W^T through the chunked lm_head path -- the [M, V] logits are never held; per row a running maximum,
a running sum of exponentials and the label's logit survive a vocabulary chunk (mmduet_amd/csrc/ops.hip, lm_nll_*; host loop lm_nll_run in model.hip).

Expectation: float64 F.cross_entropy(reduction='none') / torch.logsumexp on logits computed in fp32 by torch from the same operand bits.
Tolerance per row:
  rounding bound   1e-5 + 4 * 2^-23 * max |logit of the row|   (streaming fp32 log-sum-exp against float64)
  fp32 context     + 3e-4: F32_TOL of tests/test_gpu_model.py (GEMM accumulation order), doubled because lse and the label logit each move by at most the logit error
  bf16 context     + 2 x the largest difference between the product's own mmd_op_gemm fp32 logits and torch's, measured in the test (the library rounds a bf16
                   context's logits to bf16, as nn.Linear in bf16 does)
"""
import ctypes as C
import functools
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

K = 256
M_MAX = 300
FAMILIES = ('normal', 'sink', 'ramp', 'scaled')
INTERESTING = (255, 256, 335, 336, 8191, 8192, 55807, 55808)          # last column of a chunk and the first of the next, for the chunk widths of the cases below


@functools.lru_cache(maxsize=None)
def raw(dtype, max_step_tokens=512):
    from rawops import RawOps
    return RawOps(dtype, max_step_tokens=max_step_tokens)


def rounding_bound(max_abs):
    return 1e-5 + 4 * 2.0 ** -23 * max_abs


def operands(family, V, dtype, M=M_MAX, k=K, seed=0):
    """X [M, k], W [V, k] in `dtype` on the device such that X . W^T has the family's structure: N(0, 3) logits from the first k - 1 channels; channel k - 1 of X is
    1 and carries a column term of W: +80 in the last column (sink), a ramp rising by 60 across the vocabulary (ramp); `scaled`: the N(0, 3) logits times 3000."""
    g = torch.Generator(device='cuda').manual_seed(1000 * seed + 17 * FAMILIES.index(family) + V % 997)
    X = torch.randn(M, k, generator=g, device='cuda')
    W = torch.randn(V, k, generator=g, device='cuda') * (3.0 / (k - 1) ** 0.5)
    X[:, k - 1] = 1.0
    W[:, k - 1] = 0.0
    if family == 'sink':
        W[V - 1, k - 1] = 80.0
    elif family == 'ramp':
        W[:, k - 1] = 60.0 * torch.arange(V, device='cuda', dtype=torch.float32) / (V - 1)
    elif family == 'scaled':
        W *= 3000.0
    return X.to(dtype).contiguous(), W.to(dtype).contiguous()


def make_labels(M, V, seed=0):
    """column 0, V - 1, both sides of every chunk boundary the cases use, one ignored row, seeded random ids elsewhere"""
    g = torch.Generator().manual_seed(seed + V)
    lab = torch.randint(0, V, (M,), generator=g)
    fixed = [0, V - 1] + [c for c in INTERESTING if c < V]
    if M == 1:
        lab[0] = 256 if V <= 1000 else 8192
    else:
        for i, c in enumerate(fixed[:M - 1]):
            lab[i] = c
        lab[M - 1] = -100
    return lab.cuda()


@functools.lru_cache(maxsize=None)
def case(family, V, dtype):
    """(X, W, labels, float64 nll, float64 lse, per-row max |logit|, fp32 torch logits or None) for the M_MAX rows of a family; smaller M are its first rows"""
    X, W = operands(family, V, dtype)
    logits = X.float() @ W.float().t()
    labels = make_labels(M_MAX, V)
    l64 = logits.double()
    nll = F.cross_entropy(l64, labels, reduction='none', ignore_index=-100)
    lse = torch.logsumexp(l64, dim=1)
    gemm_err = None
    if dtype == torch.bfloat16:          # the product's own logits for the same operands: their distance from torch's is the bf16 term of the tolerance
        Y = torch.empty(M_MAX, V, dtype=torch.float32, device='cuda')
        raw(dtype).gemm_into(Y, X, W, out_f32=True)
        gemm_err = (Y - logits).abs().amax(dim=1)
    return X, W, labels, nll, lse, logits.abs().amax(dim=1), gemm_err


def run_nll(ops, X, W, labels, chunk_cols=0, ignore_index=-100, want_lse=True):
    from mmduet_amd._lib import lib, check
    from mmduet_amd.modeling_live import _ptr
    M, k = X.shape; V = W.shape[0]
    nll = torch.full((M,), 12345.0, dtype=torch.float32, device='cuda')
    lse = torch.full((M,), 12345.0, dtype=torch.float32, device='cuda') if want_lse else None
    ops.m._bind_stream()
    check(lib().mmd_op_lm_nll(ops.ctx, _ptr(X), _ptr(W), M, V, k, _ptr(labels), ignore_index, chunk_cols, _ptr(nll), _ptr(lse)), ops.ctx, 'mmd_op_lm_nll')
    torch.cuda.synchronize()
    return nll, lse


def relabel_for(M, V, labels):
    """the first M rows' labels; the last of them ignored, and for M = 1 the chunk-boundary column"""
    lab = labels[:M].clone()
    if M == 1:
        lab[0] = 256 if V <= 1000 else 8192
    elif M < M_MAX:
        lab[M - 1] = -100
    return lab


def expect_for(M, V, family, dtype):
    X, W, labels, nll, lse, mx, gerr = case(family, V, dtype)
    lab = relabel_for(M, V, labels)
    if not torch.equal(lab, labels[:M]):
        nll = F.cross_entropy((X[:M].float() @ W.float().t()).double(), lab, reduction='none', ignore_index=-100)
    extra = 2 * 3e-4 if dtype == torch.float32 else 2 * float(gerr[:M].max())
    tol = rounding_bound(mx[:M].double()) + extra
    return X[:M].contiguous(), W, lab, nll[:M], lse[:M], tol


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('V,chunk', [(1000, 256), (1000, 336), (152064, 0), (152064, 8192)])
@pytest.mark.parametrize('M', [1, 33, 300])
@pytest.mark.parametrize('family', FAMILIES)
def test_nll_and_lse_match_float64(family, M, V, chunk, dtype):
    X, W, lab, nll_ref, lse_ref, tol = expect_for(M, V, family, dtype)
    nll, lse = run_nll(raw(dtype), X, W, lab, chunk)
    e_nll = (nll.double() - nll_ref).abs(); e_lse = (lse.double() - lse_ref).abs()
    print(f'{family} M={M} V={V} chunk={chunk} {dtype}: nll err / tol {float((e_nll / tol).max()):.3f}, lse err / tol {float((e_lse / tol).max()):.3f}, tol {float(tol.max()):.3g}')
    assert torch.isfinite(nll).all() and torch.isfinite(lse).all()
    assert (e_nll <= tol).all(), (float(e_nll.max()), float(tol.max()))
    assert (e_lse <= tol).all(), (float(e_lse.max()), float(tol.max()))
    assert (nll[lab == -100] == 0).all() and (lab == -100).sum() == (0 if M == 1 else 1)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('M', [1, 33, 300])
@pytest.mark.parametrize('family', FAMILIES)
def test_result_does_not_depend_on_the_chunk_width(family, M, dtype):
    """chunk_cols 256 (four chunks, the last partial) against the vocabulary as ONE chunk: the rounding bound alone"""
    V = 1000
    X, W, lab, _, _, _ = expect_for(M, V, family, dtype)
    mx = case(family, V, dtype)[5][:M].double()
    a, la = run_nll(raw(dtype), X, W, lab, 256)
    b, lb = run_nll(raw(dtype), X, W, lab, V)
    d = torch.maximum((a.double() - b.double()).abs(), (la.double() - lb.double()).abs())
    print(f'{family} M={M} {dtype}: chunked vs single / bound {float((d / rounding_bound(mx)).max()):.3f}')
    assert (d <= rounding_bound(mx)).all(), float((d / rounding_bound(mx)).max())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_twenty_repeats_are_bit_identical(dtype):
    """M = 300, V = 152064: three vocabulary chunks, column-split partials and their merge in every one -- a race in the state merge would show as differing bits"""
    X, W, lab, _, _, _ = expect_for(300, 152064, 'normal', dtype)
    first = run_nll(raw(dtype), X, W, lab, 0)
    for _ in range(19):
        again = run_nll(raw(dtype), X, W, lab, 0)
        assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_out_of_range_label_gives_nan_in_its_row_only(dtype):
    V = 1000
    X, W, lab, nll_ref, _, tol = expect_for(33, V, 'normal', dtype)
    bad = lab.clone(); bad[3] = V; bad[7] = V + 12345; bad[11] = -7; bad[13] = 2 ** 40
    nll, lse = run_nll(raw(dtype), X, W, bad, 256)
    rows = torch.tensor([3, 7, 11, 13], device='cuda')
    assert torch.isnan(nll[rows]).all()
    keep = torch.ones(33, dtype=torch.bool, device='cuda'); keep[rows] = False
    assert ((nll.double() - nll_ref).abs()[keep] <= tol[keep]).all() and torch.isfinite(lse).all()


def test_a_row_block_of_ignored_labels_and_a_ragged_last_block():
    """max_step_tokens = 64: 300 rows are five row blocks (64 x 4 + 44); every label of the second one is ignored"""
    ops = raw(torch.float32, 64)
    V = 1000
    X, W, lab, _, lse_ref, tol = expect_for(300, V, 'ramp', torch.float32)
    lab = lab.clone(); lab[64:128] = -100
    nll_ref = F.cross_entropy((X.float() @ W.float().t()).double(), lab, reduction='none', ignore_index=-100)
    nll, lse = run_nll(ops, X, W, lab, 256)
    assert (nll[64:128] == 0).all()
    assert ((nll.double() - nll_ref).abs() <= tol).all() and ((lse.double() - lse_ref).abs() <= tol).all()


def test_custom_ignore_index_and_no_lse_buffer():
    X, W, lab, nll_ref, _, tol = expect_for(33, 1000, 'normal', torch.float32)
    lab = lab.clone(); lab[lab == -100] = 5; lab[4] = 5
    ref = F.cross_entropy((X.float() @ W.float().t()).double(), lab, reduction='none', ignore_index=5)
    nll, lse = run_nll(raw(torch.float32), X, W, lab, 336, ignore_index=5, want_lse=False)
    assert lse is None and ((nll.double() - ref).abs() <= tol).all() and (nll[lab == 5] == 0).all()


def test_true_width_lm_head():
    """M = 64 rows at the 7B model's lm_head: K = 3584, V = 152064, bf16, automatic chunk width (one chunk: the packed weight-streaming kernel serves it)"""
    dtype, V, k, M = torch.bfloat16, 152064, 3584, 64
    g = torch.Generator(device='cuda').manual_seed(5)
    X = torch.randn(M, k, generator=g, device='cuda').to(dtype)
    W = (torch.randn(V, k, generator=g, device='cuda') * (3.0 / k ** 0.5)).to(dtype)
    logits = X.float() @ W.float().t()
    lab = make_labels(M, V, seed=3)
    Y = torch.empty(M, V, dtype=torch.float32, device='cuda')
    raw(dtype).gemm_into(Y, X, W, out_f32=True)
    tol = rounding_bound(logits.abs().amax(dim=1).double()) + 2 * float((Y - logits).abs().max())
    del Y
    nll, lse = run_nll(raw(dtype), X, W, lab, 0)
    ref = F.cross_entropy(logits.double(), lab, reduction='none', ignore_index=-100)
    e_nll = (nll.double() - ref).abs(); e_lse = (lse.double() - torch.logsumexp(logits.double(), dim=1)).abs()
    print(f'true width: nll err / tol {float((e_nll / tol).max()):.3f}, lse err / tol {float((e_lse / tol).max()):.3f}, tol {float(tol.max()):.3g}')
    assert (e_nll <= tol).all() and (e_lse <= tol).all()


def test_argument_checks():
    from mmduet_amd._lib import lib
    from mmduet_amd.modeling_live import _ptr
    ops = raw(torch.float32)
    X, W, lab, _, _, _ = expect_for(33, 1000, 'normal', torch.float32)
    out = torch.zeros(33, dtype=torch.float32, device='cuda')
    f = lib().mmd_op_lm_nll
    assert f(ops.ctx, _ptr(X), _ptr(W), -1, 1000, K, _ptr(lab), -100, 0, _ptr(out), None) == -22
    assert f(ops.ctx, None, None, 0, 1000, K, None, -100, 0, None, None) == 0
    assert f(ops.ctx, None, _ptr(W), 33, 1000, K, _ptr(lab), -100, 0, _ptr(out), None) == -22
    assert f(ops.ctx, _ptr(X), _ptr(W), 33, 1000, K, None, -100, 0, _ptr(out), None) == -22
    assert f(ops.ctx, _ptr(X), _ptr(W), 33, 1000, K, _ptr(lab), -100, 0, None, None) == -22
    g = lib().mmd_lm_nll
    assert g(ops.ctx, None, -1, None, -100, 0, None, None) == -22
    assert g(ops.ctx, None, 0, None, -100, 0, None, None) == 0
    assert g(ops.ctx, None, 4, _ptr(lab), -100, 0, _ptr(out), None) == -22
