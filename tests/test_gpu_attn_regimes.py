"""Every row of the attention regime table (tests/attn_regimes.py) that mmd_op_attention can reach, on the device, through the C ABI:

  * form -- mmd_op_attention_last_form reports the row's (form, key splits): the intended kernel really ran over the intended split;
  * the output is finite;
  * parity -- against plain torch attention in float64 on the same inputs (parity_common.ref_attention), within the bound of tests/test_gpu_stress_attention.py, unchanged:
    max|o - ref| <= 1.8e-2 max(1, max|ref|) for forms 3, 4, 5 and 8, assert_close(scale = 1.5) of tests/test_gpu_ops.py for the others.

Inputs are the benign randn data of tests/test_gpu_ops.py.  The rows the operator cannot reach (the automatic choices over the arena, the tower's layout, form 9, the
rejections) are checked on the host by tests/test_attn_plan_host.py; form 9 runs on the device in test_gpu_production.py (mmd_round_multi)."""
import zlib
import pytest
import torch

pytestmark = pytest.mark.gpu
import attn_regimes as T
from parity_common import ref_attention
from test_gpu_ops import assert_close

DTYPES = {T.BF16: torch.bfloat16, T.F32: torch.float32}


@pytest.fixture(scope='module')
def ctxs():
    """one RawOps context per dtype, released with the module"""
    c = {}
    yield c
    c.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('row', T.OP_ROWS, ids=[r.name for r in T.OP_ROWS])
def test_attention_regime(ctxs, row):
    dtype = DTYPES[row.dtype]
    if dtype not in ctxs:
        from rawops import RawOps
        ctxs[dtype] = RawOps(dtype)
    ops = ctxs[dtype]
    S, nh, nkv, d, n_ctx = row.S, row.nh, row.nkv, row.d, row.n_ctx
    cap = (n_ctx + S + 63) // 64 * 64
    g = torch.Generator(device=ops.dev).manual_seed(zlib.crc32(row.name.encode()))
    q = torch.randn(S, nh * d, generator=g, device=ops.dev).to(dtype)
    K = torch.randn(nkv, cap, d, generator=g, device=ops.dev).to(dtype)
    V = torch.randn(nkv, cap, d, generator=g, device=ops.dev).to(dtype)
    o = ops.attention(q, K, V, nh, nkv, d, n_ctx, row.causal, row.variant)
    form = ops.attention_last_form()
    assert form == (row.form, row.splits), (row.name, form)
    assert torch.isfinite(o.float()).all(), row.name
    ref = ref_attention(q, K, V, nh, nkv, d, n_ctx, torch.float64, row.causal)
    err = (o.double() - ref).abs().max().item()
    den = max(1.0, ref.abs().max().item())
    print(f'{row.name}: form {form}, max|o - ref| / max(1, |ref|) = {err / den:.3e}')
    if row.form in (3, 4, 5, 8):
        assert err <= 1.8e-2 * den, (row.name, err / den)
    else:
        assert_close(o, ref, dtype, scale=1.5, what=row.name)
