"""References shared by the GPU parity tests (tests/test_gpu_production.py, tests/test_gpu_stress_*.py): plain torch attention in a chosen precision and
the max-norm error measure."""
import torch


def rel_err(got, ref):
    return (got.float() - ref.float()).abs().max().item() / max(1.0, ref.float().abs().max().item())


def ref_attention(q, K, V, nh, nkv, d, n_ctx, dtype=torch.float32, causal=True):
    """torch attention in `dtype` on q's device, one kv group at a time.  q [S, nh*d]; K/V [nkv, cap, d]; row r sees keys 0 .. n_ctx + r (all n_ctx + S
    keys when not causal)."""
    S = q.shape[0]; n_tot = n_ctx + S; rep = nh // nkv
    qh = q.to(dtype).view(S, nh, d).transpose(0, 1)
    out = torch.empty(nh, S, d, device=q.device, dtype=dtype)
    mask = torch.arange(n_tot, device=q.device)[None, :] > (torch.arange(S, device=q.device)[:, None] + n_ctx)
    for h in range(nkv):
        kk, vv = K[h, :n_tot].to(dtype), V[h, :n_tot].to(dtype)
        s = qh[h * rep:(h + 1) * rep] @ kk.T * d ** -0.5
        if causal:
            s = s.masked_fill(mask[None], float('-inf'))
        out[h * rep:(h + 1) * rep] = torch.softmax(s, -1) @ vv
    return out.transpose(0, 1).reshape(S, nh * d)


def ref_attention_rows(q, K, V, nh, nkv, d, n_ctx, rows, dtype=torch.float32):
    """attention in `dtype` of the query rows `rows` only (row r sees keys 0 .. n_ctx + r), one kv group and 256 Ki keys at a time with a running (max, sum) --
    the 1 M-key contexts never materialise an [S, n] score matrix.  q [S, nh*d]; K / V [nkv, cap, d] row-major."""
    rep = nh // nkv
    rows_t = torch.as_tensor(rows, device=q.device)
    qh = q.to(dtype).view(q.shape[0], nh, d)[rows_t].transpose(0, 1)              # [nh, R, d]
    out = torch.empty(nh, len(rows), d, device=q.device, dtype=dtype)
    n_max = n_ctx + max(rows) + 1
    for h in range(nkv):
        qq = qh[h * rep:(h + 1) * rep] * d ** -0.5
        m = torch.full((rep, len(rows), 1), float('-inf'), device=q.device, dtype=dtype); l = torch.zeros_like(m)
        acc = torch.zeros(rep, len(rows), d, device=q.device, dtype=dtype)
        for k0 in range(0, n_max, 1 << 18):
            k1 = min(n_max, k0 + (1 << 18))
            s = qq @ K[h, k0:k1].to(dtype).T
            dead = torch.arange(k0, k1, device=q.device)[None, :] > (rows_t[:, None] + n_ctx)
            s = s.masked_fill(dead[None], float('-inf'))
            m2 = torch.maximum(m, s.amax(-1, keepdim=True))
            p = torch.exp(s - m2); sc = torch.exp(m - m2)
            l = l * sc + p.sum(-1, keepdim=True); acc = acc * sc + p @ V[h, k0:k1].to(dtype); m = m2
        out[h * rep:(h + 1) * rep] = acc / l
    return out.transpose(0, 1).reshape(len(rows), nh * d)


def max_abs_score(q, K, nh, nkv, d, n_tot):
    """largest |q.k| d^-1/2 over the n_tot valid keys (float64): the magnitude an fp32 score has to be carried at"""
    S = q.shape[0]; rep = nh // nkv
    qh = q.double().view(S, nh, d).transpose(0, 1)
    return max((qh[h * rep:(h + 1) * rep] @ K[h, :n_tot].double().T).abs().max().item() for h in range(nkv)) * d ** -0.5
