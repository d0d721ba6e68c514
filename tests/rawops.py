"""ctypes access to the raw operator entry points (mmd_op_*) for the GPU parity tests."""
import ctypes as C
import torch
from mmduet_amd._lib import lib, check, EPI
from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM, _ptr
from helpers import product_config
from conftest import load_golden_weights


def quantize_ref(W):
    """Host-side statement of the fp8 scheme: per output channel, scale = amax / 448, q = float8_e4m3fn(W / scale) (round to nearest even)."""
    Wf = W.float()
    amax = Wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    q = (Wf / scale[:, None]).to(torch.float8_e4m3fn)
    return q, scale


# out-of-range write checks: quiet NaNs with a payload no kernel produces (a computed NaN is the canonical 0x7FC0 / 0x7FC00000)
SENTINEL_BITS = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5A5A5}
_INT_OF = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


def guarded(rows, cols, dtype, device, before=16, after=256):
    """A [before + rows + after, cols] buffer filled with the sentinel; -> (buffer, the [rows, cols] view in its middle).  256 rows after Y: a
    whole row tile of the largest kernel (ring: 256 rows) past M."""
    buf = torch.empty(before + rows + after, cols, dtype=dtype, device=device)
    buf.view(_INT_OF[dtype]).fill_(SENTINEL_BITS[dtype])
    return buf, buf[before:before + rows]


def sentinel_intact(t):
    """True when every element of t still holds the sentinel bits"""
    return bool((t.view(_INT_OF[t.dtype]) == SENTINEL_BITS[t.dtype]).all())


class RawOps:
    def __init__(self, dtype, max_step_tokens=64):
        """max_step_tokens > 2048: the context gets the large (192 MB) split-K slab workspace of a model that runs several streams' merged chunks."""
        cfgd, _ = load_golden_weights('A')
        self.m = VideoHeadLiveLlavaQwenForCausalLM(product_config(cfgd), torch_dtype=dtype, max_vit_batch=2, max_step_tokens=max_step_tokens, kv_initial_tokens=256)
        self.ctx, self.dtype, self.dev = self.m._ctx, dtype, self.m.device

    @classmethod
    def around(cls, model):
        """The raw calls on a model that exists already -- one with its weights loaded: mmd_op_embed_feed reads the context's embedding table."""
        self = cls.__new__(cls)
        self.m, self.ctx, self.dtype, self.dev = model, model._ctx, model.dtype, model.device
        return self

    def t(self, x):
        return x.to(device=self.dev, dtype=self.dtype).contiguous()

    def gemm(self, X, W, bias=None, R=None, epi='none', out_f32=False, variant=0):
        M, K = X.shape; N = W.shape[0]
        NO = N // 2 if epi == 'swiglu' else N
        Y = torch.empty(M, NO, device=self.dev, dtype=torch.float32 if out_f32 else self.dtype)
        self.m._bind_stream()
        Xd, Wd = self.t(X), self.t(W)                      # keep the device copies alive across the launch
        bd = self.t(bias) if bias is not None else None
        Rd = self.t(R) if R is not None else None
        check(lib().mmd_op_gemm(self.ctx, _ptr(Xd), _ptr(Wd), _ptr(bd), _ptr(Rd), _ptr(Y), M, N, K, EPI[epi], int(out_f32), variant), self.ctx, 'gemm')
        torch.cuda.synchronize()
        return Y

    # ---- raw calls on caller-owned device buffers (tests/test_gpu_gemm_regimes.py): no copies, Y may sit inside a guarded buffer ----
    def last_plan(self):
        """(kernel GEMM_K_*, output tiles, K splits, blocks) of this context's most recent GEMM"""
        p = (C.c_int * 4)()
        check(lib().mmd_op_gemm_last_plan(self.ctx, p), self.ctx, 'last_plan')
        return tuple(p)

    def gemm_into(self, Y, X, W, bias=None, R=None, epi='none', out_f32=False, variant=0):
        M, K = X.shape; N = W.shape[0]
        self.m._bind_stream()
        check(lib().mmd_op_gemm(self.ctx, _ptr(X), _ptr(W), _ptr(bias), _ptr(R), _ptr(Y), M, N, K, EPI[epi], int(out_f32), variant), self.ctx, 'gemm')
        torch.cuda.synchronize()

    def gemm_w8_into(self, Y, X, Wq, q8, scale, bias=None, R=None, epi='none', variant=0):
        M, K = X.shape; N = Wq.shape[0]
        self.m._bind_stream()
        check(lib().mmd_op_gemm_w8(self.ctx, _ptr(X), _ptr(Wq), _ptr(q8), _ptr(scale), _ptr(bias), _ptr(R), _ptr(Y), M, N, K, EPI[epi], 0, variant), self.ctx, 'gemm_w8')
        torch.cuda.synchronize()

    def gemm_slabs_into(self, slabs, X, W, max_splits, variant=2):
        """slabs: device fp32 with room for max_splits x [M, N]; -> number of slabs written"""
        M, K = X.shape; N = W.shape[0]
        n = C.c_int(0)
        self.m._bind_stream()
        check(lib().mmd_op_gemm_slabs(self.ctx, _ptr(X), _ptr(W), M, N, K, variant, _ptr(slabs), max_splits, C.byref(n)), self.ctx, 'gemm_slabs')
        torch.cuda.synchronize()
        return n.value

    def quantize_fp8(self, W):
        """mmd_op_quantize_fp8 on a copy of W [N, K]: -> (bf16(q) [N, K], q8 bytes [N, K], scale [N] fp32)"""
        N, K = W.shape
        Wq = W.to(device=self.dev, dtype=torch.bfloat16).contiguous().clone()
        q8 = torch.empty(N, K, dtype=torch.uint8, device=self.dev)
        sc = torch.empty(N, dtype=torch.float32, device=self.dev)
        self.m._bind_stream()
        check(lib().mmd_op_quantize_fp8(self.ctx, _ptr(Wq), N, K, _ptr(q8), _ptr(sc)), self.ctx, 'quantize')
        torch.cuda.synchronize()
        return Wq, q8, sc

    def gemm_slabs(self, X, W, variant=2, max_splits=16):
        """-> (sum of the fp32 partial slabs [M, N], number of slabs)"""
        M, K = X.shape; N = W.shape[0]
        Xd, Wd = self.t(X), self.t(W)
        slabs = torch.zeros(max_splits, M, N, device=self.dev, dtype=torch.float32)
        n = C.c_int(0)
        self.m._bind_stream()
        check(lib().mmd_op_gemm_slabs(self.ctx, _ptr(Xd), _ptr(Wd), M, N, K, variant, _ptr(slabs), max_splits, C.byref(n)), self.ctx, 'gemm_slabs')
        torch.cuda.synchronize()
        return slabs[:max(1, n.value)].sum(0), n.value

    def rmsnorm(self, x, w, eps):
        xd, wd = self.t(x), self.t(w)
        y = torch.empty_like(xd); self.m._bind_stream()
        check(lib().mmd_op_rmsnorm(self.ctx, _ptr(xd), _ptr(wd), _ptr(y), x.shape[0], x.shape[1], eps), self.ctx)
        torch.cuda.synchronize()
        return y

    def layernorm(self, x, w, b, eps):
        xd, wd, bd = self.t(x), self.t(w), self.t(b)
        y = torch.empty_like(xd); self.m._bind_stream()
        check(lib().mmd_op_layernorm(self.ctx, _ptr(xd), _ptr(wd), _ptr(bd), _ptr(y), x.shape[0], x.shape[1], eps), self.ctx)
        torch.cuda.synchronize()
        return y

    def rope_append(self, qkv, nh, nkv, d, theta, pos0, Kc, Vc):
        S = qkv.shape[0]
        q = torch.empty(S, nh * d, device=self.dev, dtype=self.dtype); self.m._bind_stream()
        qd = self.t(qkv)
        check(lib().mmd_op_rope_append(self.ctx, _ptr(qd), S, nh, nkv, d, theta, pos0, _ptr(q), _ptr(Kc), _ptr(Vc), Kc.shape[1]), self.ctx)
        return q

    def kv_write(self, writer, src, inv_freq, nh, nkv, d, pos0, q_out, Kc, Vc, S=None, bias=None, row0=0, attn_out=None):
        """mmd_op_kv_write on caller-owned device buffers.  Writers 0-2: src = qkv [S, w].  Writers 3 / 4: src = fp32 slabs [n_slabs, slab_rows, w], this step's S rows
        start at slab row `row0`.  inv_freq: CPU fp32 [d / 2].  -> the return code (nothing raises: refusals are part of what is tested)."""
        w = (nh + 2 * nkv) * d
        n_slabs, slab_rows, at = 0, 0, src.data_ptr()
        if writer >= 3:
            n_slabs, slab_rows = src.shape[0], src.shape[1]
            at += row0 * w * 4
        else:
            S = src.shape[0]
        fr = inv_freq.contiguous().float()
        self.m._bind_stream()
        rc = lib().mmd_op_kv_write(self.ctx, writer, C.c_void_p(at), n_slabs, slab_rows, _ptr(bias), C.c_void_p(fr.data_ptr()), S, nh, nkv, d, pos0, _ptr(q_out), _ptr(Kc), _ptr(Vc),
                                   Kc.shape[1], _ptr(attn_out))
        torch.cuda.synchronize()
        return rc

    def slab_resid_rmsnorm(self, slabs, resid, h_out, norm_w, eps, xn_out, wscale=None, splits=None, M=None, H=None):
        """mmd_op_slab_resid_rmsnorm on caller-owned device buffers (slabs fp32 [splits, M, H]; h_out may be resid).  -> the return code: refusals are part of what is tested"""
        splits = slabs.shape[0] if splits is None else splits
        M = slabs.shape[1] if M is None else M
        H = slabs.shape[2] if H is None else H
        self.m._bind_stream()
        rc = lib().mmd_op_slab_resid_rmsnorm(self.ctx, _ptr(slabs), splits, M, H, _ptr(resid), _ptr(h_out), _ptr(norm_w), eps, _ptr(xn_out), _ptr(wscale))
        torch.cuda.synchronize()
        return rc

    def gemv_chain(self, role, X, W, h, ssq, M, N, K, gamma=None, eps=0.0, Y=None, q8=None, scale=None, epi='none', max_splits=0):
        """mmd_op_gemv_chain on caller-owned device buffers: role 2 the producer (h [M, N] in place, ssq written), role 1 the consumer (h [M, K], gamma, ssq read; Y fp32 slabs
        with room for max_splits, or the SwiGLU product).  -> (return code, slabs written)"""
        n = C.c_int(0)
        self.m._bind_stream()
        rc = lib().mmd_op_gemv_chain(self.ctx, role, _ptr(X), _ptr(W), _ptr(q8), _ptr(scale), _ptr(h), _ptr(gamma), _ptr(ssq), eps, _ptr(Y), M, N, K, EPI[epi], max_splits, C.byref(n))
        torch.cuda.synchronize()
        return rc, n.value

    # ---- the kernels of the greedy token loop (tests/test_gpu_greedy.py): every call returns the native code, refusals are part of what is tested ----
    def argmax(self, form, logits, prev_ids, prev_off, penalties, tokens_out, tok_slots_out=None, append_out=None, n=None, V=None):
        """mmd_op_argmax on caller-owned device buffers: logits [n, V] fp32, prev_ids int64 (all lists back to back, or None), prev_off a list of n + 1 offsets, penalties a
        list of n floats (<= 0: none); tokens_out / tok_slots_out / append_out int64 [n] (the last two for form 2)."""
        n = logits.shape[0] if n is None else n
        V = logits.shape[1] if V is None else V
        off = (C.c_int32 * len(prev_off))(*prev_off)
        pen = (C.c_float * max(1, len(penalties)))(*penalties)
        self.m._bind_stream()
        rc = lib().mmd_op_argmax(self.ctx, form, _ptr(logits), n, V, _ptr(prev_ids), off, pen, _ptr(tokens_out), _ptr(tok_slots_out), _ptr(append_out))
        torch.cuda.synchronize()
        return rc

    def advance_state(self, token, eos, use_penalty, prev, prev_cap, n_prev, n_ctx, step):
        """mmd_op_advance_state: prev a device int64 buffer of at least prev_cap slots.  -> (return code, n_prev, n_ctx, step afterwards)"""
        a, b, c = C.c_int(n_prev), C.c_int64(n_ctx), C.c_int(step)
        self.m._bind_stream()
        rc = lib().mmd_op_advance_state(self.ctx, int(token), int(eos), int(use_penalty), _ptr(prev), prev_cap, C.byref(a), C.byref(b), C.byref(c))
        torch.cuda.synchronize()
        return rc, a.value, b.value, c.value

    def embed_feed(self, tok_slots, rows, out, out_rows=None):
        """mmd_op_embed_feed: tok_slots device int64 [n], rows a list of n row indices of out [out_rows, H]"""
        r = (C.c_int32 * max(1, len(rows)))(*rows)
        self.m._bind_stream()
        rc = lib().mmd_op_embed_feed(self.ctx, _ptr(tok_slots), r, len(rows), out.shape[0] if out_rows is None else out_rows, _ptr(out))
        torch.cuda.synchronize()
        return rc

    def attention_last_form(self):
        f = (C.c_int * 2)()
        check(lib().mmd_op_attention_last_form(self.ctx, f), self.ctx, 'attention_last_form')
        return tuple(f)

    def attention(self, q, Kc, Vc, nh, nkv, d, n_ctx, causal=True, variant=0):
        S = q.shape[0]
        o = torch.empty(S, nh * d, device=self.dev, dtype=self.dtype); self.m._bind_stream()
        qd = self.t(q)
        check(lib().mmd_op_attention(self.ctx, _ptr(qd), _ptr(Kc), _ptr(Vc), _ptr(o), S, nh, nkv, d, n_ctx, Kc.shape[1], int(causal), variant), self.ctx)
        torch.cuda.synchronize()
        return o

    def pool(self, x, grid, mode, stride):
        B, _, H = x.shape
        out = -(-grid // stride) if mode == 0 else stride if mode == 3 else grid // stride
        y = torch.empty(B, out * out, H, device=self.dev, dtype=self.dtype); self.m._bind_stream()
        xd = self.t(x)
        check(lib().mmd_op_pool(self.ctx, _ptr(xd), _ptr(y), B, grid, H, mode, stride), self.ctx)
        torch.cuda.synchronize()
        return y
