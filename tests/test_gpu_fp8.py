"""fp8-e4m3 weight path (BASELINE configs[4]): per-output-channel scaled OCP e4m3fn weights, bf16 activations, fp32
accumulate.  Parity is stated separately from the bf16 build, as the survey asks:
  * the quantiser is BIT-EXACT against torch's float8_e4m3fn cast of W / scale (scale = amax / 448);
  * every GEMM regime (fp8-streaming GEMV / skinny kernels at M <= 64, bf16(q) tile kernels above) equals fp32 math on the DEQUANTISED weights to the
    bf16 bound (1.2e-2 x max(1, |ref|));
  * the model equals the oracle run on the dequantised weights (fp32 oracle: 6e-2 on O(1) logits, the bf16 bound of the unquantised build);
  * against the UNQUANTISED model the delta is the quantisation error itself -- reported, and bounded loosely (0.35 on O(1) logits at the tiny widths).
A YouCook2-style stream (stream_end_score_sum_threshold 2, remove_assistant_turns, scripts/inference/youcook2.sh:12-14) runs on the fp8 model against the
oracle on the dequantised weights."""
import ctypes as C
import math
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
from oracle import duet_oracle as O


@pytest.fixture(scope='module')
def ops():
    from rawops import RawOps
    return RawOps(torch.bfloat16)


from rawops import quantize_ref          # noqa: E402  (shared with tests/test_gpu_gemm_regimes.py)


def hip_quantize(ops, W):
    return ops.quantize_fp8(W)


def hip_gemm_w8(ops, X, Wq, q8, sc, bias=None, R=None, epi='none', variant=0):
    from mmduet_amd._lib import lib, check, EPI
    M, K = X.shape; N = Wq.shape[0]
    NO = N // 2 if epi == 'swiglu' else N
    Y = torch.empty(M, NO, device=ops.dev, dtype=torch.bfloat16)
    Xd = X.to(ops.dev, torch.bfloat16).contiguous()
    bd = bias.to(ops.dev, torch.bfloat16).contiguous() if bias is not None else None
    Rd = R.to(ops.dev, torch.bfloat16).contiguous() if R is not None else None
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ops.m._bind_stream()
    check(lib().mmd_op_gemm_w8(ops.ctx, p(Xd), p(Wq), p(q8), p(sc), p(bd), p(Rd), p(Y), M, N, K, EPI[epi], 0, variant), ops.ctx, 'gemm_w8')
    torch.cuda.synchronize()
    return Y


@pytest.mark.parametrize('N,K', [(64, 64), (4608, 3584), (160, 18944), (2048, 1152)])
def test_quantiser_is_bit_exact_with_torch_e4m3fn(ops, N, K):
    g = torch.Generator().manual_seed(N + K)
    W = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    W[0] = 0                                    # an all-zero channel keeps scale 1 and q 0
    W[1, 3] = 7.0                               # an outlier channel: everything else lands in the subnormal range of e4m3
    Wq, q8, sc = hip_quantize(ops, W)
    q_ref, s_ref = quantize_ref(W)
    assert torch.equal(sc.cpu(), s_ref)
    assert torch.equal(q8.cpu(), q_ref.view(torch.uint8))
    assert torch.equal(Wq.cpu().float(), q_ref.float())                 # the bf16 copy holds exactly the fp8 values


@pytest.mark.parametrize('M', [1, 7, 16, 33, 49, 64, 98, 147, 200, 256, 1274])
@pytest.mark.parametrize('N,K,epi', [(4608, 3584, 'none'), (3584, 3584, 'resid'), (1024, 3584, 'swiglu'), (3584, 18944, 'resid')])
def test_fp8_gemm_every_regime_matches_fp32_on_dequantised_weights(ops, M, N, K, epi):
    """tolerance: 1.2e-2 x max(1, |ref|max) -- the bf16 output bound; the quantised VALUES are exact in every kernel"""
    if M > 64 and K > 4000 and N * K > 3584 * 18944:
        pytest.skip('size')
    dev = ops.dev
    g = torch.Generator(device=dev).manual_seed(M * 131 + N + K)
    X = (torch.randn(M, K, generator=g, device=dev) * 0.7).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g, device=dev) / math.sqrt(K)).to(torch.bfloat16)
    b = (0.1 * torch.randn(N, generator=g, device=dev)).to(torch.bfloat16) if epi == 'none' else None
    if epi == 'swiglu':
        W = torch.stack([W[:N // 2].view(-1, 16, K), W[N // 2:].view(-1, 16, K)], 1).reshape(N, K).contiguous()       # interleaved gate / up rows
    Wq, q8, sc = hip_quantize(ops, W)
    Wd = Wq.float() * sc[:, None]                                                                                      # dequantised weights
    R = torch.randn(M, N, generator=g, device=dev).to(torch.bfloat16) if epi == 'resid' else None
    Y = hip_gemm_w8(ops, X, Wq, q8, sc, b, R, epi)
    lin = F.linear(X.float(), Wd, b.float() if b is not None else None)
    if epi == 'resid':
        ref = lin.to(torch.bfloat16).float() + R.float()
    elif epi == 'swiglu':
        v = lin.view(M, -1, 2, 16)
        gg, uu = v[:, :, 0].reshape(M, -1).to(torch.bfloat16).float(), v[:, :, 1].reshape(M, -1).to(torch.bfloat16).float()
        ref = F.silu(gg).to(torch.bfloat16).float() * uu
    else:
        ref = lin
    err = (Y.float() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    assert torch.isfinite(Y.float()).all() and err <= 1.2e-2 * (2.0 if epi != 'none' else 1.0), err


# ---- model level ------------------------------------------------------------------------------------------------------------------------
CFG = dict(vocab_size=512, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, rope_theta=1e6,
           rms_norm_eps=1e-6, vit_hidden_size=32, vit_intermediate_size=64, vit_layers=2, vit_heads=4, vit_image_size=56, vit_patch_size=14,
           video_pooling_stride=2, mm_spatial_pool_mode='bilinear', frame_num_tokens=4, frame_resolution=56)
LIN = ('q_proj', 'k_proj', 'v_proj', 'o_proj', 'gate_proj', 'up_proj', 'down_proj')


def _models():
    from helpers import product_config
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    ocfg = O.OracleConfig(**CFG)
    w = O.random_weights(ocfg, seed=5, dtype=torch.bfloat16, scale='unit')
    built = {}
    for wd in (None, 'fp8_e4m3'):
        pc = product_config(CFG)
        pc.weight_dtype = wd
        m = VideoHeadLiveLlavaQwenForCausalLM(pc, torch_dtype=torch.bfloat16, max_vit_batch=8, max_step_tokens=512, kv_initial_tokens=512)
        m.load_state_dict(w)
        built[wd] = m
    wd = dict(w)
    for k, v in w.items():
        if k.startswith('model.layers.') and k.endswith('.weight') and any(f'.{n}.' in k for n in LIN):
            q, s = quantize_ref(v)
            wd[k] = q.float() * s[:, None]
    return built[None], built['fp8_e4m3'], O.OracleModel(ocfg, {k: v.float() for k, v in wd.items()}), O.OracleModel(ocfg, {k: v.float() for k, v in w.items()}), ocfg


@pytest.fixture(scope='module')
def models():
    return _models()


def test_fp8_model_matches_oracle_on_dequantised_weights(models):
    m16, m8, o_deq, o_full, ocfg = models
    g = torch.Generator().manual_seed(1)
    steps = [torch.randn(1, 23, 128, generator=g) * 0.5, torch.randn(1, 4, 128, generator=g) * 0.5, torch.randn(1, 1, 128, generator=g) * 0.5,
             torch.randn(1, 100, 128, generator=g) * 0.5, torch.randn(1, 1, 128, generator=g) * 0.5]
    c8 = c16 = cd = cf = None
    worst_deq = worst_full = worst_q = 0.0
    for x in steps:
        xb = x.to(torch.bfloat16)
        o8 = m8(inputs_embeds=xb.cuda(), past_key_values=c8); c8 = o8.past_key_values
        o16 = m16(inputs_embeds=xb.cuda(), past_key_values=c16); c16 = o16.past_key_values
        rd = o_deq(inputs_embeds=xb.float(), past_key_values=cd); cd = rd.past_key_values
        rf = o_full(inputs_embeds=xb.float(), past_key_values=cf); cf = rf.past_key_values
        for got, rdq, rfu, g16 in ((o8.informative_logits[0, -1], rd.informative_logits[0, -1], rf.informative_logits[0, -1], o16.informative_logits[0, -1]),
                                   (o8.relevance_logits[0, -1], rd.relevance_logits[0, -1], rf.relevance_logits[0, -1], o16.relevance_logits[0, -1]),
                                   (o8.logits[0, -1], rd.logits[0, -1], rf.logits[0, -1], o16.logits[0, -1])):
            worst_deq = max(worst_deq, (got.float().cpu() - rdq).abs().max().item())
            worst_full = max(worst_full, (got.float().cpu() - rfu).abs().max().item())
            worst_q = max(worst_q, (got.float().cpu() - g16.float().cpu()).abs().max().item())
    print(f'fp8 model: vs fp32 oracle on dequantised weights {worst_deq:.4f}; vs fp32 oracle on the original weights {worst_full:.4f}; vs the bf16 build {worst_q:.4f}')
    assert worst_deq < 6e-2          # same bound as the unquantised bf16 build against its oracle
    assert worst_full < 0.35 and worst_q < 0.35     # the quantisation error itself (3 mantissa bits), loose


def test_fp8_chunked_forward_equals_per_frame_steps(models):
    """The fp8-streaming kernels (M <= 64) and the bf16(q) tile kernels (chunks) carry the same weights bit for bit: a chunk equals per-frame steps up to
    accumulation order (6e-2), as in the bf16 build."""
    _, m8, _, _, _ = models
    g = torch.Generator().manual_seed(2)
    frames = [(torch.randn(4, 128, generator=g) * 0.5).to(torch.bfloat16).cuda() for _ in range(40)]
    base = m8(inputs_embeds=(torch.randn(1, 9, 128, generator=g) * 0.5).to(torch.bfloat16).cuda()).past_key_values
    per, cache = [], base
    for f in frames:
        sc, cache = m8.frame_step(f[None], cache, [3]); per.append(sc[0])
    chunk, c2 = m8.frame_step(torch.cat(frames)[None], m8.cache_prefix(base, len(base)), [4 * (j + 1) - 1 for j in range(40)])
    assert len(c2) == len(cache)
    assert (chunk - torch.stack(per)).abs().max().item() < 6e-2


def test_youcook2_style_stream_on_fp8_weights(models):
    """stream_end_score_sum_threshold 2 + remove_assistant_turns (scripts/inference/youcook2.sh:12-14).  With the assistant turns removed from the context
    every frame score is independent of what was generated, so the whole score trace of the fp8 build is comparable with the oracle on the dequantised weights
    (5e-2 on probabilities); response frames agree unless the running sum passes the threshold within that tolerance."""
    from helpers import make_args, tokenizer_for
    from mmduet_amd.inference import LiveInferForBenchmark
    _, m8, o_deq, _, ocfg = models
    g = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (24, 3, 56, 56), dtype=torch.uint8, generator=g)
    conv = [{'role': 'user', 'content': 'describe every step', 'time': 0.0}]

    def run(model, k):
        a = make_args(frame_fps=0.5, system_prompt='A tiny assistant.', max_new_tokens=6, stream_end_score_sum_threshold=2.0, remove_assistant_turns=True,
                      score_heads='informative_score', frames_per_forward=k, bf16=hasattr(model, '_ctx'))
        tok = tokenizer_for(model.config)
        model.config.eos_token_id = -1
        d = LiveInferForBenchmark(a, model=model, tokenizer=tok)
        d.input_video_stream(frames); d.input_query_stream(conv)
        resp = d.inference()
        return d, [x['informative_score'] for x in d.debug_data_list], [r['time'] for r in resp if r['role'] == 'assistant']

    d8, s8, t8 = run(m8, 1)
    d8k, s8k, t8k = run(m8, 5)
    do, so, to_ = run(o_deq, 1)
    assert len(s8) == len(so) == 24
    assert max(abs(a - b) for a, b in zip(s8, so)) < 5e-2
    assert max(abs(a - b) for a, b in zip(s8, s8k)) < 5e-2
    assert len(d8.past_key_values) == len(do.past_key_values) == len(d8k.past_key_values)         # responses never stay in the context
    if t8 != to_:                                                                                # only a borderline running sum may move a response by a frame
        assert abs(len(t8) - len(to_)) <= 1
    assert len(t8) >= 1


def test_fp8_model_at_7b_width_chunk_and_decode_rows():
    """the fp8 build at the TRUE decoder width (hidden 3584, 28 / 4 heads of 128, intermediate 18 944; 2 layers, vocab 2048): a 26-frame
    chunk (M = 1274 + prefix: bf16(q) tile kernels with the scale in the epilogue), per-frame steps (fp8-streaming skinny kernel) and single decode rows (fp8 GEMV,
    decode chain, fused attention prologue) against the oracle on the DEQUANTISED weights in fp32 -- and the three regimes against each other.
    tolerance: 6e-2 on O(1) head logits / 8e-2 on lm logits (the bf16 bound of the unquantised build at 2 layers, tests/test_gpu_production.py)."""
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    from mmduet_amd.weights import synthetic_weights
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=2, vit_num_hidden_layers=2, vit_layers_removed=1, frame_num_tokens=49, frame_resolution=384, v_placeholder='<image>')
    pcfg.weight_dtype = 'fp8_e4m3'
    ocfg = O.OracleConfig(vocab_size=2048, num_hidden_layers=2, vit_layers=1)
    m = VideoHeadLiveLlavaQwenForCausalLM(pcfg, torch_dtype=torch.bfloat16, max_vit_batch=2, max_step_tokens=1536, kv_initial_tokens=4096)
    w = {}
    for name, t in synthetic_weights(pcfg, seed=3, device=m.device, dtype=torch.bfloat16, scale='unit'):
        m.load_tensor(name, t); w[name] = t
    m.finalize()
    wd = {}
    for k, v in w.items():
        if k.startswith('model.layers.') and k.endswith('.weight') and any(f'.{l}.' in k for l in LIN):
            q, sc = quantize_ref(v)
            wd[k] = q.float() * sc[:, None]
        else:
            wd[k] = v.float()
    o32 = O.OracleModel(ocfg, wd)
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(2)
    prompt = (torch.randn(1, 29, 3584, generator=g, device=dev) * 0.5).to(torch.bfloat16)
    frames = [(torch.randn(49, 3584, generator=g, device=dev) * 0.5).to(torch.bfloat16) for _ in range(26)]
    rows = [49 * (j + 1) - 1 for j in range(26)]
    base = m(inputs_embeds=prompt).past_key_values
    per, cache = [], m.cache_prefix(base, len(base))
    for f in frames:
        sc, cache = m.frame_step(f[None], cache, [48]); per.append(sc[0])
    per = torch.stack(per)
    chunk, c_chunk = m.frame_step(torch.cat(frames)[None], m.cache_prefix(base, len(base)), rows)          # (same arena: rolls back to the prompt, then the 26 frames in one forward)
    oc = o32(inputs_embeds=prompt.float()).past_key_values
    ref = o32(inputs_embeds=torch.cat(frames)[None].float(), past_key_values=oc)
    want = torch.cat([ref.informative_logits[0, rows], ref.relevance_logits[0, rows]], -1).cpu()
    e_chunk, e_per, e_cp = (chunk - want).abs().max().item(), (per - want).abs().max().item(), (chunk - per).abs().max().item()
    # short chunks (2 .. 5 frames = 98 .. 245 rows per forward: gemm_stream_kernel on the bf16(q) copy, the per-channel scale applied to its fp32 slabs / in its
    # SwiGLU epilogue, fused slab consumers) -- round 4: the regime between the per-frame step and the tile GEMMs
    e_short = 0.0
    base2 = m(inputs_embeds=prompt).past_key_values          # (its own arena: the chunk's context above is continued by the decode rows below)
    for kf in (2, 3, 4, 5):
        cache_s, got = m.cache_prefix(base2, len(base2)), []
        for j0 in range(0, 10, kf):
            fr = frames[j0:j0 + kf]
            sc, cache_s = m.frame_step(torch.cat(fr)[None], cache_s, [49 * (j + 1) - 1 for j in range(len(fr))])
            got.append(sc)
        got = torch.cat(got)[:10]
        e_short = max(e_short, (got - want[:10]).abs().max().item())
    assert e_short < 6e-2, e_short
    # decode rows: 6 single-token steps from the chunk's context, lm logits of each
    toks = [(torch.randn(1, 1, 3584, generator=g, device=dev) * 0.5).to(torch.bfloat16) for _ in range(6)]
    hc, ocache, e_dec, e_lm = c_chunk, ref.past_key_values, 0.0, 0.0
    for t in toks:
        out = m(inputs_embeds=t, past_key_values=hc); hc = out.past_key_values
        r = o32(inputs_embeds=t.float(), past_key_values=ocache); ocache = r.past_key_values
        e_dec = max(e_dec, (torch.cat([out.informative_logits[0, -1], out.relevance_logits[0, -1]]).cpu() - torch.cat([r.informative_logits[0, -1], r.relevance_logits[0, -1]]).cpu()).abs().max().item())
        e_lm = max(e_lm, (out.logits[0, -1].float().cpu() - r.logits[0, -1].cpu()).abs().max().item())
    assert len(hc) == 29 + 26 * 49 + 6
    try:
        import json, os
        from conftest import ROOT
        path = os.path.join(ROOT, 'gpurun_out', 'parity_r04.json')
        cur = json.load(open(path)) if os.path.exists(path) else {}
        cur['fp8_true_width_2_layers'] = dict(chunk_vs_fp32=e_chunk, per_frame_vs_fp32=e_per, chunk_vs_per_frame=e_cp, short_chunks_vs_fp32=e_short, decode_rows_head_vs_fp32=e_dec, decode_rows_lm_vs_fp32=e_lm,
                                              lm_scale=r.logits.abs().max().item())
        json.dump(cur, open(path, 'w'), indent=1, sort_keys=True)
    except Exception:
        pass
    assert e_chunk < 6e-2 and e_per < 6e-2 and e_cp < 6e-2 and e_dec < 6e-2, (e_chunk, e_per, e_cp, e_dec)
    assert e_lm < 8e-2 * max(1.0, r.logits.abs().max().item()), e_lm
