"""LoRA adapters are merged into the base matrices at load time (W += (alpha/r) B A in fp32, stored in the model dtype) whereas the reference keeps them
unmerged (PeftModel.from_pretrained, models/modeling_live.py:123: y = W x + (alpha/r) B (A x), every piece rounded to bf16).  ADVICE r01 asked whether
rounding the merged matrix to bf16 loses the adapter's signal.  Measured here at the 7B layer width for relative adapter magnitudes 1e-3 .. 3e-2:
the merged-bf16 output is as close to exact arithmetic as the reference's own unmerged bf16 execution (both are dominated by the bf16 rounding of the
output; the rounding of W + dW is unbiased and adds incoherently over K = 3584, the adapter's contribution adds coherently)."""
import math
import pytest
import torch


@pytest.mark.parametrize('rel', [1e-3, 3e-3, 1e-2, 3e-2])
def test_merged_bf16_weight_is_as_accurate_as_unmerged_bf16_execution(rel):
    torch.manual_seed(0)
    K, N, r, M, s = 3584, 1024, 16, 48, 2.0
    W = (torch.randn(N, K) * 0.02).bfloat16()
    x = torch.randn(M, K).bfloat16()
    A = (torch.randn(r, K) / math.sqrt(K)).bfloat16()
    B = torch.randn(N, r)
    B = (B * (rel * 0.02 / (s * (B @ A.float())).std())).bfloat16()
    dW = s * (B.float() @ A.float())
    exact = x.float() @ (W.float() + dW).T
    # the reference: unmerged, eager bf16 (each linear rounds its output, the scaled adapter output is added in bf16)
    base = (x.float() @ W.float().T).bfloat16()
    t = (x.float() @ A.float().T).bfloat16()
    lo = ((t.float() @ B.float().T).bfloat16().float() * s).bfloat16()
    ref = (base.float() + lo.float()).bfloat16().float()
    # this build: merged in fp32, stored in bf16
    merged = (x.float() @ (W.float() + dW).bfloat16().float().T).bfloat16().float()
    e_ref, e_mer, e_none = (ref - exact).std().item(), (merged - exact).std().item(), (base.float() - exact).std().item()
    assert e_mer <= 1.15 * e_ref + 1e-5, (e_mer, e_ref)
    if rel >= 3e-3:
        assert e_mer < 0.8 * e_none          # and the adapter's signal is there: ignoring it would be measurably worse


@pytest.mark.gpu
def test_merge_lora_bf16_against_unmerged_oracle():
    """The real path (mmd_merge_lora on a bf16 context, then the model's GEMMs) against y = W x + s B (A x) in fp32 on the same bf16 tensors.  The GEMM's weight is the
    matrix lora_merge_kernel wrote: W is loaded as the embedding table of a context whose vocabulary x hidden is N x K, merged there, finalized, and read back
    bit for bit through mmd_embed_tokens."""
    from rawops import RawOps
    from helpers import product_config
    from conftest import load_golden_weights
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    from mmduet_amd.weights import synthetic_weights
    g = torch.Generator().manual_seed(1)
    K, N, r, M, s = 1152, 512, 16, 64, 2.0
    W = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    A = (torch.randn(r, K, generator=g) / math.sqrt(K)).bfloat16()
    B = (torch.randn(N, r, generator=g) * 0.004).bfloat16()
    x = torch.randn(M, K, generator=g).bfloat16()
    cfgd, _ = load_golden_weights('A')
    pc = product_config(cfgd, vocab_size=N, hidden_size=K, num_attention_heads=9, num_key_value_heads=3, intermediate_size=128, num_hidden_layers=1)
    m = VideoHeadLiveLlavaQwenForCausalLM(pc, torch_dtype=torch.bfloat16, max_vit_batch=2, max_step_tokens=64, kv_initial_tokens=256)
    for name, t in synthetic_weights(pc, seed=1, device=m.device, dtype=torch.bfloat16):
        m.load_tensor(name, t)
    m.load_tensor('model.embed_tokens.weight', W.cuda())
    m.merge_lora('model.embed_tokens.weight', A.float(), B.float(), s)
    m.finalize()
    merged = m.get_input_embeddings()(torch.arange(N))                     # what the kernel stored, on the device
    exact_w = W.double() + s * (B.double() @ A.double())
    assert merged.dtype == torch.bfloat16 and not torch.equal(merged.cpu(), W)
    assert ((merged.cpu().double() - exact_w).abs() <= exact_w.abs() * 2.0 ** -8).all()          # it is the merge, to a bf16 rounding (tests/test_gpu_lora.py has the exact bound)
    Y = RawOps.around(m).gemm(x, merged, variant=0).float().cpu()
    exact = x.float() @ (W.float() + s * (B.float() @ A.float())).T
    base = (x.float() @ W.float().T).bfloat16()
    t = (x.float() @ A.float().T).bfloat16()
    ref = (base.float() + ((t.float() @ B.float().T).bfloat16().float() * s).bfloat16().float()).bfloat16().float()
    assert (Y - exact).std().item() <= 1.15 * (ref - exact).std().item() + 1e-5
    assert (Y - exact).std().item() < 0.8 * (base.float() - exact).std().item()          # and the adapter's signal is in what the GEMM computed
