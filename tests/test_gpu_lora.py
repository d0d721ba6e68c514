"""LoRA merge and weight intake on the device (tests/lora_cases.py states the cases and the float64 reference; tests/test_lora_host.py checks that reference alone).

The merged tensors are not readable through the ABI, but two entry points return a finalized matrix exactly: mmd_embed_tokens copies rows of the embedding table,
and mmd_video_heads on an H x H identity returns out[m, o] = W4[o, m] (every product is 1 w or 0 w).  So a merge into `model.embed_tokens.weight`, or into the
two head matrices, is compared with W + s B A in float64 element by element, to a bound derived from the arithmetic (lora_cases.merge_bound); mmd_load_tensor's
conversions are compared with torch's casts as bit patterns; and adapters over all seven decoder targets are checked through the finalized model -- fused qkv,
interleaved gate / up, packed and fp8 copies -- against the oracle on float64-merged weights, to the bound the same comparison has without an adapter."""
import ctypes as C
import pytest
import torch

pytestmark = pytest.mark.gpu
import lora_cases as LC
from helpers import product_config

DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}


def new_model(cfgd, dtype, weight_dtype=None):
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    pc = product_config(cfgd)
    if weight_dtype:
        pc.weight_dtype = weight_dtype
    return VideoHeadLiveLlavaQwenForCausalLM(pc, torch_dtype=dtype, max_vit_batch=8, max_step_tokens=512, kv_initial_tokens=512)


def read_embed(m):
    """the finalized embedding table [V, H], bit for bit"""
    return m.get_input_embeddings()(torch.arange(m.config.vocab_size)).cpu()


def read_heads(m):
    """the finalized informative | relevance head matrices [4, H] in the model dtype, bit for bit (a bf16 weight is exact in the fp32 output)"""
    H = m.config.hidden_size
    out = m.video_heads(torch.eye(H, dtype=m.dtype, device=m.device))
    return out.T.contiguous().to(m.dtype).cpu()


def tiny_context(tag, dtype, prepare):
    """golden config `tag` on a `dtype` context: every weight loaded (as stored), then prepare(m, w), finalize -> (m, stored base weights)"""
    cfgd, w = LC.golden(tag)
    m = new_model(cfgd, dtype)
    w = {k: v.to(dtype) for k, v in w.items()}
    for k, v in w.items():
        m.load_tensor(k, v)
    prepare(m, w)
    m.finalize()
    return m, w


# ---- 2. kernel-level merge, read back exactly -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=[(c['id'], d) for c in LC.KERNEL_CASES for d in DTYPES], ids=lambda p: f'{p[0]}-{p[1]}')
def merged(request):
    """one context per (case, dtype): all golden weights loaded, the case's merges applied in order, finalized, read back"""
    case_id, d = request.param
    dtype = DTYPES[d]
    ref = LC.kernel_reference(case_id, dtype)

    def prepare(m, w):
        for name, (base, pairs, _, _) in ref.items():
            assert torch.equal(base, w[name])
            for A, B, scale, r in pairs:
                m.merge_lora(name, A, B, scale)
    case = next(c for c in LC.KERNEL_CASES if c['id'] == case_id)
    m, w = tiny_context(case['tag'], dtype, prepare)
    heads = read_heads(m)
    return dtype, ref, w, {LC.EMBED: read_embed(m), LC.INF: heads[0:2], LC.REL: heads[2:4]}


def test_merge_equals_float64_reference_within_the_arithmetic_bound(merged):
    dtype, ref, w, got = merged
    for name, (base, pairs, exact, bound) in ref.items():
        assert got[name].dtype == dtype and got[name].shape == base.shape
        err = (got[name].double() - exact).abs()
        over = err > bound
        print(f'{name}: worst err / bound = {(err / bound).max().item():.3f} over {err.numel()} elements, merges {[(r, s) for _, _, s, r in pairs]}')
        assert not over.any(), (name, int(over.sum()), (err / bound).max().item())          # no element exempt


def test_merge_is_visible_and_leaves_other_tensors_alone(merged):
    dtype, ref, w, got = merged
    heads = [n for n in (LC.INF, LC.REL) if n in ref]
    for names in [[LC.EMBED]] + ([heads] if heads else []):
        g = torch.cat([got[n].reshape(-1) for n in names]); b = torch.cat([w[n].reshape(-1) for n in names])
        assert (g != b).double().mean().item() > 0.99
    for name in (LC.EMBED, LC.INF, LC.REL):
        if name not in ref:
            assert torch.equal(got[name].view(torch.int32 if dtype == torch.float32 else torch.int16), w[name].view(torch.int32 if dtype == torch.float32 else torch.int16))


@pytest.mark.parametrize('d', DTYPES)
def test_load_after_merge_leaves_the_loaded_tensor(d):
    """the modules_to_save order: the saved tensor overwrites whatever was merged, bit for bit"""
    dtype = DTYPES[d]
    g = torch.Generator().manual_seed(31)
    new = {}

    def prepare(m, w):
        for i, name in enumerate((LC.EMBED, LC.INF)):
            A, B = LC.pair(w[name], 16, 32 + i, 1.0, 2.0)
            m.merge_lora(name, A, B, 2.0)
            new[name] = (torch.randn(w[name].shape, generator=g) * 0.3).to(dtype)
            m.load_tensor(name, new[name])
    m, w = tiny_context('A', dtype, prepare)
    heads = read_heads(m)
    assert torch.equal(read_embed(m), new[LC.EMBED])
    assert torch.equal(heads[0:2], new[LC.INF]) and torch.equal(heads[2:4], w[LC.REL])


# ---- 3. mmd_load_tensor conversions, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('where', ['host', 'device'])
@pytest.mark.parametrize('src,ctx', [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                     (torch.float16, torch.bfloat16), (torch.float16, torch.float32), (torch.float64, torch.bfloat16), (torch.float64, torch.float32)],
                         ids=lambda t: str(t).replace('torch.', ''))
def test_load_tensor_conversion_is_bit_exact_with_torch(src, ctx, where):
    """expected: torch's cast on the CPU (fp16 / float64 sources widened to fp32 first, as model.load_tensor does), compared as bit patterns, NaNs as 'is NaN'"""
    cfgd, _ = LC.golden('A')
    V, H = cfgd['vocab_size'], cfgd['hidden_size']
    vals = LC.CONVERT_SOURCES[src](V * H).reshape(V, H)
    want = (vals if src in (torch.float32, torch.bfloat16) else vals.float()).to(ctx)

    def prepare(m, w):
        m.load_tensor(LC.EMBED, vals.cuda() if where == 'device' else vals)
    m, _ = tiny_context('A', ctx, prepare)
    got = read_embed(m)
    bad = LC.same_bits_or_both_nan(got, want)
    if bad:
        iv = torch.int32 if ctx == torch.float32 else torch.int16
        idx = torch.nonzero(torch.where(torch.isnan(want), ~torch.isnan(got), got.view(iv) != want.view(iv)).reshape(-1))[:8, 0]
        sv = vals.reshape(-1)[idx]
        print('first mismatches (source, got bits, want bits):', [(float(s), hex(int(a) & 0xFFFFFFFF), hex(int(b) & 0xFFFFFFFF)) for s, a, b in
                                                                  zip(sv.double(), got.reshape(-1).view(iv)[idx], want.reshape(-1).view(iv)[idx])])
    assert bad == 0, f'{bad} of {got.numel()} elements differ'
    assert int(torch.isnan(want).sum()) == int(torch.isnan(got).sum()) > 0


# ---- 4. every target through the finalized model ------------------------------------------------------------------------------------------------
def build_with_adapter(mode, case_id, tmp):
    from mmduet_amd.weights import load_lora_into
    spec = LC.mode_spec(mode)
    cfgd, w = LC.base_weights(mode)
    m = new_model(cfgd, spec['dtype'], 'fp8_e4m3' if mode == 'fp8' else None)
    for k, v in w.items():
        m.load_tensor(k, v)
    ad, saved = LC.case_adapter(mode, case_id)
    assert load_lora_into(m, LC.write_adapter(str(tmp), ad, saved, originals=w)) == len(ad)
    m.finalize()
    return m, cfgd, spec


@pytest.mark.parametrize('mode,case_id', [(mode, c['id']) for c in LC.MODEL_CASES for mode in LC.MODES if mode in c['modes']])
def test_adapter_through_the_finalized_model_matches_oracle_on_merged_weights(mode, case_id, tmp_path):
    case = LC.model_case(case_id)
    m, cfgd, spec = build_with_adapter(mode, case_id, tmp_path / 'adapter')
    got = LC.run_steps(m, LC.steps(cfgd, spec['dtype']), device=m.device)
    err = LC.worst(got, LC.reference_outputs(mode, case_id))
    moved = LC.worst(got, LC.reference_outputs(mode, None))
    print(f'{mode} {case_id}: |hip - oracle(merged)| {err}; |hip - oracle(base)| {moved}')
    excess = case['excess'].get(mode)
    for k, e in err.items():
        assert e < (LC.tol_of(mode, k) if excess is None else max(LC.tol_of(mode, k), 2 * excess[k])), (k, e)
    if len(case['targets']) == 1:          # and it is the merged model that ran: far from the oracle on the base weights where the reference is (tests/test_lora_host.py)
        assert any(moved[k] >= 5 * LC.tol_of(mode, k) for k in moved), moved
    if case['saved']:
        px = LC.pixels(cfgd)
        om = LC.oracle_on(mode, LC.merged_weights(mode, case_id), dtype=torch.float32 if mode == 'f32' else torch.bfloat16)
        vr = om.visual_embed(px).float()
        v0 = LC.oracle_on(mode, LC.base_weights(mode)[1], dtype=torch.float32 if mode == 'f32' else torch.bfloat16).visual_embed(px).float()
        ve = m.visual_embed(px.cuda()).float().cpu()
        tol = spec['ve_tol'] * max(1.0, vr.abs().max().item())
        print(f'{mode} {case_id}: visual_embed |hip - oracle(saved projector)| {(ve - vr).abs().max().item():.3g} (tol {tol:.3g}); oracle saved vs base {(vr - v0).abs().max().item():.3g}')
        assert (ve - vr).abs().max().item() < tol
        assert (vr - v0).abs().max().item() > 10 * tol          # the saved projector is not the base one


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def loaded():
    """golden A in fp32, every weight loaded, NOT finalized"""
    cfgd, w = LC.golden('A')
    m = new_model(cfgd, torch.float32)
    for k, v in w.items():
        m.load_tensor(k, v)
    return m, cfgd, w


def test_merge_into_an_unknown_tensor_names_it(loaded):
    from mmduet_amd._lib import MmduetError
    m, cfgd, w = loaded
    with pytest.raises(MmduetError, match='model.layers.7.self_attn.q_proj.weight'):
        m.merge_lora('model.layers.7.self_attn.q_proj.weight', torch.zeros(4, 64), torch.zeros(64, 4), 1.0)


def test_merge_into_a_vector_is_refused(loaded):
    from mmduet_amd._lib import lib
    MMD_EINVAL = -22
    m, cfgd, w = loaded
    H = cfgd['hidden_size']
    with pytest.raises(ValueError, match='model.norm.weight'):
        m.merge_lora('model.norm.weight', torch.zeros(1, H), torch.zeros(1, 1), 1.0)
    A, B = torch.zeros(1, H), torch.zeros(H, 1)          # the library itself, past the wrapper's check (buffers large enough for any reading of the shape)
    assert lib().mmd_merge_lora(m._ctx, b'model.norm.weight', C.c_void_p(A.data_ptr()), C.c_void_p(B.data_ptr()), 1, 1.0) == MMD_EINVAL
    assert b'not a matrix' in lib().mmd_last_error(m._ctx)


def test_adapter_that_does_not_fit_never_reaches_the_library(loaded):
    m, cfgd, w = loaded
    name = LC.weight_name(0, 'k_proj')
    A, B = LC.pair(w[LC.weight_name(0, 'q_proj')], 4, 1, 1.0, 1.0)          # q_proj's pair: B has twice k_proj's rows
    with pytest.raises(ValueError, match='k_proj'):
        m.merge_lora(name, A, B, 1.0)
    with pytest.raises(ValueError, match='disagree on r'):
        m.merge_lora(name, A[:2], B[:w[name].shape[0]], 1.0)


def test_merge_and_load_after_finalize_are_refused_and_change_nothing():
    from mmduet_amd._lib import MmduetError
    cfgd, w = LC.golden('A')
    m = new_model(cfgd, torch.float32)
    m.load_state_dict(w)
    xs = LC.steps(cfgd, torch.float32)
    before = LC.run_steps(m, xs, device=m.device)
    name = LC.weight_name(0, 'q_proj')
    A, B = LC.pair(w[name], 16, 3, 1.0, 2.0)
    with pytest.raises(MmduetError, match='q_proj'):
        m.merge_lora(name, A, B, 2.0)
    with pytest.raises(MmduetError, match='finalized'):
        m.load_tensor(name, w[name] * 2)
    with pytest.raises(MmduetError):
        m.merge_lora(LC.EMBED, *LC.pair(w[LC.EMBED], 4, 4, 1.0, 1.0), 1.0)
    after = LC.run_steps(m, xs, device=m.device)
    for a, b in zip(before, after):
        assert all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(read_embed(m), w[LC.EMBED])
