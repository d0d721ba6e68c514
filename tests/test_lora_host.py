"""Weight intake on the host: the adapter loader against a recording stand-in for the model (key spellings, scale, refusals before any native call), and the two
conditions tests/test_gpu_lora.py relies on, asserted on the reference alone -- a merge of tests/lora_cases.py is visible in more than 99 % of the elements it
is read back from, and every one-target adapter moves a compared output of the oracle by at least 10 x the tolerance it is compared with."""
import json
import pytest
import torch
import lora_cases as LC
from helpers import product_config
from mmduet_amd.weights import load_lora_into, load_pretrained_into, save_checkpoint, expected_tensors


class Recorder:
    """has what the loaders use of the model: config, load_tensor, merge_lora"""

    def __init__(self, tag='A'):
        self.cfgd, self.w = LC.golden(tag)
        self.config = product_config(self.cfgd)
        self.calls = []

    def load_tensor(self, name, t):
        self.calls.append(('load', name, t.clone()))

    def merge_lora(self, name, A, B, scale):
        self.calls.append(('merge', name, A.clone(), B.clone(), scale))

    def merges(self):
        return {c[1]: c for c in self.calls if c[0] == 'merge'}

    def loads(self):
        return {c[1]: c[2] for c in self.calls if c[0] == 'load'}


def write(tmp_path, tensors, r=4, alpha=6):
    from safetensors.torch import save_file
    d = tmp_path / 'adapter'; d.mkdir()
    save_file({k: v.contiguous() for k, v in tensors.items()}, str(d / 'adapter_model.safetensors'))
    json.dump({'r': r, 'lora_alpha': alpha}, open(d / 'adapter_config.json', 'w'))
    return str(d)


def ab(rec, name, r=4, seed=0):
    out_f, in_f = rec.w[name].shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(r, in_f, generator=g), torch.randn(out_f, r, generator=g)


def test_key_spellings_map_to_canonical_names_and_scale_is_alpha_over_r(tmp_path):
    rec = Recorder()
    q0, d1, k1, g0 = (LC.weight_name(0, 'q_proj'), LC.weight_name(1, 'down_proj'), LC.weight_name(1, 'k_proj'), LC.weight_name(0, 'gate_proj'))
    pairs = {n: ab(rec, n, seed=i) for i, n in enumerate((q0, d1, k1, g0))}
    mod = lambda n: n[:-len('.weight')]
    new = {n: torch.randn(rec.w[n].shape, generator=torch.Generator().manual_seed(40 + i)) for i, n in enumerate(LC.PROJECTOR + (LC.INF, LC.REL))}
    t = {f'base_model.model.{mod(q0)}.lora_A.weight': pairs[q0][0], f'base_model.model.{mod(q0)}.lora_B.weight': pairs[q0][1],                       # prefix, no adapter name
         f'base_model.model.{mod(d1)}.lora_A.default.weight': pairs[d1][0], f'base_model.model.{mod(d1)}.lora_B.default.weight': pairs[d1][1],       # prefix, .default.
         f'{mod(k1)}.lora_A.weight': pairs[k1][0], f'{mod(k1)}.lora_B.weight': pairs[k1][1],                                                         # neither
         f'{mod(g0)}.lora_A.default.weight': pairs[g0][0], f'{mod(g0)}.lora_B.default.weight': pairs[g0][1],                                         # no prefix, .default.
         # the projector's indexed names, as PEFT wraps the Sequential: <module>.modules_to_save.default.<index>.<param>
         'base_model.model.model.mm_projector.modules_to_save.default.0.weight': new[LC.PROJECTOR[0]],
         'base_model.model.model.mm_projector.modules_to_save.default.0.bias': new[LC.PROJECTOR[1]],
         'base_model.model.model.mm_projector.modules_to_save.default.2.weight': new[LC.PROJECTOR[2]],
         'model.mm_projector.2.bias': new[LC.PROJECTOR[3]],                                                                                          # as a saved adapter file spells it
         'base_model.model.informative_head.modules_to_save.default.weight': new[LC.INF],
         'base_model.model.relevance_head.weight': new[LC.REL],
         # what PEFT keeps of the replaced tensors: never loaded
         'base_model.model.model.mm_projector.original_module.0.weight': rec.w[LC.PROJECTOR[0]] + 1,
         'base_model.model.informative_head.original_module.weight': rec.w[LC.INF] + 1,
         'base_model.model.some_other_module.weight': torch.zeros(3)}                                                                                # not on the path: ignored
    assert load_lora_into(rec, write(tmp_path, t, r=4, alpha=6)) == 4
    merges, loads = rec.merges(), rec.loads()
    assert set(merges) == set(pairs)
    for n, (A, B) in pairs.items():
        _, _, gA, gB, scale = merges[n]
        assert torch.equal(gA, A) and torch.equal(gB, B) and scale == 6 / 4
    assert set(loads) == set(new) and all(torch.equal(loads[n], new[n]) for n in new)
    assert len(rec.calls) == len(pairs) + len(new)          # nothing twice, no original_module


def test_written_adapter_round_trips_through_the_loader(tmp_path):
    """the writer the GPU tests use (LC.write_adapter, the PEFT spelling with original_module copies) -> the loader: every pair under its name, scale alpha / r"""
    rec = Recorder()
    ad, saved = LC.case_adapter('f32', 'saved+q_proj')
    _, w = LC.base_weights('f32')
    assert load_lora_into(rec, LC.write_adapter(str(tmp_path / 'a'), ad, saved, originals=w)) == len(ad) == rec.cfgd['num_hidden_layers']
    merges, loads = rec.merges(), rec.loads()
    assert set(merges) == set(ad) and set(loads) == set(saved) == set(LC.PROJECTOR + (LC.INF, LC.REL))
    for n, (A, B) in ad.items():
        assert torch.equal(merges[n][2], A) and torch.equal(merges[n][3], B) and merges[n][4] == LC.ALPHA / LC.R
    assert all(torch.equal(loads[n], saved[n]) for n in saved)


@pytest.mark.parametrize('drop', ['lora_A', 'lora_B'])
def test_unmatched_half_of_a_pair_is_a_key_error_before_any_call(tmp_path, drop):
    rec = Recorder()
    q0, q1 = LC.weight_name(0, 'q_proj'), LC.weight_name(1, 'q_proj')
    t = {}
    for n in (q0, q1):
        A, B = ab(rec, n)
        t[f'base_model.model.{n[:-7]}.lora_A.weight'], t[f'base_model.model.{n[:-7]}.lora_B.weight'] = A, B
    del t[f'base_model.model.{q1[:-7]}.{drop}.weight']
    t['base_model.model.informative_head.modules_to_save.default.weight'] = rec.w[LC.INF]
    with pytest.raises(KeyError, match='q_proj'):
        load_lora_into(rec, write(tmp_path, t))
    assert rec.calls == []


@pytest.mark.parametrize('what', ['A_in', 'B_out', 'r_disagree', 'transposed', 'A_1d', 'k_as_q'])
def test_adapter_that_does_not_fit_is_a_value_error_before_any_call(tmp_path, what):
    rec = Recorder()
    name = LC.weight_name(1, 'k_proj')                    # [32, 64] on golden A
    A, B = ab(rec, name)
    if what == 'A_in':
        A = torch.randn(4, A.shape[1] + 1)
    elif what == 'B_out':
        B = torch.randn(B.shape[0] - 1, 4)
    elif what == 'r_disagree':
        B = torch.randn(B.shape[0], 8)
    elif what == 'transposed':
        A, B = A.T.contiguous(), B.T.contiguous()
    elif what == 'A_1d':
        A = A.reshape(-1)
    elif what == 'k_as_q':                                # a q_proj pair under k_proj's name: B has the q rows
        A, B = ab(rec, LC.weight_name(1, 'q_proj'))
    good = LC.weight_name(0, 'down_proj')                 # sorts before the bad one: must not have been merged either
    gA, gB = ab(rec, good)
    t = {f'{name[:-7]}.lora_A.weight': A, f'{name[:-7]}.lora_B.weight': B, f'{good[:-7]}.lora_A.weight': gA, f'{good[:-7]}.lora_B.weight': gB,
         'informative_head.weight': rec.w[LC.INF]}
    with pytest.raises(ValueError, match='k_proj'):
        load_lora_into(rec, write(tmp_path, t))
    assert rec.calls == []


def test_check_lora_shapes_accepts_what_fits():
    from mmduet_amd.weights import check_lora_shapes
    rec = Recorder()
    shapes = expected_tensors(rec.config)
    for t in LC.TARGETS:
        n = LC.weight_name(0, t)
        A, B = ab(rec, n, r=16)
        check_lora_shapes(n, A, B, shapes[n])
        assert shapes[n] == tuple(rec.w[n].shape)
    with pytest.raises(ValueError):
        check_lora_shapes('model.norm.weight', torch.zeros(4, 64), torch.zeros(64, 4), shapes['model.norm.weight'])          # a 1-D target


def test_checkpoint_loader_hands_over_every_tensor_once(tmp_path):
    """load_pretrained_into against the recorder: LLaVA's spellings of the tower names arrive under the canonical ones, the deleted layer and the pooling head do not arrive"""
    from oracle import duet_oracle as O
    rec = Recorder()
    extra = {}
    for k, v in rec.w.items():
        extra[k.replace(O.VT, 'model.vision_tower.vision_tower.') if 'layers.0.' in k and k.startswith(O.VT) else k] = v          # the spelling without vision_model.
    C = rec.cfgd['vit_hidden_size']
    extra[O.VT + f"encoder.layers.{rec.cfgd['vit_layers']}.layer_norm1.weight"] = torch.ones(C)
    extra[O.VT + 'head.probe'] = torch.zeros(1, 1, C)
    extra['model.image_newline'] = torch.zeros(rec.cfgd['hidden_size'])
    del extra[LC.REL]
    save_checkpoint(extra, str(tmp_path / 'ck'), rec.config)
    assert load_pretrained_into(rec, str(tmp_path / 'ck')) == [LC.REL]
    loads = rec.loads()
    need = set(expected_tensors(rec.config)) - {LC.REL}
    assert set(loads) == need and len(rec.calls) == len(need)
    assert all(torch.equal(loads[n], rec.w[n]) for n in need)


# ---- what the GPU tests rely on, on the reference alone -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', LC.KERNEL_CASES, ids=lambda c: c['id'])
def test_kernel_case_merges_are_visible_in_the_reference(case, dtype):
    ref = LC.kernel_reference(case['id'], dtype)
    heads = [n for n in (LC.INF, LC.REL) if n in ref]
    groups = [[LC.EMBED]] + ([heads] if heads else [])          # the heads are read back as one matrix
    for names in groups:
        base = torch.cat([ref[n][0].reshape(-1) for n in names])
        want = torch.cat([ref[n][2].to(dtype).reshape(-1) for n in names])
        assert (want != base).double().mean().item() > 0.99
        bound = torch.cat([ref[n][3].reshape(-1) for n in names])
        exact = torch.cat([ref[n][2].reshape(-1) for n in names])
        # and the bound separates the merge from no merge, a dropped scale and a transposed index by a wide margin: most elements of the update are > 100 bounds
        assert ((exact - base.double()).abs() > 100 * bound).double().mean().item() > (0.9 if dtype == torch.float32 else 0.5)


def test_merge_bound_is_the_stated_formula():
    W = torch.tensor([[1.0, -2.0]]); A = torch.tensor([[0.5, 0.25]]); B = torch.tensor([[-4.0]])
    exact = LC.merge_ref64(W, A, B, 0.5)
    assert exact.tolist() == [[0.0, -2.5]]
    b32 = LC.merge_bound(W, A, B, 0.5, 1, torch.float32)
    assert b32.tolist() == [[4 * 2.0 ** -24 * 2.0, 4 * 2.0 ** -24 * 2.5]]
    b16 = LC.merge_bound(W, A, B, 0.5, 1, torch.bfloat16)
    assert LC.bf16_half_ulp(exact).tolist() == [[2.0 ** -134, 2.0 ** (1 - 8)]]          # 0: the subnormal spacing; 2.5: floor(log2) = 1
    assert torch.equal(b16, b32 + LC.bf16_half_ulp(exact))
    x = torch.tensor([1.0, 1.9999, 2.0, 2.0 ** -126, 2.0 ** -127, 2.0 ** -140, 3e38], dtype=torch.float64)
    assert LC.bf16_half_ulp(x).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -134, 2.0 ** -134, 2.0 ** -134, 2.0 ** 119]
    # half an ulp really is the worst rounding error of torch's cast
    v = torch.randn(4096, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    assert ((v.to(torch.bfloat16).double() - v).abs() <= LC.bf16_half_ulp(v)).all()


def test_conversion_values_hold_every_named_edge():
    n = 512 * 64
    f = LC.convert_values_f32(n)
    b = f.to(torch.bfloat16)
    assert f.numel() == n and LC.convert_values_bf16(n).numel() == n and LC.convert_values_f16(n).numel() == n and LC.convert_values_f64(n).numel() == n
    assert torch.isnan(f).sum() > 4 and torch.isinf(f).sum() >= 2 and (f == 0).sum() >= 2
    assert (torch.isinf(b) & ~torch.isinf(f)).sum() >= 3                                   # finite fp32 that rounds to bf16 inf
    sub = (b != 0) & (b.float().abs() < 2.0 ** -126)
    assert sub.sum() >= 4                                                                  # bf16-subnormal results
    bits = f.view(torch.int32)
    tie = ((bits & 0xFFFF) == 0x8000) & torch.isfinite(f)
    up = tie & (((bits >> 16) & 1) == 1); down = tie & (((bits >> 16) & 1) == 0)
    assert up.sum() >= 3 and down.sum() >= 3                                               # ties to even in both directions
    assert (b.view(torch.int16)[up].int() & 1 == 0).all() and (b.view(torch.int16)[down].int() & 1 == 0).all()


@pytest.mark.parametrize('mode', LC.MODES)
@pytest.mark.parametrize('case_id', LC.ONE_TARGET_IDS)
def test_one_target_adapter_moves_the_oracle_by_ten_tolerances(mode, case_id):
    if mode not in LC.model_case(case_id)['modes']:
        return
    moved = LC.worst(LC.reference_outputs(mode, case_id), LC.reference_outputs(mode, None))
    assert any(moved[k] >= 10 * LC.tol_of(mode, k) for k in moved), moved


@pytest.mark.parametrize('mode', LC.MODES)
def test_model_case_adapters_are_what_the_issue_names(mode):
    cfgd, w = LC.base_weights(mode)
    L = cfgd['num_hidden_layers']
    full, _ = LC.case_adapter(mode, 'full')
    assert set(full) == {LC.weight_name(i, t) for i in range(L) for t in LC.TARGETS}
    for n, (A, B) in full.items():
        assert A.shape == (16, w[n].shape[1]) and B.shape == (w[n].shape[0], 16)
        assert abs(LC.rms((LC.ALPHA / LC.R) * (B.double() @ A.double())) / LC.rms(w[n]) - LC.FULL_REL) < 1e-3 * LC.FULL_REL
    last, _ = LC.case_adapter('bf16', 'k_proj-last')
    assert set(last) == {LC.weight_name(LC.base_weights('bf16')[0]['num_hidden_layers'] - 1, 'k_proj')}
    ad, saved = LC.case_adapter(mode, 'saved+q_proj')
    assert set(ad) == {LC.weight_name(i, 'q_proj') for i in range(L)} and set(saved) == set(LC.PROJECTOR + (LC.INF, LC.REL))


@pytest.mark.parametrize('target,mode', [(t, m) for t, by_mode in LC.ONE_TARGET_EXCESS.items() for m in by_mode])
def test_recorded_excess_is_the_references_own(target, mode):
    """the excess a case table entry records is what the oracle in bf16 loses against the oracle in float64 on the same merged weights -- not more than that"""
    cfgd, _ = LC.base_weights(mode)
    mw, xs = LC.merged_weights(mode, target), LC.steps(cfgd, torch.bfloat16)
    lo = LC.run_steps(LC.oracle_on(mode, mw, torch.bfloat16), xs)
    hi = LC.run_steps(LC.oracle_on(mode, mw, torch.float64), [x.double() for x in xs])
    measured, recorded = LC.worst(lo, hi), LC.ONE_TARGET_EXCESS[target][mode]
    assert all(recorded[k] <= 1.25 * measured[k] for k in measured), (measured, recorded)          # (bf16 matmuls on another CPU may sum in another order)
