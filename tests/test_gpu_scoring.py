"""Teacher-forced scoring through the model call: forward(labels=..., informative_labels=..., relevance_labels=...) returns the reference's lm_loss / video_loss / loss
(models/live_llava/video_head_live_llava_qwen.py:163-189) without ever holding all-position logits for the loss (model.token_nll -> mmd_lm_nll).

The expectation comes from the reference's own recorded logits in tests/golden/cfg{A,B}_ops.npz run through torch's CrossEntropyLoss.  A loss is a mean of
(logsumexp - label logit): it moves by at most twice the logit error, hence 2 x the logit tolerances of tests/test_gpu_model.py.
"""
import pytest
import torch
import torch.nn.functional as F
from conftest import load_npz
from helpers import hip_model, oracle_model, product_config

pytestmark = pytest.mark.gpu

F32_TOL = 3e-4           # tests/test_gpu_model.py: fp32 HIP path vs reference fp32
BF16_TOL = 6e-2          # tests/test_gpu_model.py: bf16 HIP path vs the oracle executed in bf16


def seeded_labels(S, V, seed, ignore_every=3):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, V, (1, S), generator=g)
    lab[0, torch.rand(S, generator=g) < 1.0 / ignore_every] = -100
    if not (lab != -100).any():
        lab[0, 0] = int(torch.randint(0, V, (1,), generator=g))
    return lab


def seeded_video_labels(S, seed):
    """[1, S] of {0, 1, -100}"""
    g = torch.Generator().manual_seed(seed)
    return torch.tensor([0, 1, -100])[torch.randint(0, 3, (1, S), generator=g)]


def ref_video_loss(inf, rel, il, rl):
    """the reference expression (:178-183) over recorded head logits [S,2]"""
    video_labels = torch.cat([il, rl], dim=0).clone()
    video_logits = torch.cat([inf[None], rel[None]], dim=0).float()
    if not (video_labels != -100).any():
        video_labels[:, 0] = 0
    return F.cross_entropy(video_logits.flatten(0, 1), video_labels.flatten())


@pytest.fixture(scope='module', params=['A', 'B'])
def f32(request):
    m, cfgd, w = hip_model(request.param, torch.float32)
    m.config.all_position_logits = True
    ops = {k: torch.from_numpy(v) for k, v in load_npz(f'cfg{request.param}_ops.npz').items()}
    return request.param, m, cfgd, w, ops


def test_losses_of_six_steps_match_the_recorded_reference(f32):
    tag, m, cfgd, w, ops = f32
    V = cfgd['vocab_size']
    m.lm_loss_weight, m.video_loss_weight = 0.75, 1.5
    try:
        cache = None
        for i in range(6):
            x = ops[f'step{i}_in']; S = x.shape[0]
            labels = seeded_labels(S, V, 10 + i); il = seeded_video_labels(S, 20 + i); rl = seeded_video_labels(S, 30 + i)
            if i == 4:          # the one-row step: make its label count
                labels[0, 0] = 7
            out = m(inputs_embeds=x[None].cuda(), past_key_values=cache, labels=labels.clone(), informative_labels=il, relevance_labels=rl)
            cache = out.past_key_values
            lm_ref = F.cross_entropy(ops[f'step{i}_logits'].float(), labels[0])
            v_ref = ref_video_loss(ops[f'step{i}_inf'], ops[f'step{i}_rel'], il, rl)
            assert out.lm_loss.shape == () and out.lm_loss.dtype == torch.float32 and out.lm_loss.is_cuda
            print(f'{tag} step {i}: lm_loss {float(out.lm_loss):.6f} ref {float(lm_ref):.6f}; video_loss {float(out.video_loss):.6f} ref {float(v_ref):.6f}')
            assert abs(float(out.lm_loss) - float(lm_ref)) < 2 * F32_TOL
            assert abs(float(out.video_loss) - float(v_ref)) < 2 * F32_TOL
            assert abs(float(out.loss) - (0.75 * float(out.lm_loss) + 1.5 * float(out.video_loss))) < 1e-6
            assert len(cache) == int(ops[f'step{i}_kvlen'])
            assert (out.logits[0].cpu() - ops[f'step{i}_logits']).abs().max().item() < F32_TOL
    finally:
        m.lm_loss_weight = m.video_loss_weight = 1


def test_token_nll_combines_forced_chunks(f32):
    """chunk_cols = 128: four (A, V = 512) / three (B, V = 320, the last partial) vocabulary chunks inside the model's own lm_head"""
    tag, m, cfgd, w, ops = f32
    V = cfgd['vocab_size']
    x = ops['step0_in']; S = x.shape[0]
    labels = seeded_labels(S, V, 41)
    out = m(inputs_embeds=x[None].cuda())
    nll, lse = m.token_nll(out.hidden_states[0], labels[0], chunk_cols=128, return_lse=True)
    ref = F.cross_entropy(ops['step0_logits'].float(), labels[0], reduction='none')
    assert (nll.cpu() - ref).abs().max().item() < 2 * F32_TOL
    assert (lse.cpu() - torch.logsumexp(ops['step0_logits'].float(), dim=1)).abs().max().item() < 2 * F32_TOL
    auto = m.token_nll(out.hidden_states[0], labels[0])
    assert (auto - nll).abs().max().item() < 1e-5 + 4 * 2.0 ** -23 * ops['step0_logits'].abs().max().item()
    assert nll.dtype == torch.float32 and nll.is_cuda and (nll[labels[0].cuda() == -100] == 0).all()


def test_reference_quirks(f32):
    tag, m, cfgd, w, ops = f32
    V = cfgd['vocab_size']
    x = ops['step0_in']; S = x.shape[0]
    gold = ops['step0_logits'].float()
    ids = torch.randint(0, V, (1, S), generator=torch.Generator().manual_seed(3))
    # all labels ignored + input_ids: labels[:, 0] = input_ids[:, 1] in the CALLER's tensor (:168-169)
    labels = torch.full((1, S), -100)
    out = m(input_ids=ids, inputs_embeds=x[None].cuda(), labels=labels)
    assert int(labels[0, 0]) == int(ids[0, 1]) and (labels[0, 1:] == -100).all()
    assert abs(float(out.lm_loss) - float(F.cross_entropy(gold, labels[0]))) < 2 * F32_TOL
    assert out.video_loss == 0. and abs(float(out.loss) - float(out.lm_loss)) < 1e-7
    # ... and without input_ids the reference fails with a TypeError
    with pytest.raises(TypeError):
        m(inputs_embeds=x[None].cuda(), labels=torch.full((1, S), -100))
    # all video labels ignored: position 0 of BOTH rows of the concatenated copy counts as class 0; the caller's tensors stay as they were
    il = torch.full((1, S), -100); rl = torch.full((1, S), -100)
    out = m(inputs_embeds=x[None].cuda(), informative_labels=il, relevance_labels=rl)
    assert (il == -100).all() and (rl == -100).all()
    assert abs(float(out.video_loss) - float(ref_video_loss(ops['step0_inf'], ops['step0_rel'], il, rl))) < 2 * F32_TOL
    assert out.lm_loss == 0. and abs(float(out.loss) - float(out.video_loss)) < 1e-7
    # one video label tensor alone: no video loss
    labels = seeded_labels(S, V, 5)
    out = m(inputs_embeds=x[None].cuda(), labels=labels, informative_labels=seeded_video_labels(S, 6))
    assert out.video_loss == 0. and abs(float(out.loss) - float(out.lm_loss)) < 1e-7
    out = m(inputs_embeds=x[None].cuda(), relevance_labels=seeded_video_labels(S, 6))
    assert out.video_loss == 0. and out.lm_loss == 0. and out.loss == 0.
    # return_dict=False: the loss comes first
    tup = m(inputs_embeds=x[None].cuda(), labels=labels, return_dict=False)
    assert len(tup) == 3 and abs(float(tup[0]) - float(F.cross_entropy(gold, labels[0]))) < 2 * F32_TOL and tup[1].shape == (1, S, V)
    # a label >= V raises like torch's loss
    bad = labels.clone(); bad[0, 2] = V
    with pytest.raises(IndexError):
        m(inputs_embeds=x[None].cuda(), labels=bad)
    with pytest.raises(IndexError):
        m.token_nll(out.hidden_states[0], torch.full((S,), -5))


@pytest.mark.parametrize('tag', ['A', 'B'])
def test_bf16_lm_loss_matches_the_bf16_oracle(tag):
    m, cfgd, w = hip_model(tag, torch.bfloat16)
    om, _, _ = oracle_model(tag, torch.bfloat16)
    ops = {k: torch.from_numpy(v) for k, v in load_npz(f'cfg{tag}_ops.npz').items()}
    V = cfgd['vocab_size']
    cache = ocache = None
    for i in range(5):
        x = ops[f'step{i}_in'][None]; S = x.shape[1]
        labels = seeded_labels(S, V, 50 + i)
        if i == 4:
            labels[0, 0] = 7
        out = m(inputs_embeds=x.cuda(), past_key_values=cache, labels=labels.clone()); cache = out.past_key_values
        oo = om(inputs_embeds=x, past_key_values=ocache); ocache = oo.past_key_values
        ref = F.cross_entropy(oo.logits[0].float(), labels[0])
        print(f'{tag} bf16 step {i}: lm_loss {float(out.lm_loss):.5f} oracle {float(ref):.5f}')
        assert abs(float(out.lm_loss) - float(ref)) < 2 * BF16_TOL


def test_long_sequence_equals_the_count_weighted_losses_of_two_calls():
    """S = 75 > max_step_tokens = 32: __call__ loops mmd_llm_step three times and mmd_lm_nll walks three row blocks (32 + 32 + 11)"""
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    from conftest import load_golden_weights
    cfgd, w = load_golden_weights('A')
    m = VideoHeadLiveLlavaQwenForCausalLM(product_config(cfgd), torch_dtype=torch.float32, max_vit_batch=8, max_step_tokens=32, kv_initial_tokens=512)
    m.load_state_dict(w)
    V = cfgd['vocab_size']
    ids = torch.randint(0, V, (1, 75), generator=torch.Generator().manual_seed(9))
    x = m.get_input_embeddings()(ids.cuda())
    labels = seeded_labels(75, V, 61)
    whole = m(inputs_embeds=x, labels=labels.clone())
    a = m(inputs_embeds=x[:, :40], labels=labels[:, :40].clone())
    b = m(inputs_embeds=x[:, 40:], labels=labels[:, 40:].clone(), past_key_values=a.past_key_values)
    na, nb = int((labels[0, :40] != -100).sum()), int((labels[0, 40:] != -100).sum())
    assert na > 0 and nb > 0 and len(whole.past_key_values) == 75 == len(b.past_key_values)
    two = (float(a.lm_loss) * na + float(b.lm_loss) * nb) / (na + nb)
    print(f'long: {float(whole.lm_loss):.6f} vs two calls {two:.6f}')
    assert abs(float(whole.lm_loss) - two) < 2 * F32_TOL


def test_no_cost_without_labels():
    """A label-free call after the scoring path has run is what it was on the fresh model: same bits, same launches per kernel class"""
    m, cfgd, w = hip_model('A', torch.float32)
    m.config.all_position_logits = True
    ops = {k: torch.from_numpy(v) for k, v in load_npz('cfgA_ops.npz').items()}
    x = ops['step0_in'][None].cuda(); S = x.shape[1]

    def plain():
        m.prof_enable(True); m.prof_reset()
        out = m(inputs_embeds=x)
        h, lg = out.hidden_states.clone(), out.logits.clone()
        torch.cuda.synchronize()
        launches = {k: v['launches'] for k, v in m.prof_read().items()}
        m.prof_enable(False)
        assert out.loss == 0.0 and out.lm_loss == 0.0 and out.video_loss == 0.0
        return h, lg, launches

    h0, lg0, n0 = plain()
    scored = m(inputs_embeds=x, labels=seeded_labels(S, cfgd['vocab_size'], 70), informative_labels=seeded_video_labels(S, 71), relevance_labels=seeded_video_labels(S, 72))
    assert float(scored.loss) > 0
    h1, lg1, n1 = plain()
    assert torch.equal(h0, h1) and torch.equal(lg0, lg1)
    assert n0 == n1 and sum(n0.values()) > 0, (n0, n1)
