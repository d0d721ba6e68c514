"""The step regime table (tests/step_regimes.py) on the device: every row a bf16 context takes eagerly is run on the 2-layer true-width model, and
`step_last_plan()` -- the plan llm_step_segs launched from -- must equal the table's.  The switch rows run in a context created under their environment (mmd_create reads
the switches), so a switch that is misread, or not read, fails here.  (tests/test_step_plan_host.py checks every row, the other contexts included, against step_plan() on
the host.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu
import step_regimes as T


@pytest.fixture(scope='module')
def models():
    """env -> model: one set of weights, one context per environment of the table (created at first use, under that environment)"""
    from oracle import duet_oracle as O
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    ocfg = O.OracleConfig(vocab_size=2048, num_hidden_layers=2, vit_layers=1)          # every other dimension is the 7B / so400m default
    w = O.random_weights(ocfg, seed=3, dtype=torch.bfloat16, scale='unit')
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=2, vit_num_hidden_layers=2, vit_layers_removed=1,
                                        frame_num_tokens=49, frame_resolution=384, v_placeholder='<image>')
    made = {}

    def get(env):
        key = tuple(sorted(env.items()))
        if key not in made:
            with pytest.MonkeyPatch.context() as mp:
                for k in T.SWITCHES:
                    mp.delenv(k, raising=False)
                for k, v in env.items():
                    mp.setenv(k, v)
                m = VideoHeadLiveLlavaQwenForCausalLM(pcfg, torch_dtype=torch.bfloat16, max_vit_batch=1, max_step_tokens=T.MAX_STEP_TOKENS, kv_initial_tokens=1024)
            m.load_state_dict(w)
            made[key] = m
        return made[key]
    return get


def run_row(m, row, g):
    """the step of a row through the public entry that reaches it: forward() (every hidden row), frame_step() (head rows), multi_step() (every stream's last row);
    each stream starts a fresh arena"""
    x = lambda n: (torch.randn(n, m.config.hidden_size, generator=g) * 0.5).to(torch.bfloat16).cuda()
    if len(row.segs) > 1:
        out = m.multi_step([dict(x=x(n), cache=None, head_rows=[], hidden='last') for n in row.segs], want_logits=False)
        assert [len(o['cache']) for o in out] == list(row.segs)
        return torch.cat([o['hidden'] for o in out]).float()
    S = row.segs[0]
    if row.hidden_out:
        return m(inputs_embeds=x(S)[None]).informative_logits.float()
    heads, cache = m.frame_step(x(S), None, list(range(S - row.need, S)))
    assert len(cache) == S
    return heads


@pytest.mark.parametrize('row', T.gpu_rows(), ids=[r.name for r in T.gpu_rows()])
def test_step_takes_the_plan_of_the_table(models, row):
    model = models(row.env)
    out = run_row(model, row, torch.Generator().manual_seed(len(row.segs) * 1000 + sum(row.segs)))
    assert tuple(model.step_last_plan()[f] for f in T.FIELDS) == row.plan, (row.name, model.step_last_plan())
    assert torch.isfinite(out).all()


def test_the_table_reaches_the_named_boundaries_on_the_device():
    names = {r.name for r in T.gpu_rows()}
    assert {'no_multi_fuse_63', 'no_multi_fuse_64', 'no_multi_fuse_65', 'no_multi_fuse_talk_1x2', 'no_multi_attn_talk_1x2', 'no_multi_attn_talk_1x16'} <= names
    assert {k for r in T.gpu_rows() for k in r.env} == set(T.SWITCHES)


def test_the_plan_is_the_contexts_most_recent_step(models):
    R = T.rows_by_name()
    g = torch.Generator().manual_seed(1)
    a, b = models({}), models({'MMDUET_NO_MULTI_ATTN': '1'})          # ... and of THIS context: another context's step does not disturb it
    for name in ('frame_700', 'fwd_1', 'talk_1x2', 'fwd_5'):
        run_row(a, R[name], g)
        assert tuple(a.step_last_plan().values()) == R[name].plan, name
    run_row(b, R['no_multi_attn_talk_1x2'], g)
    assert tuple(b.step_last_plan().values()) == R['no_multi_attn_talk_1x2'].plan and tuple(a.step_last_plan().values()) == R['fwd_5'].plan
