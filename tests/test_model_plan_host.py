"""What a context is built from (mmduet_amd/csrc/model_plan.h), without a GPU: tests/model_plan_shim.cpp is compiled with the host C++ compiler into a temporary directory,
loaded with ctypes, and asked for the dimensions, the weight plan and the workspace plan of every configuration of tests/model_plan_cases.py.  The names against the golden
checkpoints, the fused shapes, mmd_weight_bytes, the workspace sizes and mmd_create's refusals against restatements written out here; the refusals of finalize and the
release order against the plan's own order."""
import ctypes as C
import json
import os
import shutil
import subprocess
import pytest

import model_plan_cases as M
from mmduet_amd._lib import MmdConfig

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler')

ALIAS, CAT_ROWS, INTERLEAVE16, PAD_COLS, PAD_ROWS, SPLIT_QKV = range(6)
PACK_NONE, PACK_KEEP, PACK_RELEASE = range(3)
IN_CTX, IN_LLM_LAYER, IN_VIT_LAYER = range(3)


def up(a, b):
    return -(-a // b) * b


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('model_plan') / 'model_plan_shim.so')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', os.path.join(HERE, 'model_plan_shim.cpp'), '-o', so], check=True)
    return C.CDLL(so)


def struct_of(cfg, struct_size=0):
    assert {n for n, _ in MmdConfig._fields_} == set(M.FIELDS) | {'struct_size'}          # the table fills every field of the ABI's struct
    s = MmdConfig(**cfg)
    s.struct_size = C.sizeof(MmdConfig) + struct_size
    return s


@pytest.fixture(scope='module')
def plan(shim):
    def ask(cfg, **over):
        over = dict(over)
        s = struct_of({**cfg, **{k: v for k, v in over.items() if k != 'struct_size'}}, over.get('struct_size', 0))
        n = shim.model_plan_shim_dump(C.byref(s), M.STEP_STATE_BYTES, None, 0)
        buf = C.create_string_buffer(n + 1)
        assert shim.model_plan_shim_dump(C.byref(s), M.STEP_STATE_BYTES, buf, n + 1) == n
        return json.loads(buf.value.decode())
    return ask


@pytest.fixture(scope='module')
def check(shim):
    def ask(cfg, loaded):
        s = struct_of(cfg)
        names = (C.c_char_p * max(1, len(loaded)))(*[k.encode() for k in loaded])
        numels = (C.c_longlong * max(1, len(loaded)))(*loaded.values())
        err = C.create_string_buffer(256)
        rc = shim.model_plan_shim_check(C.byref(s), names, numels, len(loaded), err, len(err))
        return rc, err.value.decode()
    return ask


def canon(shim, name):
    out = C.create_string_buffer(256)
    shim.model_plan_shim_canon(name.encode(), out, len(out))
    return out.value.decode()


def sources(p):
    return [(name, n) for w in p['weights'] for name, n in w['src']]


CASE_IDS = list(M.CASES)


# ---- names ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASE_IDS)
def test_every_source_is_consumed_exactly_once(plan, case):
    p = plan(M.CASES[case])
    assert p['rc'] == M.MMD_OK, p['error']
    names = [n for n, _ in sources(p)]
    assert names and len(set(names)) == len(names)
    fields = [(w['scope'], w['layer'], f) for w in p['weights'] for f in (w['field'], w['field2']) if f]
    assert len(set(fields)) == len(fields)          # ... and every destination is written once


def test_canon_name(shim):
    assert canon(shim, 'model.vision_tower.vision_tower.vision_model.encoder.layers.3.mlp.fc1.bias') == 'vit.encoder.layers.3.mlp.fc1.bias'
    assert canon(shim, 'model.vision_tower.vision_tower.embeddings.patch_embedding.weight') == 'vit.embeddings.patch_embedding.weight'
    for same in ('vit.head.probe', 'model.layers.0.mlp.up_proj.weight', 'lm_head.weight', 'vision_encoder.vision_tower.post_layernorm.bias', 'model.vision_tower.other'):
        assert canon(shim, same) == same


@pytest.mark.parametrize('tag', ['A', 'B'])
def test_the_golden_checkpoints_are_what_the_plan_consumes(shim, plan, check, tag):
    cfg = M.CASES['cfg' + tag]
    _, sizes = M.golden(tag)
    loaded = {canon(shim, k): n for k, n in sizes.items()}
    assert len(loaded) == len(sizes)
    consumed = dict(sources(plan(cfg)))
    rest = set(loaded) - set(consumed)
    assert set(consumed) <= set(loaded) and {k: loaded[k] for k in consumed} == consumed
    assert rest and all(M.dropped(k, cfg) for k in rest), sorted(k for k in rest if not M.dropped(k, cfg))
    assert not any(M.dropped(k, cfg) for k in consumed)
    assert check(cfg, loaded) == (M.MMD_OK, '')


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------------------------------
def expected_shapes(g, d):
    """field -> (op, [N, K], pack, zero-filled) of the fused layouts, restated: q|k|v rows, 2 I interleaved rows, vit_kpad columns, vit_ipad rows / columns"""
    H, I, V, C_, CI = g['hidden_size'], g['intermediate_size'], g['vocab_size'], g['vit_hidden'], g['vit_intermediate']
    q, kv = g['num_heads'] * g['head_dim'], g['num_kv_heads'] * g['head_dim']
    out = {}
    if not g['vision_only']:
        out.update({(IN_CTX, 0, 'embed'): (ALIAS, [V, H], PACK_NONE, 0), (IN_CTX, 0, 'lm_head'): (ALIAS, [V, H], PACK_KEEP, 0), (IN_CTX, 0, 'heads4'): (CAT_ROWS, [4, H], PACK_NONE, 1),
                    (IN_CTX, 0, 'p0w'): (ALIAS, [H, C_], PACK_KEEP, 0), (IN_CTX, 0, 'p2w'): (ALIAS, [H, H], PACK_KEEP, 0)})
        for i in range(g['num_layers']):
            out.update({(IN_LLM_LAYER, i, 'wqkv'): (CAT_ROWS, [q + 2 * kv, H], PACK_RELEASE, 0), (IN_LLM_LAYER, i, 'bqkv'): (CAT_ROWS, [q + 2 * kv, 1], PACK_NONE, 0),
                        (IN_LLM_LAYER, i, 'wo'): (ALIAS, [H, q], PACK_RELEASE, 0), (IN_LLM_LAYER, i, 'wgu'): (INTERLEAVE16, [2 * I, H], PACK_RELEASE, 0),
                        (IN_LLM_LAYER, i, 'wdown'): (ALIAS, [H, I], PACK_RELEASE, 0)})
    kpad, ipad = up(3 * g['vit_patch'] ** 2, 64), up(CI, 64)
    assert (d['vit_kpad'], d['vit_ipad']) == (kpad, ipad)
    out[(IN_CTX, 0, 'patch_w')] = (PAD_COLS, [C_, kpad], PACK_KEEP, 0)
    out[(IN_CTX, 0, 'pos_emb')] = (ALIAS, [d['vit_seq'], C_], PACK_NONE, 0)
    for i in range(g['vit_layers']):
        out.update({(IN_VIT_LAYER, i, 'wqkv'): (CAT_ROWS, [3 * C_, C_], PACK_RELEASE, 0), (IN_VIT_LAYER, i, 'bqkv'): (CAT_ROWS, [3 * C_, 1], PACK_NONE, 0),
                    (IN_VIT_LAYER, i, 'wo'): (ALIAS, [C_, C_], PACK_RELEASE, 0), (IN_VIT_LAYER, i, 'w1'): (PAD_ROWS, [ipad, C_], PACK_RELEASE, 1),
                    (IN_VIT_LAYER, i, 'b1'): (PAD_ROWS, [ipad, 1], PACK_NONE, 1), (IN_VIT_LAYER, i, 'w2'): (PAD_COLS, [C_, ipad], PACK_RELEASE, 0)})
    if g['vit_pool_head']:
        out.update({(IN_CTX, 0, 'hd_wq'): (SPLIT_QKV, [C_, C_], PACK_NONE, 0), (IN_CTX, 0, 'hd_bq'): (SPLIT_QKV, [C_, 1], PACK_NONE, 0)})
    return out


@pytest.mark.parametrize('case', CASE_IDS)
def test_dimensions_and_fused_shapes(plan, case):
    g = M.CASES[case]
    p = plan(g)
    d = p['dims']
    grid = g['vit_image'] // g['vit_patch']
    assert (d['vit_grid'], d['vit_tokens'], d['vit_seq']) == (grid, grid * grid, grid * grid + g['vit_class_token'])
    assert d['qkv_w'] == (0 if g['vision_only'] else (g['num_heads'] + 2 * g['num_kv_heads']) * g['head_dim'])
    want = expected_shapes(g, d)
    got = {(w['scope'], w['layer'], w['field']): w for w in p['weights']}
    for key, (op, shape, pack, zero) in want.items():
        w = got[key]
        assert (w['op'], [w['N'], w['K']], w['pack'], w['zero']) == (op, shape, pack, zero), key
    for key, w in got.items():          # everything not restated above is a loaded tensor as it came: one source, its size, no copy
        if key not in want:
            assert w['op'] == ALIAS and w['pack'] == PACK_NONE and len(w['src']) == 1 and w['src'][0][1] == w['N'] * w['K'] and not w['fp8'] and not w['counted'], key
    for w in p['weights']:
        total = sum(n for _, n in w['src'])
        if w['op'] in (ALIAS, CAT_ROWS, INTERLEAVE16):
            assert total == w['N'] * w['K'], w['field']
        elif w['op'] == SPLIT_QKV:
            assert total == (w['N'] + w['N2']) * w['K'] and w['N2'] == 2 * w['N'] and w['field2'] == w['field'].replace('q', 'kv'), w['field']
        else:          # padded: the source fills part of the destination
            assert total <= w['N'] * w['K'] and (w['op'] == PAD_COLS or w['zero']), w['field']
        assert w['fp8'] == int(g['weight_dtype'] == M.W_FP8 and w['scope'] == IN_LLM_LAYER and w['field'] in ('wqkv', 'wo', 'wgu', 'wdown')), w['field']
    if g['vit_pool_head']:
        assert {f for s, _, f in got if s == IN_CTX and f.startswith('hd_')} == {'hd_probe', 'hd_wq', 'hd_bq', 'hd_wo', 'hd_bo', 'hd_lnw', 'hd_lnb', 'hd_w1', 'hd_b1', 'hd_w2', 'hd_b2'}
    assert ((IN_CTX, 0, 'cls_emb') in got) == bool(g['vit_class_token']) and ((IN_CTX, 0, 'pre_w') in got) == bool(g['vit_pre_layernorm'])
    assert ((IN_CTX, 0, 'post_w') in got) == bool(g['vit_post_layernorm'])


def test_pack_and_release_on_both_sides_of_its_thresholds(shim):
    packs = lambda dt, N, K: shim.model_plan_shim_packs(dt, N, K)
    assert [packs(M.BF16, N, K) for N, K in ((64, 64), (128, 192), (3584, 18944))] == [3, 3, 3]
    assert [packs(M.BF16, N, K) for N, K in ((63, 64), (48, 64), (64, 32), (64, 96), (65, 64), (64, 65), (128, 127))] == [0, 1, 1, 1, 0, 0, 0]          # N % 16, K % 32; then % 64
    assert [packs(M.BF16, N, K) for N, K in ((16, 32), (15, 32), (16, 31), (17, 32), (16, 33))] == [1, 0, 0, 0, 0]
    assert [packs(M.F32, N, K) for N, K in ((64, 64), (16, 32))] == [0, 0]          # bf16 contexts only
    assert packs(M.BF16, 3 * 1152, 1152) == 3 and packs(M.BF16, 4352, 1152) == 3 and packs(M.BF16, 1152, 4304) == 0 and packs(M.BF16, 152064, 3584) == 3


# ---- weight_bytes ---------------------------------------------------------------------------------------------------------------------------------------------------
def closed_formula(g, d):
    """mmd_weight_bytes as mmd_finalize_weights computed it before the plan"""
    e = 4 if g['dtype'] == M.F32 else 2
    H, I, V, C_ = g['hidden_size'], g['intermediate_size'], g['vocab_size'], g['vit_hidden']
    nh_d = g['num_heads'] * g['head_dim']
    layer = d['qkv_w'] * H + H * nh_d + 3 * I * H
    wb = (2 * V * H + g['num_layers'] * layer + g['vit_layers'] * (4 * C_ * C_ + 2 * d['vit_ipad'] * C_) + C_ * d['vit_kpad'] + H * C_ + H * H) * e
    if g['weight_dtype'] == M.W_FP8:
        wb += g['num_layers'] * layer
    return wb


@pytest.mark.parametrize('case', CASE_IDS)
def test_weight_bytes_is_the_closed_formula(plan, case):
    g = M.CASES[case]
    p = plan(g)
    assert p['weight_bytes'] == closed_formula(g, p['dims'])
    e = 4 if g['dtype'] == M.F32 else 2
    assert p['weight_bytes'] == sum(w['N'] * w['K'] * (e + w['fp8']) for w in p['weights'] if w['counted']) + p['phantom_elems'] * e
    assert p['phantom_elems'] == (g['hidden_size'] * (g['vit_hidden'] + g['hidden_size']) if g['vision_only'] else 0)


def test_the_7b_model_keeps_one_copy_in_hbm(shim, plan):
    """pack_and_release's claim, '15.8 GB instead of 31 GB for the 7B model', within the terms the formula counts: the counted matrices are 16.06e9 bytes (14.96 GiB, the formula evaluated by
    hand), 1.6 % from the comment's rounded figure; those whose row-major original stays next to the packed copy (lm_head, the projector, the patch embedding) are 1.13e9 of them"""
    g = M.CASES['true_7b']
    p = plan(g)
    counted = [w for w in p['weights'] if w['counted']]
    size = lambda w: w['N'] * w['K'] * 2
    released = [w for w in counted if w['pack'] == PACK_RELEASE and shim.model_plan_shim_packs(M.BF16, w['N'], w['K']) == 3]
    twice = [w for w in counted if w['pack'] == PACK_KEEP and shim.model_plan_shim_packs(M.BF16, w['N'], w['K']) & 1]
    assert p['weight_bytes'] == sum(map(size, counted)) == 16_063_430_656
    assert {w['field'] for w in released} == {'wqkv', 'wo', 'wgu', 'wdown', 'w1', 'w2'} and {w['field'] for w in twice} == {'lm_head', 'patch_w', 'p0w', 'p2w'}
    resident = p['weight_bytes'] + sum(map(size, twice))
    assert abs(p['weight_bytes'] - 15.8e9) <= 0.02 * 15.8e9 and 2 * p['weight_bytes'] >= 31e9 and resident - p['weight_bytes'] == 1_125_416_960


# ---- configuration refusals -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,base,over,message', M.REFUSED, ids=[r[0] for r in M.REFUSED])
def test_configurations_mmd_create_refuses(plan, name, base, over, message):
    assert plan(M.CASES[base])['rc'] == M.MMD_OK
    p = plan(M.CASES[base], **over)
    assert (p['rc'], p['error']) == (M.MMD_EINVAL, message) and 'dims' not in p


@pytest.mark.parametrize('name,base,over', M.ACCEPTED, ids=[r[0] for r in M.ACCEPTED])
def test_their_valid_neighbours_are_accepted(plan, name, base, over):
    p = plan(M.CASES[base], **over)
    assert (p['rc'], p['error']) == (M.MMD_OK, '')


def test_a_null_configuration(shim):
    buf = C.create_string_buffer(256)
    shim.model_plan_shim_dump(None, M.STEP_STATE_BYTES, buf, len(buf))
    assert json.loads(buf.value.decode()) == {'rc': M.MMD_EINVAL, 'error': 'null argument'}


def test_every_message_of_the_ladder_is_in_the_table():
    assert {r[3] for r in M.REFUSED} == {'mmd_config size mismatch (ABI)', 'unsupported dtype', 'weight_dtype fp8_e4m3 needs a bf16 context', 'unsupported head configuration',
                                         'unsupported ViT head configuration', M.TOWER_FORM, M.TOWER_RANGE}


# ---- plan refusals --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['cfgA', 'cfgB_fp8', 'clip', 'pool_head', 'small_tower_f16_1'])
def test_missing_and_missized_tensors_name_the_first_offender(plan, check, case):
    g = M.CASES[case]
    order = sources(plan(g))
    loaded = dict(order)
    assert check(g, loaded) == (M.MMD_OK, '')
    assert check(g, {**loaded, 'model.image_newline': 7}) == (M.MMD_OK, '')          # a tensor the plan does not name is not its business
    picks = sorted({0, 1, len(order) // 3, len(order) // 2, len(order) - 2, len(order) - 1})
    for i in picks:
        name, n = order[i]
        assert check(g, {k: v for k, v in loaded.items() if k != name}) == (M.MMD_ENOENT, f"missing weight tensor '{name}'")
        assert check(g, {**loaded, name: n + 1}) == (M.MMD_EINVAL, f"weight '{name}' has {n + 1} elements, expected {n}")
    for i, j in zip(picks, picks[1:]):          # two offenders: the one the plan takes first
        (a, na), (b, _) = order[i], order[j]
        assert check(g, {k: v for k, v in loaded.items() if k not in (a, b)}) == (M.MMD_ENOENT, f"missing weight tensor '{a}'")
        assert check(g, {k: v for k, v in {**loaded, a: na + 5}.items() if k != b}) == (M.MMD_EINVAL, f"weight '{a}' has {na + 5} elements, expected {na}")
    assert check(g, {}) == (M.MMD_ENOENT, f"missing weight tensor '{order[0][0]}'")


def test_the_order_of_the_takes(plan):
    """the order mmd_finalize_weights took its tensors in before the plan: head of the decoder, its layers, the tower's embeddings, its layers, post-LN, projector, pooling head"""
    names = [n for n, _ in sources(plan(M.CASES['cfgA']))]
    L0 = ['input_layernorm.weight', 'post_attention_layernorm.weight', 'self_attn.q_proj.weight', 'self_attn.k_proj.weight', 'self_attn.v_proj.weight', 'self_attn.q_proj.bias',
          'self_attn.k_proj.bias', 'self_attn.v_proj.bias', 'self_attn.o_proj.weight', 'mlp.gate_proj.weight', 'mlp.up_proj.weight', 'mlp.down_proj.weight']
    V0 = ['layer_norm1.weight', 'layer_norm1.bias', 'layer_norm2.weight', 'layer_norm2.bias', 'self_attn.q_proj.weight', 'self_attn.k_proj.weight', 'self_attn.v_proj.weight',
          'self_attn.q_proj.bias', 'self_attn.k_proj.bias', 'self_attn.v_proj.bias', 'self_attn.out_proj.weight', 'self_attn.out_proj.bias', 'mlp.fc1.weight', 'mlp.fc1.bias',
          'mlp.fc2.weight', 'mlp.fc2.bias']
    want = ['model.embed_tokens.weight', 'model.norm.weight', 'lm_head.weight', 'informative_head.weight', 'relevance_head.weight']
    want += [f'model.layers.{i}.{n}' for i in range(2) for n in L0]
    want += ['vit.embeddings.patch_embedding.weight', 'vit.embeddings.patch_embedding.bias', 'vit.embeddings.position_embedding.weight']
    want += [f'vit.encoder.layers.{i}.{n}' for i in range(2) for n in V0]
    want += ['model.mm_projector.0.weight', 'model.mm_projector.0.bias', 'model.mm_projector.2.weight', 'model.mm_projector.2.bias']
    assert names == want
    head = [n for n, _ in sources(plan(M.CASES['pool_head']))]
    assert head[:3] == want[len(want) - 39:len(want) - 36] and head[-13:] == ['vit.post_layernorm.weight', 'vit.post_layernorm.bias'] + ['vit.head.' + n for n in (
        'probe', 'attention.in_proj_weight', 'attention.in_proj_bias', 'attention.out_proj.weight', 'attention.out_proj.bias', 'layernorm.weight', 'layernorm.bias',
        'mlp.fc1.weight', 'mlp.fc1.bias', 'mlp.fc2.weight', 'mlp.fc2.bias')]
    clip = [n for n, _ in sources(plan(M.CASES['clip']))]
    assert clip[:6] == want[len(want) - 39:len(want) - 36] + ['vit.embeddings.class_embedding', 'vit.pre_layrnorm.weight', 'vit.pre_layrnorm.bias'] and 'post_layernorm' not in ' '.join(clip)


def test_fp8_and_intermediate_size_refusals(plan, check):
    # cfgA: down_proj is [64, 160], and 160 is no multiple of 64 -- the first of a layer's four matrices fp8 cannot take, reported behind the layer's last take
    g = dict(M.CASES['cfgA'], weight_dtype=M.W_FP8)
    loaded = dict(sources(plan(g)))
    msg = 'fp8 weights need N % 16 == 0 and K % 64 == 0 (got 64 x 160)'
    assert check(g, loaded) == (M.MMD_EINVAL, msg)
    drop = lambda *names: {k: v for k, v in loaded.items() if k not in names}
    assert check(g, drop('model.layers.0.mlp.down_proj.weight')) == (M.MMD_ENOENT, "missing weight tensor 'model.layers.0.mlp.down_proj.weight'")
    assert check(g, drop('model.layers.1.input_layernorm.weight', 'vit.embeddings.patch_embedding.bias')) == (M.MMD_EINVAL, msg)
    g = dict(M.CASES['cfgB_fp8'], head_dim=36)          # q|k|v: 216 rows, the first offender of four
    assert check(g, dict(sources(plan(g)))) == (M.MMD_EINVAL, 'fp8 weights need N % 16 == 0 and K % 64 == 0 (got 216 x 128)')
    assert check(M.CASES['cfgB_fp8'], dict(sources(plan(M.CASES['cfgB_fp8'])))) == (M.MMD_OK, '') and check(M.CASES['cfgA'], dict(sources(plan(M.CASES['cfgA'])))) == (M.MMD_OK, '')
    # intermediate_size: refused where gate | up are fused, in front of down_proj's take
    for I, ok in ((160, True), (168, False), (176, True), (161, False)):
        g = dict(M.CASES['cfgA'], intermediate_size=I)
        loaded = dict(sources(plan(g)))
        want = (M.MMD_OK, '') if ok else (M.MMD_EINVAL, f'intermediate_size must be a multiple of 16 (got {I})')
        assert check(g, loaded) == want
        if not ok:
            assert check(g, {k: v for k, v in loaded.items() if k != 'model.layers.0.mlp.down_proj.weight'}) == want
            assert check(g, {k: v for k, v in loaded.items() if k != 'model.layers.0.mlp.up_proj.weight'})[0] == M.MMD_ENOENT


# ---- workspaces -----------------------------------------------------------------------------------------------------------------------------------------------------
def expected_workspaces(g, d):
    """alloc_workspaces before the plan, restated: [(field, bytes, pinned)] in its order"""
    e = 4 if g['dtype'] == M.F32 else 2
    C_, H, Bm = g['vit_hidden'], g['hidden_size'], g['max_vit_batch']
    Mv = up(Bm * d['vit_seq'], 128)
    ws = [('v_col', Mv * d['vit_kpad'] * e, 0), ('v_h', Mv * C_ * e, 0), ('v_xn', Mv * C_ * e, 0)]
    if g['tower_f16'] == 1:
        pout = -(-d['vit_grid'] // g['pool_stride'])
        ws.append(('v_h32', (Mv + Bm * 4 * pout * pout) * C_ * 4, 0))
    ws += [('v_qkv', Mv * 3 * C_ * e, 0), ('v_attn', Mv * C_ * e, 0), ('v_mlp', up(Mv, 16) * d['vit_ipad'] * e, 0)]
    if g['vit_class_token']:
        ws.append(('v_patch', Mv * C_ * e, 0))
    ws += [('v_splitk_ws', 32 << 20, 0), ('v_attn_ws', 32 << 20, 0)]
    if g['vit_pool_head']:
        ws += [('hd_q', C_ * e, 0), ('hd_kv', Mv * 2 * C_ * e, 0), ('hd_a', Bm * C_ * e, 0), ('hd_h', Bm * C_ * e, 0), ('hd_n', Bm * C_ * e, 0), ('hd_m', Bm * g['vit_intermediate'] * e, 0)]
    if g['vision_only']:
        return ws
    S = up(g['max_step_tokens'], 128)
    qw = g['num_heads'] * g['head_dim']
    state = M.STEP_STATE_BYTES
    ws += [('v_p1', Mv * H * e, 0), ('v_p2', Mv * H * e, 0), ('l_h', S * H * e, 0), ('l_xn', S * H * e, 0), ('l_qkv', S * d['qkv_w'] * e, 0), ('l_q', S * qw * e, 0),
           ('l_attn', S * qw * e, 0), ('l_act', up(S, 16) * g['intermediate_size'] * e, 0), ('l_hid', S * H * e, 0),
           ('splitk_ws', (192 if g['max_step_tokens'] > 2048 else 64) << 20, 0), ('chain_ssq', 4 * 256 * 4, 0), ('rope_tab', S * 64 * 2 * 4, 0), ('attn_ws', 128 << 20, 0),
           ('logits_ws', g['vocab_size'] * 4, 0), ('heads_dev', S * 4 * 4, 0), ('rows_dev', S * 4, 0), ('tok_dev', 64, 0), ('argmax_scratch', 1024, 0), ('prev_dev', 16384 * 8, 0),
           ('gen_embed', H * e, 0), ('heads_host', S * 4 * 4, 1), ('rows_host', S * 4, 1), ('tok_host', 64, 1), ('step_host', state, 1), ('seg_host', 8 * 64 * state, 1),
           ('seg_dev', 8 * 64 * state, 0), ('step_dev', state, 0)]
    return ws


@pytest.mark.parametrize('case', CASE_IDS)
def test_workspaces_are_those_of_alloc_workspaces(plan, case):
    g = M.CASES[case]
    p = plan(g)
    assert [tuple(w) for w in p['workspaces']] == expected_workspaces(g, p['dims'])
    assert len({w[0] for w in p['workspaces']}) == len(p['workspaces'])
    dec = not g['vision_only']
    assert (p['v_splitk_bytes'], p['v_attn_bytes']) == (32 << 20, 32 << 20)          # what the planners are handed: the constants
    assert (p['splitk_bytes'], p['attn_bytes'], p['prev_cap']) == (((192 if g['max_step_tokens'] > 2048 else 64) << 20, 128 << 20, 16384) if dec else (0, 0, 0))
    assert p['v_h32_rows'] == (up(g['max_vit_batch'] * p['dims']['vit_seq'], 128) if g['tower_f16'] == 1 else 0)
    by = dict((w[0], w[1]) for w in p['workspaces'])
    assert by['v_splitk_ws'] == p['v_splitk_bytes'] and by['v_attn_ws'] == p['v_attn_bytes'] and by.get('splitk_ws', 0) == p['splitk_bytes'] and by.get('attn_ws', 0) == p['attn_bytes']


def test_the_capacities_are_the_named_constants(shim):
    out = (C.c_longlong * 4)()
    for tokens, mb in ((1, 64), (2048, 64), (2049, 192), (4096, 192)):
        shim.model_plan_shim_constants(tokens, out)
        assert tuple(out) == (mb << 20, 128 << 20, 32 << 20, 16384), tokens


# ---- release order --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASE_IDS)
def test_sources_are_released_before_the_next_layer_is_taken(plan, case):
    """walk the plan as finalize does: an alias keeps its tensor, every other entry's sources wait for the next release point -- none may wait across a layer's end"""
    p = plan(M.CASES[case])
    waiting, at = [], None
    for w in p['weights']:
        here = (w['scope'], w['layer'])
        if here != at:
            assert not waiting, (at, here, waiting)          # a layer (or the context's part in front of it) left nothing behind
            at = here
        if w['op'] != ALIAS:
            waiting += [n for n, _ in w['src']]
        if w['release']:
            waiting = []
    assert not waiting
    layers = {}
    for w in p['weights']:
        if w['scope'] != IN_CTX:
            layers.setdefault((w['scope'], w['layer']), []).append(w)
    assert len(layers) == M.CASES[case]['vit_layers'] + (0 if M.CASES[case]['vision_only'] else M.CASES[case]['num_layers'])
    for key, ws in layers.items():          # one template per kind of layer: the same entries in every layer, the release point at its end
        first = layers[(key[0], 0)]
        strip = lambda w: {k: v for k, v in w.items() if k not in ('layer', 'src')}
        assert [strip(w) for w in ws] == [strip(w) for w in first] and ws[-1]['release'] and [len(w['src']) for w in ws] == [len(w['src']) for w in first]
