"""Decoder inputs with the statistics of a real Qwen2-7B checkpoint (plain builders; imports without a GPU).

The step-schedule tests (tests/test_gpu_step_regimes.py) and the model-level parity tests (tests/test_gpu_production.py) feed 0.5 x randn rows through scale='unit'
weights: every score is O(1), attention is near uniform, and a talking row on a fresh arena attends to itself alone.  stress_llm_weights(w, cfg, pattern) takes that
weight dict (2-layer true-width decoder: H 3584, I 18944, 28 / 4 heads of 128) and returns a copy whose DECODER tensors are changed so that the fp32 oracle shows one
named statistic; tests/test_llm_stress_host.py checks each one at the true width, tests/test_gpu_llm_stress.py runs every step schedule on them over live contexts.

  sink                row 0 of a stream (stress_embeds(first=True): the "BOS" row) carries SINK_AMP on the residual channels SINK_CH, no other row does.  The k_proj
                      columns of those channels point along a per-kv-head unit vector u in the four lowest-frequency rotary pairs (inv_freq 2.4e-6 .. 1.2e-6: the
                      rotation over 4200 positions is below 0.011 rad) and the q_proj bias SINK_Q u reads it: key 0 scores SINK_SCORE for every later row of every
                      head.  A constant score on one key cannot hold a mass band for rows 1 .. 4200 beside near-uniform other keys (their mass grows with the row
                      index), so the other keys get what RoPE gives a real checkpoint: equal q / k bias components WIN_W on the 56 higher-frequency pairs add
                      WIN_C x sum_i cos(w_i D) to the score at distance D -- WIN_C x 56 on the row itself, falling by ~ 2 ln D (the count of pairs slower than 1 / D)
                      -- so the non-sink mass converges within a few keys and key 0 keeps 0.5 .. 0.99 of every later row's mass at any context length.  The random
                      q_proj / k_proj weights are scaled by QK_SHRINK, so that band holds for EVERY row and head and not merely on average; row 0's own window
                      component is cancelled through the same two k_proj columns.  The other ~ 20 % of the mass sits on the last few keys: an error there shows.
  qk_bias             q / k biases of QKB_Q / QKB_K on one mid-frequency rotary pair per kv head (pairs 22 .. 25: periods 720 .. 1400 positions), the q bias of the
                      seven query heads of a group turned by 0, 1/7, ... 6/7 of a circle: scaled scores of +-QKB_Q QKB_K / sqrt(128) = +-265 that depend on distance
                      alone; phase 0 puts the maximum on the newest keys (the LAST key split), the other phases anywhere in the context, so the running maximum
                      moves across key tiles and across splits.
  outlier_channels    every token carries |h| of 10^2 .. 10^3 on OUTLIER_CH from the first attention sublayer on: the v_proj bias OUT_VB on eight dimensions of every
                      head passes the softmax unchanged, and the o_proj rows of the three channels read it (OUT_STEP per layer, the steady growth); the down_proj rows
                      of the channels are scaled x OUT_ROW_GAIN (a per-token part).  RMSNorm gains on the channels are OUT_GAIN (5 .. 20); the columns of q / k / v /
                      gate / up that read them are scaled by OUT_COL (as a real checkpoint's are small there): max|h| < 30 on every other channel.  (The BOS row's
                      SINK_CH belong to the outlier group of every pattern: stress_embeds puts them there whatever the weights.)
  swiglu_saturation   SAT_COLS gate_proj rows per layer scaled x SAT_ROW_GAIN: gate pre-activations of 6 <= |x| <= 50 on both signs, `up` stays O(1).

The seeds the device test uses (weights, prefixes, step rows) are constants of this module, so the host test checks the very inputs the device sees."""
import math
import torch
from oracle import duet_oracle as O
from tower_stress import grouped_distances, bound_of, channel_groups          # noqa: F401  (the bound and its grouping are the tower suite's: imported, not copied)

PATTERNS = ('sink', 'qk_bias', 'outlier_channels', 'swiglu_saturation')
WEIGHT_SEED = 3
PREFIX_LENGTHS = (63, 64, 65, 127, 129, 255, 257, 330, 1000)          # both sides of a 64-key tile and of a key split
PREFIX_SEED = 100          # + the prefix length
STEP_SEED = 7000           # + a per-test offset

SINK_CH = (1415, 2158)
SINK_AMP = 2048.0
SINK_PAIRS = (60, 61, 62, 63)
SINK_Q = 8.0
QK_SHRINK = 0.1
WIN_PAIRS = 56
WIN_C = 0.45                                       # score per pair at distance 0
WIN_W = math.sqrt(WIN_C * math.sqrt(128.0))        # q and k bias component: WIN_W^2 / sqrt(d) = WIN_C
SINK_LOGIT = 1.7                                   # ln(key 0's mass / the other keys' mass) aimed at: 0.85 of the mass

QKB_PAIRS = (22, 23, 24, 25)
QKB_Q = 60.0
QKB_K = 50.0

OUTLIER_CH = (100, 1500, 3000)
OUT_VB = 3.0
OUT_VDIMS = 8
OUT_STEP = (250.0, -180.0, 320.0)
OUT_ROW_GAIN = 8.0
OUT_GAIN = (10.0, 8.0, 12.0)
OUT_COL = 0.125

SAT_COLS = 384
SAT_ROW_GAIN = 10.0

LAYER = 'model.layers.'


def oracle_config():
    return O.OracleConfig(vocab_size=2048, num_hidden_layers=2, vit_layers=1)          # every other dimension is the 7B / so400m default


def product_config(weight_dtype=None):
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=2, vit_num_hidden_layers=2, vit_layers_removed=1, frame_num_tokens=49, frame_resolution=384,
                                        v_placeholder='<image>')
    if weight_dtype:
        pcfg.weight_dtype = weight_dtype
    return pcfg


_BASE = []


def base_weights():
    """synthetic_weights(scale='unit') of the 2-layer true-width model in bf16, generated on the HOST (a device generator draws other numbers): host and device tests
    share the values.  Built once per process; nobody writes into it."""
    if not _BASE:
        from mmduet_amd.weights import synthetic_weights
        _BASE.append(dict(synthetic_weights(product_config(), seed=WEIGHT_SEED, device='cpu', dtype=torch.bfloat16, scale='unit')))
    return _BASE[0]


def decoder_names(w):
    return [k for k in w if k.startswith(LAYER) or k == 'model.norm.weight']


def outlier_channels_of(pattern):
    return sorted(SINK_CH + (OUTLIER_CH if pattern == 'outlier_channels' else ()))


def inv_freq(cfg):
    d = cfg.head_dim
    return 1.0 / (cfg.rope_theta ** (torch.arange(0, d, 2, dtype=torch.float64) / d))


def window_score(cfg, dist):
    """WIN_C x sum over the window pairs of cos(w_i D), for a tensor of distances (float64)"""
    return WIN_C * torch.cos(dist.double()[..., None] * inv_freq(cfg)[:WIN_PAIRS]).sum(-1)


def sink_score(cfg):
    """the score of key 0 that leaves it e^SINK_LOGIT times the mass of the other keys of a long context: their mass is sum_D exp(window_score(D)), converged long
    before 4096 keys"""
    z = torch.logsumexp(window_score(cfg, torch.arange(4096)), 0).item()
    return z + SINK_LOGIT


def sink_xnorm(cfg):
    """RMSNorm image (gain 1) of SINK_AMP in the BOS row: two channels at SINK_AMP among H of variance 0.25"""
    H = cfg.hidden_size
    return SINK_AMP / math.sqrt((len(SINK_CH) * SINK_AMP ** 2 + (H - len(SINK_CH)) * 0.25) / H)


def _sink_dirs(cfg, seed):
    """one unit vector per kv head over the dimensions of SINK_PAIRS: [nkv, d]"""
    nkv, d = cfg.num_key_value_heads, cfg.head_dim
    g = torch.Generator().manual_seed(seed)
    dims = [p for p in SINK_PAIRS] + [p + d // 2 for p in SINK_PAIRS]
    u = torch.zeros(nkv, d)
    u[:, dims] = (torch.randint(0, 2, (nkv, len(dims)), generator=g).float() * 2 - 1) / math.sqrt(len(dims))
    return u


def stress_llm_weights(w, cfg, pattern):
    """A copy of `w` (name -> tensor) with the decoder tensors changed as the module docstring says.  Every changed tensor is rounded back to the dtype it came in, so
    the product and every oracle see the same values; every other entry of the copy IS the input's tensor."""
    assert pattern in PATTERNS, pattern
    out = dict(w)
    edit = {}

    def f(name):
        if name not in edit:
            assert name.startswith(LAYER) or name == 'model.norm.weight', name
            edit[name] = w[name].float().clone()
        return edit[name]

    H, I, L = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
    nh, nkv, d = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    rep, half = nh // nkv, d // 2
    g = torch.Generator().manual_seed(4321 + PATTERNS.index(pattern))
    lay = lambda i: f'{LAYER}{i}.'
    if pattern == 'sink':
        u = _sink_dirs(cfg, 78)
        xn = sink_xnorm(cfg)
        a = sink_score(cfg) * math.sqrt(d) / (xn * SINK_Q)          # |key 0 along u| = a xn;  score = SINK_Q a xn / sqrt(d)
        win = torch.zeros(d); win[:WIN_PAIRS] = WIN_W
        for i in range(L):
            p = lay(i) + 'self_attn.'
            f(lay(i) + 'input_layernorm.weight')[list(SINK_CH)] = 1.0
            f(p + 'q_proj.weight').mul_(QK_SHRINK); f(p + 'k_proj.weight').mul_(QK_SHRINK)
            bq = f(p + 'q_proj.bias').zero_().view(nh, d)
            bk = f(p + 'k_proj.bias').zero_().view(nkv, d)
            bq += win[None] + SINK_Q * u.repeat_interleave(rep, 0)
            bk += win[None]
            col = (a * u - win[None] / xn) / len(SINK_CH)          # per channel: its share of the sink key, and of the cancellation of the BOS row's own window part
            for c in SINK_CH:
                f(p + 'k_proj.weight')[:, c] = col.reshape(-1)
    elif pattern == 'qk_bias':
        for i in range(L):
            p = lay(i) + 'self_attn.'
            bq, bk = f(p + 'q_proj.bias').view(nh, d), f(p + 'k_proj.bias').view(nkv, d)
            for j in range(nkv):
                pr = QKB_PAIRS[j % len(QKB_PAIRS)]
                bk[j, pr] = QKB_K; bk[j, pr + half] = 0.0
                for r in range(rep):
                    phi = 2 * math.pi * r / rep
                    bq[j * rep + r, pr] = QKB_Q * math.cos(phi); bq[j * rep + r, pr + half] = QKB_Q * math.sin(phi)
    elif pattern == 'outlier_channels':
        ch = list(OUTLIER_CH)
        vd = torch.arange(OUT_VDIMS)
        odims = (torch.arange(nh)[:, None] * d + vd[None]).reshape(-1)          # the attention output's columns that carry the v bias
        for i in range(L):
            p = lay(i)
            f(p + 'self_attn.v_proj.bias').view(nkv, d)[:, :OUT_VDIMS] = OUT_VB
            for c, step, gain in zip(ch, OUT_STEP, OUT_GAIN):
                f(p + 'self_attn.o_proj.weight')[c, odims] = step / (OUT_VB * len(odims))
                f(p + 'mlp.down_proj.weight')[c] *= OUT_ROW_GAIN
                f(p + 'input_layernorm.weight')[c] = gain
                f(p + 'post_attention_layernorm.weight')[c] = gain
            for lin in ('self_attn.q_proj', 'self_attn.k_proj', 'self_attn.v_proj', 'mlp.gate_proj', 'mlp.up_proj'):
                f(p + lin + '.weight')[:, ch] *= OUT_COL
        for c, gain in zip(ch, OUT_GAIN):
            f('model.norm.weight')[c] = gain
    else:
        for i in range(L):
            rows = torch.randperm(I, generator=g)[:SAT_COLS]
            f(lay(i) + 'mlp.gate_proj.weight')[rows] *= SAT_ROW_GAIN
    for name, t in edit.items():
        out[name] = t.to(device=w[name].device, dtype=w[name].dtype)
    return out


def stress_embeds(cfg, S, first, seed):
    """input rows [S, H] in bf16: 0.5 x randn (generated on the host: the same on every device); first=True makes row 0 the stream's BOS row, SINK_AMP on SINK_CH"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, cfg.hidden_size, generator=g) * 0.5
    if first:
        x[0, list(SINK_CH)] = SINK_AMP
    return x.to(torch.bfloat16)


def prefix_embeds(cfg, n):
    return stress_embeds(cfg, n, True, PREFIX_SEED + n)


# ---- the fp32 oracle with its intermediates ----------------------------------------------------------------------------------------------------------------------
def trace_fp32(w, cfg, x):
    """oracle.duet_oracle.llm_forward in fp32 over one stream from an empty context, restated from the oracle's own functions, keeping what the statistics are about.
    Returns a dict: scores [L][nh, S, S] (scaled, -inf above the diagonal), gate / up [L][S, I] (pre-activations), h [L + 1][S, H] (the residual stream before
    every layer and behind the last), mid [L][S, H] (behind the attention sublayer) and `out` (== llm_forward's hidden state, which the host test asserts)."""
    w = {k: w[k].float() for k in decoder_names(w)}
    h = x.float()
    S = h.shape[0]
    nh, nkv, d = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    cos, sin = O.rope_tables(cfg, torch.arange(S), h.dtype)
    tr = dict(h=[h], mid=[], scores=[], gate=[], up=[])
    for i in range(cfg.num_hidden_layers):
        p = f'{LAYER}{i}.'
        r = h
        xn = O.rms_norm(h, w[p + 'input_layernorm.weight'], cfg.rms_norm_eps)
        q = O.linear(xn, w[p + 'self_attn.q_proj.weight'], w[p + 'self_attn.q_proj.bias']).view(S, nh, d).transpose(0, 1)
        k = O.linear(xn, w[p + 'self_attn.k_proj.weight'], w[p + 'self_attn.k_proj.bias']).view(S, nkv, d).transpose(0, 1)
        v = O.linear(xn, w[p + 'self_attn.v_proj.weight'], w[p + 'self_attn.v_proj.bias']).view(S, nkv, d).transpose(0, 1)
        q, k = O.apply_rope(q, cos, sin), O.apply_rope(k, cos, sin)
        rep = nh // nkv
        kk = k[:, None].expand(nkv, rep, S, d).reshape(nh, S, d)
        vv = v[:, None].expand(nkv, rep, S, d).reshape(nh, S, d)
        s = torch.matmul(q, kk.transpose(1, 2)) * (d ** -0.5)
        pos = torch.arange(S)
        s = s.masked_fill((pos[None, :] > pos[:, None])[None], float('-inf'))
        tr['scores'].append(s)
        a = torch.softmax(s, dim=-1, dtype=torch.float32)
        o = torch.matmul(a, vv).transpose(0, 1).reshape(S, nh * d)
        h = r + O.linear(o, w[p + 'self_attn.o_proj.weight'])
        tr['mid'].append(h)
        r = h
        xn = O.rms_norm(h, w[p + 'post_attention_layernorm.weight'], cfg.rms_norm_eps)
        gate = O.linear(xn, w[p + 'mlp.gate_proj.weight'])
        up = O.linear(xn, w[p + 'mlp.up_proj.weight'])
        tr['gate'].append(gate); tr['up'].append(up)
        h = r + O.linear(torch.nn.functional.silu(gate) * up, w[p + 'mlp.down_proj.weight'])
        tr['h'].append(h)
    tr['out'] = O.rms_norm(h, w['model.norm.weight'], cfg.rms_norm_eps)
    return tr


def tail_scores_fp32(w, cfg, x, n_tail, chunk=1050):
    """scaled scores [L][nh, n_tail, S] of the last n_tail rows of one stream over ALL its keys in the fp32 oracle, without the S x S score matrix of trace_fp32: the
    rows in front go through oracle.duet_oracle.llm_forward in chunks (its KV is the context), the tail rows through the layer restated as in trace_fp32"""
    w = {k: w[k].float() for k in decoder_names(w)}
    S = x.shape[0]
    n = S - n_tail
    past = None
    for s0 in range(0, n, chunk):
        _, past = O.llm_forward(w, cfg, x[s0:min(n, s0 + chunk)].float(), past)
    h = x[n:].float()
    nh, nkv, d = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    rep = nh // nkv
    cos, sin = O.rope_tables(cfg, torch.arange(n, S), h.dtype)
    out = []
    for i in range(cfg.num_hidden_layers):
        p = f'{LAYER}{i}.'
        xn = O.rms_norm(h, w[p + 'input_layernorm.weight'], cfg.rms_norm_eps)
        q = O.linear(xn, w[p + 'self_attn.q_proj.weight'], w[p + 'self_attn.q_proj.bias']).view(n_tail, nh, d).transpose(0, 1)
        k = O.linear(xn, w[p + 'self_attn.k_proj.weight'], w[p + 'self_attn.k_proj.bias']).view(n_tail, nkv, d).transpose(0, 1)
        q, k = O.apply_rope(q, cos, sin), O.apply_rope(k, cos, sin)
        kk = torch.cat([past.k[i], k], 1)[:, None].expand(nkv, rep, S, d).reshape(nh, S, d)
        s = torch.matmul(q, kk.transpose(1, 2)) * (d ** -0.5)
        s = s.masked_fill((torch.arange(S)[None, :] > torch.arange(n, S)[:, None])[None], float('-inf'))
        out.append(s)
        h, _, _ = O.llm_layer(w, cfg, i, h, cos, sin, past.k[i], past.v[i])
    return out
