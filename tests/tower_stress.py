"""Vision-tower inputs with the statistics of a real SigLIP-so400m checkpoint (plain builders; imports without a GPU).

The tower tests of tests/test_gpu_production.py feed randn pixels through synthetic_weights(scale='unit'): every activation, score and GELU argument is O(1).
stress_tower_weights(w, cfg, pattern) takes that weight dict and returns a copy whose TOWER tensors are changed so that the fp32 oracle shows one named statistic
(tests/test_tower_stress_host.py checks each one at the true width; tests/test_gpu_tower_stress.py runs the product on them in every tower mode):

  outlier_channels   residual channels OUTLIER_CH carry +-10^3 .. 10^4 at the last layer (seeded by the position table, fed in every sublayer by the out_proj / fc2
                     bias of the channel -- the steady growth -- and by its weight row scaled x 8 -- a per-token part), max|h| < 100 on every other channel;
  register_tokens    three tokens carry REG_AMP on channel REG_CH of the position table; every layer's k_proj column REG_CH turns that into a key component along a
                     per-head unit vector u and the q_proj bias REG_Q u reads it: scaled scores of +30 .. +80 on those three keys for every query row of every head,
                     O(1) on the others, so every row puts >= 1 - 1e-3 of its mass on them.  Token 1 is grid (0, 0); token 2 lies on the outermost ring the bilinear
                     pool reads (first tap row, last tap column); token 3 is one the pool never reads, in the last grid row (key 714: inside the last, 25-wide
                     key tile) -- its key still reaches every query of the sparse last layer;
  gelu_saturation    fc1 pre-activations of 6 <= |x| <= 50 on both signs in 384 columns per layer (256 by their bias, 128 by a weight row scaled x 12);
  half_range         (fp16 towers) channel HALF_CH of the LAST layer's fc2 output lands at HALF_BASE = 45 056 (3e4 .. 6e4: one fp16 ulp is 32, one bf16 ulp 256);
  half_overflow      (fp16 towers) the same, and in the one frame of stress_pixels that carries a constant offset the channel passes 65 520 in the fp32 oracle
                     -- fp16(v) is inf there, as torch's half gives it, not 65 504: HALF_COLS fc1 columns read the direction a constant pixel offset leaves in the
                     LayerNorm output (the row sums of the patch embedding), and fc2's row HALF_CH reads those columns.

No tap of the true geometry clamps.  F.interpolate(bilinear, align_corners=False) clamps a tap only where (o + 0.5) g / out - 0.5 leaves [0, g - 1], i.e. only for
out >= g; the 27 -> 7 pool reads rows / columns {1, 2, 5, 6, 9, 10, 13, 14, 16, 17, 20, 21, 24, 25} (196 distinct tokens, none twice; 14 with weight exactly 0), and the
4 -> 2 pool of the golden models {0, 1, 2, 3}.  "The border taps" of this suite are therefore the outermost ring the pool reads (rows / columns 1 and 25) and the
weight-0 partners (row / column 14); pool_geometry() returns them and the host test pins the fact."""
import math
import numpy as np
import torch
from oracle import duet_oracle as O

VT = O.VT
PATTERNS = ('outlier_channels', 'register_tokens', 'gelu_saturation', 'half_range', 'half_overflow')
HALF_ONLY = ('half_range', 'half_overflow')
# mode -> (model dtype, config.tower_dtype)
MODES = {'fp32': (torch.float32, None), 'bf16': (torch.bfloat16, 'bf16'), 'fp16': (torch.bfloat16, 'fp16'), 'fp16_resid16': (torch.bfloat16, 'fp16_resid16')}

OUTLIER_CH = (7, 700)
OUTLIER_SEED = (1500.0, -1000.0)          # position table
OUTLIER_STEP = (900.0, -700.0)            # out_proj / fc2 bias of the channel, every sublayer: 1500 + 4 x 900 = 5100, -1000 - 4 x 700 = -3800 after two layers
OUTLIER_ROW_GAIN = 8.0
REG_CH = 300
REG_AMP = 1000.0
REG_Q = 15.0                              # |q_proj bias| along u;  score = REG_Q x_norm[REG_CH] / sqrt(d) = 15 * 31.4 / 8.49 ~ 55 (x_norm: 1000 over a row rms of 31.8)
SAT_BIAS = (10.0, 44.0)
SAT_ROW_GAIN = 12.0
HALF_CH = 500
HALF_BASE = 45056.0                       # (a bf16 value)
HALF_COLS = 8
HALF_ALPHA = 25.0                         # fc1 pre-activation of the HALF_COLS columns in the offset frame
HALF_BETA = 190.0                         # fc2.weight[HALF_CH, col]: 8 x 190 x gelu(~24) ~ 36 000 on top of HALF_BASE
BRIGHT_FRAME = 1
BRIGHT_OFFSET = 3.0


def tower_names(w):
    return [k for k in w if k.startswith(VT)]


def pool_geometry(cfg):
    """(taps per axis [(i0, i1, lam)], compact token list in gather_pool_rows_kernel's order u = (2 oy + ty) 2 out + 2 ox + tx, sorted tap indices of one axis)"""
    g = cfg.vit_grid
    out = math.ceil(g / cfg.video_pooling_stride)
    taps = O.bilinear_taps(g, out)
    compact = []
    for ry in range(2 * out):
        for rx in range(2 * out):
            compact.append(taps[ry >> 1][ry & 1] * g + taps[rx >> 1][rx & 1])
    return taps, compact, sorted({t[k] for t in taps for k in (0, 1)})


def register_tokens(cfg):
    taps, compact, axis = pool_geometry(cfg)
    g = cfg.vit_grid
    unread = sorted(set(range(g)) - set(axis))
    t1 = 0
    t2 = axis[0] * g + axis[-1]
    t3 = unread[-1] * g + unread[len(unread) // 2]          # the last grid row: inside the last, partly filled 64-key tile of the attention kernels
    assert t1 not in compact and t2 in compact and t3 not in compact
    return [t1, t2, t3]


def pooled_rows_reading(cfg, tokens):
    """pooled rows oy * out + ox (of one frame) whose 2 x 2 taps include one of `tokens`"""
    taps, _, _ = pool_geometry(cfg)
    g, out = cfg.vit_grid, len(taps)
    rows = []
    for oy in range(out):
        for ox in range(out):
            four = {taps[oy][a] * g + taps[ox][b] for a in (0, 1) for b in (0, 1)}
            if four & set(tokens):
                rows.append(oy * out + ox)
    return rows


def border_tap_tokens(cfg):
    """tokens of the outermost ring the pool reads and of its weight-0 partners (see the module docstring)"""
    taps, compact, axis = pool_geometry(cfg)
    g = cfg.vit_grid
    zero = {t[1] for t in taps if t[2] < 1e-9}
    edge = {axis[0], axis[-1]} | zero
    return sorted({t for t in compact if t // g in edge or t % g in edge})


def outlier_channels_of(pattern):
    return {'outlier_channels': list(OUTLIER_CH), 'register_tokens': [REG_CH], 'gelu_saturation': [], 'half_range': [HALF_CH], 'half_overflow': [HALF_CH]}[pattern]


def _unit_dirs(cfg, seed, device):
    """one unit vector per head, concatenated: [C]"""
    nh = cfg.vit_heads; hd = cfg.vit_hidden_size // nh
    g = torch.Generator().manual_seed(seed)
    s = (torch.randint(0, 2, (nh, hd), generator=g).float() * 2 - 1) / math.sqrt(hd)
    return s.reshape(-1).to(device)


def stress_tower_weights(w, cfg, pattern):
    """A copy of `w` (name -> tensor, as synthetic_weights(scale='unit') yields them) with the tower tensors changed as the module docstring says.  Every changed tensor
    is rounded back to the dtype it came in, so the product and every oracle see the same values."""
    assert pattern in PATTERNS, pattern
    out = dict(w)
    edit = {}

    def f(name):
        if name not in edit:
            assert name.startswith(VT), name
            edit[name] = w[name].float().clone()
        return edit[name]

    C, I, L = cfg.vit_hidden_size, cfg.vit_intermediate_size, cfg.vit_layers
    dev = w[VT + 'embeddings.position_embedding.weight'].device
    T = cfg.vit_tokens
    g = torch.Generator().manual_seed(1234 + PATTERNS.index(pattern))
    lay = lambda i: VT + f'encoder.layers.{i}.'
    if pattern == 'outlier_channels':
        pos = f(VT + 'embeddings.position_embedding.weight')
        for c, a, s in zip(OUTLIER_CH, OUTLIER_SEED, OUTLIER_STEP):
            pos[:, c] = a * (1.0 + 0.05 * torch.randn(T, generator=g).to(dev))
            for i in range(L):
                for lin in ('self_attn.out_proj', 'mlp.fc2'):
                    f(lay(i) + lin + '.weight')[c] *= OUTLIER_ROW_GAIN
                    f(lay(i) + lin + '.bias')[c] = s
    elif pattern == 'register_tokens':
        pos = f(VT + 'embeddings.position_embedding.weight')
        u = _unit_dirs(cfg, 77, dev)
        for t in register_tokens(cfg):
            pos[t, REG_CH] = REG_AMP
        for i in range(L):
            f(lay(i) + 'layer_norm1.weight')[REG_CH] = 1.0
            f(lay(i) + 'layer_norm1.bias')[REG_CH] = 0.0
            f(lay(i) + 'self_attn.k_proj.weight')[:, REG_CH] = u
            f(lay(i) + 'self_attn.q_proj.bias').add_(REG_Q * u)
    elif pattern == 'gelu_saturation':
        for i in range(L):
            perm = torch.randperm(I, generator=g)
            by_bias, by_row = perm[:256].to(dev), perm[256:384].to(dev)
            amp = torch.linspace(SAT_BIAS[0], SAT_BIAS[1], 128).repeat_interleave(2).to(dev)
            sign = torch.tensor([1.0, -1.0]).repeat(128).to(dev)
            f(lay(i) + 'mlp.fc1.bias')[by_bias] = amp * sign
            f(lay(i) + 'mlp.fc1.weight')[by_row] *= SAT_ROW_GAIN
    else:
        last = lay(L - 1)
        f(last + 'mlp.fc2.bias')[HALF_CH] = HALF_BASE          # (the row keeps its random weights: the accumulator adds an O(1) part that the ONE rounding of acc + bias sees)
        if pattern == 'half_overflow':
            # a constant pixel offset adds offset x (row sums of the patch embedding) to every token: the direction D that survives LayerNorm 2 as g2 D~ + b2
            D = w[VT + 'embeddings.patch_embedding.weight'].float().flatten(1).sum(1)
            Dn = (D - D.mean()) / D.std(unbiased=False)
            cols = torch.randperm(I, generator=g)[:HALF_COLS].to(dev)
            f(last + 'mlp.fc1.weight')[cols] = HALF_ALPHA * Dn[None] / C
            f(last + 'mlp.fc1.bias')[cols] = 0.0
            f(last + 'mlp.fc2.weight')[HALF_CH, cols] = HALF_BETA
    for name, t in edit.items():
        out[name] = t.to(w[name].dtype)
    return out


def stress_pixels(pattern, n, seed=0, device='cpu', dtype=torch.float32):
    """randn frames [n, 3, 384, 384] (generated on the host: the same on every device); under half_overflow frame BRIGHT_FRAME carries a constant offset"""
    g = torch.Generator().manual_seed(seed)
    px = torch.randn(n, 3, 384, 384, generator=g)
    if pattern == 'half_overflow':
        assert n > BRIGHT_FRAME
        px[BRIGHT_FRAME] += BRIGHT_OFFSET
    return px.to(device=device, dtype=dtype)


FRAME_KINDS = ('zeros', 'full', 'checker1', 'checker2', 'stripes')


def stress_frames(kind, n, R):
    """uint8 frames [n, 3, R, R] on which Pillow's bicubic resampler over- and undershoots and has to clip at both ends: all 0, all 255, a checkerboard of period
    1 and of period 2 pixels, 0 / 255 stripes (vertical in even frames, horizontal in odd ones; 3 pixels wide, so they beat against every resize ratio)"""
    assert kind in FRAME_KINDS, kind
    y, x = np.meshgrid(np.arange(R), np.arange(R), indexing='ij')
    fr = np.empty((n, 3, R, R), dtype=np.uint8)
    for t in range(n):
        if kind == 'zeros':
            a = np.zeros((R, R), dtype=np.uint8)
        elif kind == 'full':
            a = np.full((R, R), 255, dtype=np.uint8)
        elif kind == 'checker1':
            a = (((x + y + t) & 1) * 255).astype(np.uint8)
        elif kind == 'checker2':
            a = ((((x >> 1) + (y >> 1) + t) & 1) * 255).astype(np.uint8)
        else:
            a = ((((x if t % 2 == 0 else y) // 3) & 1) * 255).astype(np.uint8)
        for c in range(3):
            fr[t, c] = a if c != 1 else 255 - a          # the green plane inverted: the three planes are not copies of one another
    return torch.from_numpy(fr)


# ---- the fp32 oracle with its intermediates ----------------------------------------------------------------------------------------------------------------------
def trace_fp32(w, cfg, px):
    """oracle.duet_oracle.vit_forward in fp32, built from the oracle's own functions, keeping what the statistics are about.  Returns a dict:
    h [L + 1][B, T, C] (the residual stream after the embeddings and after every layer), scores [L][B, nh, T, T] (scaled), pre [L][B, T, I] (fc1 pre-activations),
    fc2 [L][B, T, C] and out_proj [L][B, T, C] (the sublayer outputs before the residual add), and `out` (== vit_forward, which the host test asserts)."""
    w = {k: w[k].float() for k in tower_names(w)}
    h = O.vit_patch_embed(w, cfg, px.float())
    tr = dict(h=[h], scores=[], pre=[], fc2=[], out_proj=[])
    nh = cfg.vit_heads
    for i in range(cfg.vit_layers):
        p = VT + f'encoder.layers.{i}.'
        x = O.layer_norm(h, w[p + 'layer_norm1.weight'], w[p + 'layer_norm1.bias'], cfg.vit_layer_norm_eps)
        B, N, C = x.shape
        hd = C // nh
        q = O.linear(x, w[p + 'self_attn.q_proj.weight'], w[p + 'self_attn.q_proj.bias']).view(B, N, nh, hd).transpose(1, 2)
        k = O.linear(x, w[p + 'self_attn.k_proj.weight'], w[p + 'self_attn.k_proj.bias']).view(B, N, nh, hd).transpose(1, 2)
        tr['scores'].append(torch.matmul(q, k.transpose(2, 3)) * (hd ** -0.5))
        a = O.vit_attention(w, cfg, p, x)
        tr['out_proj'].append(a)
        h = h + a
        x = O.layer_norm(h, w[p + 'layer_norm2.weight'], w[p + 'layer_norm2.bias'], cfg.vit_layer_norm_eps)
        pre = O.linear(x, w[p + 'mlp.fc1.weight'], w[p + 'mlp.fc1.bias'])
        tr['pre'].append(pre)
        y = O.linear(O.gelu_tanh(pre), w[p + 'mlp.fc2.weight'], w[p + 'mlp.fc2.bias'])
        tr['fc2'].append(y)
        h = h + y
        tr['h'].append(h)
    tr['out'] = h
    return tr


# ---- the bound ------------------------------------------------------------------------------------------------------------------------------------------------------
def _dist(a, b):
    return (a.double() - b.double()).abs().max().item() if a.numel() else 0.0


def grouped_distances(ours, oracle, ref, groups):
    """groups: name -> index applied as t[..., idx] (channel groups) or a tuple applied as t[idx] (row groups).  Returns name -> (d_ours, d_oracle, scale), every
    figure over the SAME group: max|ours - ref|, max|oracle - ref|, max(1, max|ref|)."""
    res = {}
    for name, idx in groups.items():
        pick = (lambda t: t[idx]) if isinstance(idx, tuple) else (lambda t: t[..., idx])
        r = pick(ref)
        if r.numel() == 0:
            continue
        res[name] = (_dist(pick(ours), r), _dist(pick(oracle), r) if oracle is not None else 0.0, max(1.0, r.double().abs().max().item()))
    return res


def bound_of(mode, d_oracle, scale):
    """the project's existing forms: the fp32 model within 1e-3 x scale of the fp32 oracle (test_secondary_encoders_at_true_width); a 16-bit tower within
    3 x (the matching-precision oracle's own distance to fp32) + 2e-2 x scale (test_tower_batch_of_35_frames_true_width).  Keyed on the mode alone."""
    return 1e-3 * scale if mode == 'fp32' else 3.0 * d_oracle + 2e-2 * scale


def channel_groups(C, outlier, device='cpu'):
    m = torch.zeros(C, dtype=torch.bool, device=device)
    if len(outlier):
        m[torch.tensor(outlier, device=device)] = True
    return {'outlier_channels': m, 'other_channels': ~m}


def embed_row_groups(cfg, n_frames, device='cpu'):
    """rows of visual_embed [n_frames * out^2, H]: those whose 2 x 2 taps include a register token, and the rest"""
    per = cfg.frame_num_tokens
    hot = pooled_rows_reading(cfg, register_tokens(cfg))
    m = torch.zeros(n_frames * per, dtype=torch.bool, device=device)
    for b in range(n_frames):
        m[torch.tensor(hot, device=device) + b * per] = True
    return {'register_rows': (m,), 'other_rows': (~m,)}
