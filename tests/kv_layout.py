"""The KV arena's layout and the host statement of what a writer stores, for tests/test_gpu_kv_write.py, tests/test_gpu_kv_arena.py and (CPU only) tests/test_kv_layout_host.py.

K is stored as rotated rows [nkv, cap, d].  V is stored in transposed 64-token blocks: token t, dim e of a head lives at ((t >> 6) * d + e) * 64 + (t & 63) of the head's
row.  The layout is stated here independently of the kernels: once as that scalar formula (v_index), once as a permute of the raw [nkv, n / 64, d, 64] view (v_logical)."""
import torch
from oracle import duet_oracle as O

BLK = 64


def v_index(t, e, d):
    """element offset of (token t, dim e) inside one kv head's V row"""
    return ((t >> 6) * d + e) * 64 + (t & 63)


def v_logical(V_raw):
    """[nkv, n / 64, d, 64] as stored -> [nkv, n, d] (a copy)"""
    nkv, nb, d, b = V_raw.shape
    assert b == BLK
    return V_raw.permute(0, 1, 3, 2).reshape(nkv, nb * BLK, d)


def v_raw(V_log):
    """[nkv, n, d] -> [nkv, n / 64, d, 64] as stored (a copy); n % 64 == 0"""
    nkv, n, d = V_log.shape
    assert n % BLK == 0
    return V_log.reshape(nkv, n // BLK, BLK, d).permute(0, 1, 3, 2).contiguous()


def inv_freq(d, theta=1e6):
    """the fp32 table the model hands to the library (transformers qwen2/modeling_qwen2.py:84-85)"""
    return 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.float32) / d))


def qkv_from_slabs(slabs, bias):
    """first stage of a slab writer: the fp32 slabs [n, S, w] summed in slab order 0, 1, 2, ..., plus the bf16 bias, rounded once -> bf16 [S, w]"""
    acc = slabs[0].float().clone()
    for z in range(1, slabs.shape[0]):
        acc = acc + slabs[z].float()
    return (acc + bias.float()[None, :]).to(torch.bfloat16)


def ref_kv_write(src, bias, inv_freq_tab, pos0, nh, nkv, d, dtype):
    """What a write of S tokens at pos0 stores.  src: qkv [S, w] (bias None; rounded to `dtype` first) or fp32 slabs [n, S, w] with a bf16 bias.
    cos / sin of the fp32 angle pos * inv_freq are rounded to the storage type; each product is rounded, then their sum (O.apply_rope in `dtype`).
    -> q [S, nh * d], k [nkv, S, d], v [nkv, S, d], all in `dtype` (v in token order: the layout is the caller's business)."""
    x = qkv_from_slabs(src, bias) if src.ndim == 3 else src.to(dtype)
    assert x.dtype == dtype
    S = x.shape[0]
    fr = torch.arange(pos0, pos0 + S).float()[:, None] * inv_freq_tab.float()[None, :]
    emb = torch.cat([fr, fr], -1)
    cos, sin = emb.cos().to(dtype), emb.sin().to(dtype)
    q = O.apply_rope(x[:, :nh * d].view(S, nh, d).transpose(0, 1), cos, sin).transpose(0, 1).reshape(S, nh * d)
    k = O.apply_rope(x[:, nh * d:(nh + nkv) * d].view(S, nkv, d).transpose(0, 1), cos, sin).contiguous()
    v = x[:, (nh + nkv) * d:].view(S, nkv, d).transpose(0, 1).contiguous()
    return q, k, v


# ---- the cases of tests/test_gpu_kv_write.py -----------------------------------------------------------------------------------------------------------------
HEADS = [(28, 4, 128), (32, 8, 128), (4, 2, 128)]          # (32, 8): 40 q + k heads, the chunk kernel's `head += 32` loop runs twice; (4, 2): fewer than 32
SMALL_HEADS = (4, 2, 32)                                   # writers 0 / 1 only, fp32 and bf16
# (pos0, S): start and end on every residue mod 8 (the chunk kernel stores 8 tokens at a time where a group lies inside the step) and on either side of a 64-token block edge
POS_S = [(0, 1), (0, 64), (1, 7), (7, 9), (56, 8), (57, 7), (57, 8), (63, 1), (63, 2), (64, 1), (60, 70), (5, 130), (127, 130), (4095, 66), (70000, 49),
         (2, 65), (3, 9), (6, 7), (58, 12), (66, 3), (62, 72), (60, 3)]
BIG_POS = 70000                                            # 72 MB per arena in bf16: nkv = 4 only
SLAB_COUNTS = [1, 3, 4, 5, 9, 16]                          # writer 3 (16 = the whole unrolled sum); writer 4 takes the first three
DECODE_POS = [0, 1, 63, 64, 127, 128, 4095, 4096, 16383]   # writer 4: decode runs 64 key splits of whole 64-key tiles, so these sit on split boundaries
DECODE_S = [1, 2]


def cap_for(pos0, S):
    """the smallest arena of whole blocks that holds the step and one more block behind it (so that `nothing written behind the step` has slots to look at)"""
    return ((pos0 + S + BLK - 1) // BLK + 1) * BLK


def write_cases():
    """(nh, nkv, d, pos0, S, n_slabs) for writers 1-3; n_slabs cycles so that every count meets every head shape"""
    out = []
    for hi, (nh, nkv, d) in enumerate(HEADS):
        for pi, (pos0, S) in enumerate(POS_S):
            if pos0 >= BIG_POS and nkv != 4:
                continue
            out.append((nh, nkv, d, pos0, S, SLAB_COUNTS[(pi + hi) % len(SLAB_COUNTS)]))
    return out


def decode_cases():
    """(nh, nkv, d, pos0, S, n_slabs) for writer 4"""
    out = []
    for hi, (nh, nkv, d) in enumerate(HEADS):
        for pi, pos0 in enumerate(DECODE_POS):
            for S in DECODE_S:
                out.append((nh, nkv, d, pos0, S, SLAB_COUNTS[(pi + hi + S) % 3]))
    return out
