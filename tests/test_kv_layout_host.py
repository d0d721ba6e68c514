"""CPU checks of tests/kv_layout.py: the two statements of the V layout agree, the host reference's two input forms agree, and the case lists of
tests/test_gpu_kv_write.py cover what they claim to cover."""
import torch
import kv_layout as L


def test_permute_and_formula_agree_on_every_slot_of_three_blocks():
    nkv, d, n = 2, 32, 3 * L.BLK
    raw = torch.arange(nkv * n * d, dtype=torch.int64).view(nkv, n // L.BLK, d, L.BLK)
    log = L.v_logical(raw)
    flat = raw.reshape(nkv, -1)
    for t in range(n):
        for e in range(d):
            assert log[1, t, e] == flat[1, L.v_index(t, e, d)], (t, e)
    assert sorted(L.v_index(t, e, d) for t in range(n) for e in range(d)) == list(range(n * d))          # a bijection onto the row
    assert torch.equal(L.v_raw(log), raw)


def test_one_slab_and_zero_bias_is_the_plain_qkv_form():
    nh, nkv, d, S, pos0 = 4, 2, 32, 9, 61
    g = torch.Generator().manual_seed(0)
    w = (nh + 2 * nkv) * d
    slab = torch.randn(1, S, w, generator=g)
    fr = L.inv_freq(d)
    a = L.ref_kv_write(slab, torch.zeros(w, dtype=torch.bfloat16), fr, pos0, nh, nkv, d, torch.bfloat16)
    b = L.ref_kv_write(slab[0].to(torch.bfloat16), None, fr, pos0, nh, nkv, d, torch.bfloat16)
    for x, y in zip(a, b):
        assert x.dtype == torch.bfloat16 and torch.equal(x, y)
    # and the slab sum really is sequential fp32: three slabs that round differently when summed in another order
    s3 = torch.tensor([1.0, 2.0 ** -24, -1.0]).view(3, 1, 1).expand(3, 1, w).contiguous()
    assert torch.equal(L.qkv_from_slabs(s3, torch.zeros(w, dtype=torch.bfloat16)), torch.zeros(1, w, dtype=torch.bfloat16))


def test_rope_reference_rounds_each_product_then_the_sum():
    d, pos0 = 8, 5
    fr = L.inv_freq(d)
    x = torch.randn(1, 3 * d, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    q, k, v = L.ref_kv_write(x, None, fr, pos0, 1, 1, d, torch.bfloat16)
    ang = torch.tensor(float(pos0)) * fr
    c, s = ang.cos().to(torch.bfloat16).float(), ang.sin().to(torch.bfloat16).float()
    x1, x2 = x[0, :d // 2].float(), x[0, d // 2:d].float()
    rb = lambda t: t.to(torch.bfloat16).float()
    assert torch.equal(q[0, :d // 2].float(), rb(rb(x1 * c) + rb(-x2 * s)))
    assert torch.equal(q[0, d // 2:].float(), rb(rb(x2 * c) + rb(x1 * s)))
    assert torch.equal(v[0, 0], x[0, 2 * d:])


def test_case_lists_cover_every_residue_and_both_sides_of_a_block_edge():
    starts = {p % 8 for p, _ in L.POS_S}
    ends = {(p + s) % 8 for p, s in L.POS_S}
    assert starts == set(range(8)) and ends == set(range(8))
    assert {p % 64 for p, _ in L.POS_S} >= {0, 1, 63} and {(p + s) % 64 for p, s in L.POS_S} >= {0, 1, 63}          # first / last token on either side of an edge
    assert any(p // 64 != (p + s - 1) // 64 for p, s in L.POS_S if s < 8)                                              # a short step across an edge
    assert any((p + s - 1) // 64 - p // 64 >= 2 for p, s in L.POS_S)                                                   # a whole block in the middle
    assert any(s >= 64 for _, s in L.POS_S) and any(s < 64 for _, s in L.POS_S)                                        # both sides of the model's chunk_rope threshold
    required = [(0, 1), (0, 64), (1, 7), (7, 9), (56, 8), (57, 7), (57, 8), (63, 1), (63, 2), (64, 1), (60, 70), (5, 130), (127, 130), (4095, 66), (70000, 49)]
    assert all(c in L.POS_S for c in required)
    cases = L.write_cases()
    for nh, nkv, d in L.HEADS:
        mine = [c for c in cases if c[:3] == (nh, nkv, d)]
        assert {c[5] for c in mine} == set(L.SLAB_COUNTS)
        assert {(c[3], c[4]) for c in mine} == {ps for ps in L.POS_S if ps[0] < L.BIG_POS or nkv == 4}
    assert all(L.cap_for(c[3], c[4]) <= 4352 or (c[3] == L.BIG_POS and c[1] == 4 and L.cap_for(c[3], c[4]) == 70144) for c in cases)
    dec = L.decode_cases()
    assert {(c[3], c[4]) for c in dec} == {(p, s) for p in L.DECODE_POS for s in L.DECODE_S}
    for nh, nkv, d in L.HEADS:
        assert {c[5] for c in dec if c[:3] == (nh, nkv, d)} == {1, 3, 4}
        assert all(c[4] * (nh // nkv) <= 16 for c in dec)
    # decode cuts the keys into at most 64 splits of whole 64-key tiles: positions on the first and the last slot of a split, for one and for several tiles per split
    for pos0 in (63, 64, 127, 128, 4095, 4096):
        tiles = (pos0 + 1 + 63) // 64
        per = -(-tiles // min(64, tiles)) * 64
        assert pos0 % per in (0, per - 1), (pos0, per)
