"""What the KV arena's writers store, bit for bit (operator level, mmd_op_kv_write on caller-owned buffers filled with a sentinel).

Writers: 0 rope_append_kernel with row-major V (control), 1 the same with V in transposed 64-token blocks, 2 rope_append_chunk_kernel over the step's (cos, sin) table,
3 slab_rope_append_kernel, 4 the q / k / v preparation inside the decode attention.  Per case:
  * footprint: every K element and V slot outside [pos0, pos0 + S) still holds the sentinel -- the rest of the partly written first and last V blocks and every other
    head's rows included -- and so do the guard rows around q_out;
  * V inside the range equals the host reference (tests/kv_layout.py ref_kv_write) bit for bit: V is a copy, or one fp32 sum and one rounding;
  * K and q are bit-identical between writers 1, 2 and 3, and K between those and writer 4, on the same inputs (the slabs' sum plus bias rounds to the qkv rows the
    others read): all of them call the device's cosf / sinf on the same fp32 angle.  Writer 4 never stores q: its q is compared through the attention output, which must
    equal -- bit for bit -- attention variant 3 over the arena writer 3 left, with writer 3's q;
  * K and q against the host reference at assert_close's bound of tests/test_gpu_ops.py (host and device cosf may differ in the last fp32 ulp).

Mutants (throw-away builds, never committed, one run each; they leave slots unwritten or overwrite sentinel slots of these tests' own buffers):
  (a) rope_append_chunk_kernel without the scalar tail `else` branch (ragged ends of a step's V never stored);
  (b) its vector-path condition `p0 + 8 <= hi` weakened to `p0 < hi` (a group of 8 that starts inside the step is stored whole: slots behind the step are clobbered);
  (c) the fused preparation's `pos >= kbeg + kv_per_split` changed to `>` (a token on the first slot of a split is also written by the block of the split before it).
What each run showed (the new files are this one and tests/test_gpu_kv_arena.py, 190 tests; of the old suite only tests/test_gpu_trueshape.py and
tests/test_gpu_multistream.py, 22 tests, were run against the mutants -- the rest of the old suite is unmeasured):
  (a) new: 125 fail -- every case of test_writers_1_2_3_store_the_same_bits_in_their_own_slots whose step has a ragged end (58), 12 cases of
      test_slab_writer_sums_every_slab_count_in_order, all 54 of test_decode_attention_prepares_the_token_it_attends_to (its writer-2 comparison) and
      test_gpu_kv_arena.py::test_tile_step_with_chunk_rope ("elements inside [pos0, pos0 + S) were never written").
      old: test_gpu_trueshape.py::test_fused_and_unfused_schedules_agree fails, the other 21 pass -- the prediction that the old suite passes (a) was wrong for that test.
  (b) new: 89 fail -- 40 cases of test_writers_1_2_3_..., 12 of test_slab_writer_..., 36 of test_decode_attention_... and test_tile_step_with_chunk_rope
      ("elements outside [pos0, pos0 + S) changed").  old: all 22 pass.
  (c) new: all 190 pass; old: all 22 pass.  The mutant is not observable in the arena: the second block writes the same token from the same slabs, hence the same bits,
      into the same slot, and it does not read that tile.  So a fourth mutant was run for the split boundary:
  (d) `pos >= kbeg + kv_per_split - 1`: the token on the LAST slot of a split is written by no block.  new: 25 fail -- the 21 cases of test_decode_attention_... at
      pos0 = 63, 127, 4095 (S = 1 and 2) and 16383 (S = 1), and in test_gpu_kv_arena.py test_decode_chain_step[63], [127],
      test_graph_replayed_generate_across_a_block_edge and test_round_of_three_talking_streams[talking].  old: all 22 pass.
With the unmodified kernels every new test passes: no test of this pull request exposed a bug in a writer, the stash or the growth paths.
"""
import math
import pytest
import torch

pytestmark = pytest.mark.gpu
import kv_layout as L
from rawops import RawOps, SENTINEL_BITS, _INT_OF, guarded, sentinel_intact
from test_gpu_ops import assert_close

MMD_EINVAL = -22
BF = torch.bfloat16


@pytest.fixture(scope='module')
def ops():
    return RawOps(BF)


@pytest.fixture(scope='module')
def ops_f32():
    return RawOps(torch.float32)


def sentinel(shape, dtype, dev):
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(_INT_OF[dtype]).fill_(SENTINEL_BITS[dtype])
    return t


def bits(t):
    return t.contiguous().view(_INT_OF[t.dtype])


def logical_v(Vc, v_tr):
    """Vc [nkv, cap, d] as the writer left it -> [nkv, cap, d] in token order"""
    nkv, cap, d = Vc.shape
    return L.v_logical(Vc.view(nkv, cap // L.BLK, d, L.BLK)) if v_tr else Vc


def assert_footprint(Kc, Vl, base_K, base_Vl, pos0, S, what):
    """outside [pos0, pos0 + S) Kc / Vl (token order) hold exactly the bits of base_* (None: the sentinel); inside, no sentinel is left"""
    sb = SENTINEL_BITS[Kc.dtype]
    for name, t, base in (('K', Kc, base_K), ('V', Vl, base_Vl)):
        ti = t.view(_INT_OF[t.dtype])
        for lo, hi in ((0, pos0), (pos0 + S, t.shape[1])):
            want = sb if base is None else base.view(_INT_OF[t.dtype])[:, lo:hi]
            bad = int((ti[:, lo:hi] != want).sum())
            assert bad == 0, f'{what}: {bad} {name} elements outside [{pos0}, {pos0 + S}) changed (tokens [{lo}, {hi}))'
        left = int((ti[:, pos0:pos0 + S] == sb).sum())
        assert left == 0, f'{what}: {left} {name} elements inside [{pos0}, {pos0 + S}) were never written'


def make_inputs(nh, nkv, d, S, n_slabs, seed, dev):
    """slabs [n_slabs, S + 3, w] whose rows [2, 2 + S) are this step's (the other rows hold the fp32 sentinel: reading a wrong row shows), the bf16 bias, and the
    qkv rows their sum rounds to"""
    g = torch.Generator().manual_seed(seed)
    w = (nh + 2 * nkv) * d
    mine = torch.randn(n_slabs, S, w, generator=g) / math.sqrt(n_slabs)
    bias = (0.1 * torch.randn(w, generator=g)).to(BF)
    full = sentinel((n_slabs, S + 3, w), torch.float32, dev)
    full[:, 2:2 + S] = mine.to(dev)
    return full, bias.to(dev), L.qkv_from_slabs(mine, bias), 2


def run_write_case(ops, nh, nkv, d, pos0, S, n_slabs):
    dev = ops.dev
    slabs, bias, qkv, row0 = make_inputs(nh, nkv, d, S, n_slabs, pos0 * 131 + S * 7 + nh, dev)
    fr = L.inv_freq(d)
    q_ref, k_ref, v_ref = L.ref_kv_write(qkv, None, fr, pos0, nh, nkv, d, BF)
    cap = L.cap_for(pos0, S)
    qkv_dev = qkv.to(dev)
    Kc, Vc = sentinel((nkv, cap, d), BF, dev), sentinel((nkv, cap, d), BF, dev)
    got = {}
    for writer in (1, 2, 3):
        what = f'writer {writer} heads {nh}/{nkv} pos0 {pos0} S {S} slabs {n_slabs}'
        Kc.view(torch.int16).fill_(SENTINEL_BITS[BF]); Vc.view(torch.int16).fill_(SENTINEL_BITS[BF])
        qbuf, q = guarded(S, nh * d, BF, dev)
        if writer == 3:
            rc = ops.kv_write(3, slabs, fr, nh, nkv, d, pos0, q, Kc, Vc, S=S, bias=bias, row0=row0)
        else:
            rc = ops.kv_write(writer, qkv_dev, fr, nh, nkv, d, pos0, q, Kc, Vc)
        assert rc == 0, what
        Vl = logical_v(Vc, 1)
        assert_footprint(Kc, Vl, None, None, pos0, S, what)
        assert sentinel_intact(qbuf[:16]) and sentinel_intact(qbuf[16 + S:]), f'{what}: q_out guard'
        Kin, Vin, qc = Kc[:, pos0:pos0 + S].cpu(), Vl[:, pos0:pos0 + S].cpu(), q.cpu().clone()
        assert torch.equal(bits(Vin), bits(v_ref)), f'{what}: V differs from the reference in {int((bits(Vin) != bits(v_ref)).sum())} elements'
        assert_close(Kin, k_ref, BF, what=what + ' K')
        assert_close(qc, q_ref, BF, what=what + ' q')
        got[writer] = (qc, Kin)
    for writer in (2, 3):
        for name, a, b in (('q', got[1][0], got[writer][0]), ('K', got[1][1], got[writer][1])):
            assert torch.equal(bits(a), bits(b)), f'writer {writer} vs 1, heads {nh}/{nkv} pos0 {pos0} S {S}: {name} differs in {int((bits(a) != bits(b)).sum())} elements'


@pytest.mark.parametrize('nh,nkv,d,pos0,S,n_slabs', L.write_cases())
def test_writers_1_2_3_store_the_same_bits_in_their_own_slots(ops, nh, nkv, d, pos0, S, n_slabs):
    run_write_case(ops, nh, nkv, d, pos0, S, n_slabs)


@pytest.mark.parametrize('n_slabs', L.SLAB_COUNTS)
@pytest.mark.parametrize('pos0,S', [(57, 8), (60, 70)])
def test_slab_writer_sums_every_slab_count_in_order(ops, pos0, S, n_slabs):
    run_write_case(ops, 28, 4, 128, pos0, S, n_slabs)


@pytest.mark.parametrize('dtype', [torch.float32, BF], ids=['f32', 'bf16'])
@pytest.mark.parametrize('pos0,S', [ps for ps in L.POS_S if ps[0] < L.BIG_POS])
def test_scalar_writer_row_major_and_transposed(ops, ops_f32, dtype, pos0, S):
    """writers 0 / 1 (rope_append_kernel, v_tr = 0 / 1) at head_dim 32 in both dtypes: same q and K bits, V exact in either layout"""
    o = ops if dtype == BF else ops_f32
    nh, nkv, d = L.SMALL_HEADS
    dev = o.dev
    g = torch.Generator().manual_seed(pos0 * 17 + S)
    qkv = torch.randn(S, (nh + 2 * nkv) * d, generator=g).to(dtype)
    fr = L.inv_freq(d)
    q_ref, k_ref, v_ref = L.ref_kv_write(qkv, None, fr, pos0, nh, nkv, d, dtype)
    cap = L.cap_for(pos0, S)
    got = {}
    for writer in (0, 1):
        what = f'writer {writer} {dtype} pos0 {pos0} S {S}'
        Kc, Vc = sentinel((nkv, cap, d), dtype, dev), sentinel((nkv, cap, d), dtype, dev)
        qbuf, q = guarded(S, nh * d, dtype, dev)
        assert o.kv_write(writer, qkv.to(dev), fr, nh, nkv, d, pos0, q, Kc, Vc) == 0, what
        Vl = logical_v(Vc, writer)
        assert_footprint(Kc, Vl, None, None, pos0, S, what)
        assert sentinel_intact(qbuf[:16]) and sentinel_intact(qbuf[16 + S:]), f'{what}: q_out guard'
        assert torch.equal(bits(Vl[:, pos0:pos0 + S].cpu()), bits(v_ref)), what + ' V'
        assert_close(Kc[:, pos0:pos0 + S], k_ref, dtype, what=what + ' K')
        assert_close(q, q_ref, dtype, what=what + ' q')
        got[writer] = (q.cpu().clone(), Kc[:, pos0:pos0 + S].cpu())
    assert torch.equal(bits(got[0][0]), bits(got[1][0])) and torch.equal(bits(got[0][1]), bits(got[1][1]))


@pytest.mark.parametrize('nh,nkv,d,pos0,S,n_slabs', L.decode_cases())
def test_decode_attention_prepares_the_token_it_attends_to(ops, nh, nkv, d, pos0, S, n_slabs):
    """writer 4 against writers 1, 2, 3 and attention variant 3, over pos0 context tokens already in the arena.  Run once with the sentinel behind the context (footprint: the
    context and everything behind the step keep their bits) and once with zeros there (a key tile reaches past the live length, and P = 0 times a NaN V is NaN: the
    attention outputs are compared on finite slots, as the model keeps them)."""
    dev = ops.dev
    slabs, bias, qkv, row0 = make_inputs(nh, nkv, d, S, n_slabs, pos0 * 31 + S + nkv, dev)
    fr = L.inv_freq(d)
    _, k_ref, v_ref = L.ref_kv_write(qkv, None, fr, pos0, nh, nkv, d, BF)
    cap = L.cap_for(pos0, S)
    g = torch.Generator(device=dev).manual_seed(pos0 + 5)
    ctxK = torch.randn(nkv, pos0, d, generator=g, device=dev).to(BF)
    ctxV = torch.randn(nkv, pos0, d, generator=g, device=dev).to(BF)
    what = f'heads {nh}/{nkv} pos0 {pos0} S {S} slabs {n_slabs}'
    for tail in ('sentinel', 'zeros'):
        baseK = sentinel((nkv, cap, d), BF, dev) if tail == 'sentinel' else torch.zeros(nkv, cap, d, dtype=BF, device=dev)
        baseVl = baseK.clone()
        baseK[:, :pos0] = ctxK; baseVl[:, :pos0] = ctxV
        baseV = L.v_raw(baseVl).view(nkv, cap, d)
        # writer 3 + the attention over what it wrote
        K3, V3 = baseK.clone(), baseV.clone()
        qbuf, q3 = guarded(S, nh * d, BF, dev)
        assert ops.kv_write(3, slabs, fr, nh, nkv, d, pos0, q3, K3, V3, S=S, bias=bias, row0=row0) == 0
        # writer 4
        K4, V4 = baseK.clone(), baseV.clone()
        qbuf4, q4 = guarded(S, nh * d, BF, dev)
        obuf, o4 = guarded(S, nh * d, BF, dev)
        assert ops.kv_write(4, slabs, fr, nh, nkv, d, pos0, q4, K4, V4, S=S, bias=bias, row0=row0, attn_out=o4) == 0, what
        assert ops.attention_last_form()[0] == 3
        assert sentinel_intact(qbuf4), f'{what}: writer 4 stores no q'
        assert sentinel_intact(obuf[:16]) and sentinel_intact(obuf[16 + S:]), f'{what}: attention output guard'
        V3l, V4l = logical_v(V3, 1), logical_v(V4, 1)
        if tail == 'sentinel':
            assert_footprint(K4, V4l, baseK, baseVl, pos0, S, what + ' writer 4')
            assert_footprint(K3, V3l, baseK, baseVl, pos0, S, what + ' writer 3')
        assert torch.equal(bits(K4), bits(K3)), f'{what}: K of writer 4 differs from writer 3 in {int((bits(K4) != bits(K3)).sum())} elements'
        assert torch.equal(bits(V4), bits(V3)), f'{what}: V of writer 4 differs from writer 3 in {int((bits(V4) != bits(V3)).sum())} elements'
        assert torch.equal(bits(V4l[:, pos0:pos0 + S].cpu()), bits(v_ref)), what + ' V vs reference'
        assert_close(K4[:, pos0:pos0 + S], k_ref, BF, what=what + ' K')
        if tail == 'sentinel':          # writers 1 and 2 on the qkv rows the slabs round to, at this very position: the K bits of all four, directly
            for writer in (1, 2):
                K1, V1 = baseK.clone(), baseV.clone()
                qbuf1, q1 = guarded(S, nh * d, BF, dev)
                assert ops.kv_write(writer, qkv.to(dev), fr, nh, nkv, d, pos0, q1, K1, V1) == 0
                assert torch.equal(bits(K1), bits(K4)) and torch.equal(bits(V1), bits(V4)), f'{what}: arena of writer {writer} differs from writer 4'
                assert torch.equal(bits(q1), bits(q3)), f'{what}: q of writer {writer} differs from writer 3'
        if tail == 'zeros':
            o3 = ops.attention(q3, K3, V3l.contiguous(), nh, nkv, d, pos0, causal=True, variant=3)
            assert ops.attention_last_form()[0] == 3
            assert torch.isfinite(o4.float()).all() and torch.isfinite(o3.float()).all()
            assert torch.equal(bits(o4), bits(o3)), f'{what}: attention output differs in {int((bits(o4) != bits(o3)).sum())} of {o3.numel()} elements'


def test_unsupported_combinations_are_refused_before_any_launch(ops, ops_f32):
    dev = ops.dev

    def attempt(o, writer, nh, nkv, d, pos0, S, cap, n_slabs=1, dtype=BF, with_out=True):
        w = (nh + 2 * nkv) * d
        Kc, Vc = sentinel((nkv, cap, d), dtype, dev), sentinel((nkv, cap, d), dtype, dev)
        qbuf, q = guarded(S, nh * d, dtype, dev)
        obuf, out = guarded(S, nh * d, dtype, dev)
        src = torch.zeros(n_slabs, S, w, device=dev) if writer >= 3 else torch.zeros(S, w, dtype=dtype, device=dev)
        bias = torch.zeros(w, dtype=BF, device=dev)
        rc = o.kv_write(writer, src, L.inv_freq(d), nh, nkv, d, pos0, q, Kc, Vc, S=S, bias=bias, attn_out=out if with_out else None)
        assert sentinel_intact(Kc) and sentinel_intact(Vc) and sentinel_intact(qbuf) and sentinel_intact(obuf)
        return rc
    assert attempt(ops, 5, 4, 2, 128, 0, 1, 128) == MMD_EINVAL
    assert attempt(ops, 2, 4, 2, 32, 0, 1, 128) == MMD_EINVAL                       # the chunk kernel is head_dim 128 only
    assert attempt(ops_f32, 2, 4, 2, 128, 0, 1, 128, dtype=torch.float32) == MMD_EINVAL
    assert attempt(ops_f32, 3, 4, 2, 128, 0, 1, 128, dtype=torch.float32) == MMD_EINVAL
    assert attempt(ops, 3, 4, 2, 128, 0, 1, 128, n_slabs=17) == MMD_EINVAL
    assert attempt(ops, 4, 4, 2, 128, 0, 1, 128, n_slabs=5) == MMD_EINVAL
    assert attempt(ops, 4, 28, 4, 128, 0, 3, 128) == MMD_EINVAL                     # 21 rows per kv head
    assert attempt(ops, 4, 4, 2, 128, 0, 1, 128, with_out=False) == MMD_EINVAL
    assert attempt(ops, 1, 4, 2, 128, 0, 1, 100) == MMD_EINVAL                      # transposed V needs whole blocks
    assert attempt(ops, 1, 4, 2, 128, 120, 9, 128) == MMD_EINVAL                    # past the end of the arena
    assert attempt(ops, 1, 5, 2, 128, 0, 1, 128) == MMD_EINVAL                      # heads not a multiple of kv heads
