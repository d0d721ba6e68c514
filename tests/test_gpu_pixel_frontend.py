"""The pixel front end on the device, bit for bit: uint8 frame -> letterbox -> Pillow-exact bicubic resample -> normalise -> patch-embed operand, over the case table of
tests/pixel_cases.py.  The reference is always the numpy restatement of Pillow's resampler (oracle/preprocess.py::pil_resize_bicubic_u8, held to Pillow itself on the
same images by tests/test_pixel_taps_host.py) followed by the two fp32 operations of oracle.preprocess.siglip_preprocess; a bf16 result is that fp32 value rounded once.
Both resampling passes are integer arithmetic, so every comparison is torch.equal / np.array_equal; a failure names the first differing (t, c, y, x) and the largest
distance in LSBs of the uint8 image recovered from the output.

  * resampler sweep -- image_processor.preprocess for every source size of R_SWEEP_56 and the identity, every image family, 3 frames, fp32 and bf16;
  * cache sequences -- the tap tables are cached per context, keyed on the source size; the scratch image only grows; ksize is carried over: each sequence of (R, T) calls
    runs on one model, every call against the oracle, the first call again at the end; then the same sequence through visual_embed_frames, interleaved with preprocess
    calls at other sizes (both entry points share the tables);
  * fused against two-call -- visual_embed_frames(fr) == visual_embed(preprocess(fr)) over FUSED_R x {noise, checker, corners} x {1, max_vit_batch, max_vit_batch + 3}
    frames, fp32 and bf16; and in both half-precision tower modes of tests/tower_regimes.py, whose fused path writes an fp16 operand.  No entry point exposes that operand
    (mmd_vit_debug_tap returns the tower's output and the projector's), so the half towers are held end to end: the fused result must also equal visual_embed of the ORACLE's
    pixels rounded to bf16, which only an operand equal to ref.to(bfloat16).to(float16) gives;
  * letterbox -> preprocess against ov.letterbox_frame -> pil_resize_bicubic_u8 -> normalise, with a pad colour that shows a misplaced border after the resample;
  * mmd_normalize_frames on a vision-only context with three different means and stds, uint8 and float32 input, fp32 and bf16;
  * once at the true width: R_SWEEP_384 -> 384, one frame, fp32."""
import ctypes as C
import functools
import json
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import pixel_cases as P
import tower_regimes as TR
from conftest import load_npz
from helpers import hip_model
from oracle import video_input as ov
from oracle.preprocess import pil_resize_bicubic_u8

DTYPES = (torch.float32, torch.bfloat16)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------------------
def _resampled(frames_u8, size):
    """uint8 [T,3,R,R] -> uint8 [T,3,size,size] as Pillow resamples it (the identity at R == size, as the image processor skips the resize there)"""
    if frames_u8.shape[2] == size:
        return frames_u8.copy()
    return np.stack([pil_resize_bicubic_u8(np.ascontiguousarray(f.transpose(1, 2, 0)), size).transpose(2, 0, 1) for f in frames_u8])


def _normalised(u8):
    """oracle.preprocess.siglip_preprocess's arithmetic: x * float32(1/255), (x - 0.5) / 0.5, in fp32"""
    return (torch.from_numpy(np.ascontiguousarray(u8)).float() * np.float32(1 / 255) - 0.5) / 0.5


@functools.lru_cache(maxsize=None)
def _case(family, T, R, size=P.SIZE, seed=0):
    """-> (frames uint8 [T,3,R,R], resampled uint8, fp32 pixel_values), computed once per case and shared (read-only) by the tests"""
    fr = P.frames(family, T, R, seed)
    u8 = _resampled(fr, size)
    ref = _normalised(u8)
    u8.setflags(write=False)
    return torch.from_numpy(fr), u8, ref


def _same_pixels(pv, u8, ref, what):
    """pv (device, model dtype) == ref (fp32) rounded once to pv's dtype; on failure: where first, and how far in LSBs of the uint8 image behind pv"""
    got, want = pv.cpu(), ref.to(pv.dtype)
    if got.shape == want.shape and torch.equal(got, want):
        return
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    back = torch.round((got.float() * 0.5 + 0.5) * 255).clamp(0, 255).to(torch.int64).numpy()
    lsb = np.abs(back - u8.astype(np.int64))
    first = tuple(int(v) for v in np.argwhere((got != want).numpy())[0])
    raise AssertionError(f'{what}: {int((got != want).sum())} of {got.numel()} values differ, first at (t, c, y, x) = {first}: got {got[first].item()!r}, '
                         f'want {want[first].item()!r}; recovered uint8 image: max distance {int(lsb.max())} LSB, {int((lsb > 0).sum())} pixels off')


def _ordinal(t):
    """fp32 / bf16 values as integers in value order, so that a difference counts units in the last place"""
    i = t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).to(torch.int64)
    mag = i & (0x7fffffff if t.dtype == torch.float32 else 0x7fff)
    return torch.where(i < 0, -mag, mag)


def _preprocess(m, fr):
    return m.get_vision_tower().image_processor.preprocess(fr)['pixel_values']


@pytest.fixture(scope='module')
def models():
    ms = {dt: hip_model('A', dt)[0] for dt in DTYPES}
    assert all(m.config.vit_image_size == P.SIZE and m.max_vit_batch == 8 for m in ms.values())
    yield ms
    ms.clear()
    torch.cuda.empty_cache()


# ---- resampler sweep -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', P.R_SWEEP_56 + (P.SIZE,))
def test_preprocess_equals_pillow_resampler_over_the_sweep(models, R):
    for family in P.FAMILIES:
        fr, u8, ref = _case(family, 3, R)
        for dt, m in models.items():
            pv = _preprocess(m, fr)
            assert pv.dtype == dt
            _same_pixels(pv, u8, ref, f'preprocess {family} R={R} {dt}')


# ---- the tap-table cache ---------------------------------------------------------------------------------------------------------------------------------------------
def _other(R):
    """a source size with other tables than R's (and another ksize than most)"""
    return 63 if R in (140, 400, P.SIZE) else 140


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', list(P.CACHE_SEQUENCES))
def test_table_cache_sequences_on_one_model(name, dtype):
    seq = P.CACHE_SEQUENCES[name]
    m = hip_model('A', dtype)[0]          # a context of its own: the cache starts empty
    calls = [(R, T) + _case('noise', T, R, seed=7 + i % 3) for i, (R, T) in enumerate(seq)]
    for i, (R, T, fr, u8, ref) in enumerate(calls + calls[:1]):
        _same_pixels(_preprocess(m, fr), u8, ref, f'{name} call {i}: preprocess R={R} T={T}')
    # the same sequence through the fused entry, a preprocess call at another size after each: against visual_embed of the ORACLE's pixels (which touches no table)
    for i, (R, T, fr, u8, ref) in enumerate(calls + calls[:1]):
        one = m.visual_embed_frames(fr)
        two = m.visual_embed(ref.to(dtype))
        assert one.shape == two.shape == (T * m.tokens_per_frame, m.config.hidden_size) and torch.equal(one, two), f'{name} call {i}: visual_embed_frames R={R} T={T}'
        fr2, u82, ref2 = _case('binary', 2, _other(R))
        _same_pixels(_preprocess(m, fr2), u82, ref2, f'{name} call {i}: preprocess R={_other(R)} after visual_embed_frames R={R}')
        assert torch.equal(m.visual_embed_frames(fr), two), f'{name} call {i}: visual_embed_frames R={R} T={T} after preprocess R={_other(R)}'


# ---- fused against two-call --------------------------------------------------------------------------------------------------------------------------------------------
def _fused_is_two_call(m, R, batches, families=P.FUSED_FAMILIES, size=P.SIZE):
    for family in families:
        for B in batches:
            fr = torch.from_numpy(P.frames(family, B, R, seed=B))
            pv = _preprocess(m, fr)
            assert pv.shape == (B, 3, size, size) and pv.dtype == m.dtype
            two = m.visual_embed(pv)
            one = m.visual_embed_frames(fr)
            assert one.shape == two.shape == (B * m.tokens_per_frame, m.config.hidden_size) and torch.isfinite(one.float()).all(), (family, R, B)
            assert torch.equal(one, two), (family, R, B, int((one != two).sum()))


@pytest.mark.parametrize('R', P.FUSED_R)
def test_fused_entry_equals_preprocess_then_visual_embed(models, R):
    for dt, m in models.items():
        _fused_is_two_call(m, R, (1, m.max_vit_batch, m.max_vit_batch + 3))


# ---- fp16 towers: the fused path writes an fp16 operand (the fp32 value rounded to bf16, then to half) ------------------------------------------------------------------
HALF_MODES = [mode for mode, (_, f16) in TR.MODES.items() if f16]
HALF_GRID = TR.TOWERS['small16']['grid']
HALF_SIZE = HALF_GRID * 14
HALF_FAMILIES = ('noise', 'corners')
HALF_R = (1, 57, 113, HALF_SIZE - 1, HALF_SIZE, HALF_SIZE + 1, 400, 2 * HALF_SIZE + 1)


@pytest.mark.parametrize('mode', HALF_MODES)
def test_fused_entry_in_the_half_precision_towers(mode):
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    from mmduet_amd.weights import synthetic_weights
    assert HALF_MODES == ['fp16', 'fp16_resid16'] and TR.MODES[mode][0] == TR.BF16
    tw = TR.TOWERS['small16']
    out = -(-HALF_GRID // tw['pool_stride'])
    pcfg = VideoHeadLiveLlavaQwenConfig(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                                        vit_hidden_size=tw['C'], vit_intermediate_size=tw['ipad'], vit_num_hidden_layers=tw['layers'] + 1, vit_layers_removed=1,
                                        vit_num_attention_heads=tw['heads'], vit_image_size=HALF_SIZE, vit_patch_size=14, video_pooling_stride=tw['pool_stride'],
                                        frame_num_tokens=out * out, frame_resolution=HALF_SIZE, v_placeholder='<image>')
    pcfg.tower_dtype = mode
    m = VideoHeadLiveLlavaQwenForCausalLM(pcfg, torch_dtype=torch.bfloat16, max_vit_batch=tw['max_batch'], max_step_tokens=64, kv_initial_tokens=256)
    assert m.tower_dtype == mode
    for name, t in synthetic_weights(pcfg, seed=7, device=m.device, dtype=torch.bfloat16, scale='unit'):
        m.load_tensor(name, t)
    m.finalize()
    for R in HALF_R:
        # B = 1 keeps the full last layer, B >= 2 runs it on the pooled rows (fp16_g16_b1 | b2 of the regime table); 11 frames: a partial last tower batch
        _fused_is_two_call(m, R, (1, m.max_vit_batch + 3), families=HALF_FAMILIES, size=HALF_SIZE)
        assert m.tower_last_plan()['dt'] == TR.F16
        for family in HALF_FAMILIES:          # ... and against the oracle's pixels, on both sides of that gate
            for B in (1, 3):
                fr, u8, ref = _case(family, B, R, HALF_SIZE)
                _same_pixels(_preprocess(m, fr), u8, ref, f'{mode}: preprocess {family} R={R} B={B}')
                assert torch.equal(m.visual_embed_frames(fr), m.visual_embed(ref.to(m.dtype))), (mode, family, R, B, 'oracle pixels')


# ---- letterbox -> preprocess ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', P.LETTERBOX_HW)
def test_letterbox_then_preprocess_equals_the_composition(models, H, W):
    from mmduet_amd import video_input as pv
    raw = np.random.default_rng([H, W]).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    raw[1] = 255 * (raw[1] > 127)          # one saturated frame
    for R in P.LETTERBOX_R:
        boxed = np.stack([ov.letterbox_frame(f, R, P.LETTERBOX_PAD, True) for f in raw])
        u8 = _resampled(boxed, P.SIZE)
        ref = _normalised(u8)
        for dt, m in models.items():
            lb = pv.letterbox_frames(m, torch.from_numpy(raw), R, pad_color=P.LETTERBOX_PAD, bgr_input=True)
            assert lb.dtype == torch.uint8 and np.array_equal(lb.cpu().numpy(), boxed), (H, W, R, 'letterbox')
            _same_pixels(_preprocess(m, lb), u8, ref, f'letterbox {H}x{W} -> {R} -> preprocess {dt}')


# ---- mmd_normalize_frames ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_normalize_frames_with_three_different_means_and_stds(dtype):
    """((x.float() * float32(rescale) - mean) / std) in fp32, rounded once to the context dtype: fp32 bit-equal (the library is built with -ffp-contract=off and hipcc's
    fp32 division is correctly rounded, as torch's on the host and numpy's are -- the same expression in numpy float32 is held equal to torch's here)."""
    from mmduet_amd import vision_live as VL
    z = load_npz('vision_live.npz')
    cfg = json.loads(bytes(z['__config__']).decode())['siglip']
    w = {k[len('siglip.w.'):]: torch.from_numpy(v) for k, v in z.items() if k.startswith('siglip.w.')}
    enc = VL.LiveVisionEncoder.from_state_dict('siglip', cfg, w, torch_dtype=dtype, frame_token_cls=False, frame_token_pooled=(2, 2))
    assert enc._cfg.vision_only == 1
    mean, std = (C.c_float * 3)(*P.NORM_MEAN), (C.c_float * 3)(*P.NORM_STD)
    mt, st = (torch.tensor(v, dtype=torch.float32).view(1, 3, 1, 1) for v in (P.NORM_MEAN, P.NORM_STD))
    for R in P.NORM_R:
        base = P.frames('noise', P.NORM_B, R, seed=R)
        base[0, :, 0, :4] = np.array([0, 1, 254, 255], np.uint8)
        if R * R >= 256:
            base[1].reshape(3, -1)[:, :256] = np.arange(256, dtype=np.uint8)          # every uint8 value under every mean and std
        for kind, x in ((0, torch.from_numpy(base)), (1, torch.from_numpy(base).float() + torch.linspace(-0.5, 0.5, R).view(1, 1, 1, R))):
            ref = (x.float() * np.float32(P.NORM_RESCALE) - mt) / st
            xn = x.float().numpy()
            ref_np = (xn * np.float32(P.NORM_RESCALE) - mt.numpy()) / st.numpy()
            assert ref.dtype == torch.float32 and ref_np.dtype == np.float32 and np.array_equal(ref.numpy(), ref_np)
            xd = x.to(enc.device).contiguous()
            out = torch.empty(P.NORM_B, 3, R, R, dtype=dtype, device=enc.device)
            with enc._lock:
                VL.lib().mmd_set_stream(enc._ctx, C.c_void_p(torch.cuda.current_stream(enc.device).cuda_stream))
                VL.check(VL.lib().mmd_normalize_frames(enc._ctx, VL._p(xd), kind, P.NORM_B, R, mean, std, np.float32(P.NORM_RESCALE).item(), VL._p(out)), enc._ctx,
                         'mmd_normalize_frames')
            got, want = out.cpu(), ref.to(dtype)
            bad = got != want
            if bad.any():
                first = tuple(int(v) for v in np.argwhere(bad.numpy())[0])
                ulp = (_ordinal(got) - _ordinal(want)).abs()
                raise AssertionError(f'normalize R={R} kind={kind} {dtype}: {int(bad.sum())} of {bad.numel()} differ, first at (b, c, y, x) = {first}: x = {x[first].item()!r}, '
                                     f'got {got[first].item()!r}, want {want[first].item()!r}; max distance {int(ulp.max())} ulp')


# ---- the true width ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model384():
    """the small model of test_gpu_model.py::test_preprocess_336_to_384_bit_exact: a 384 px tower in front of a 64-wide everything"""
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    cfg = VideoHeadLiveLlavaQwenConfig(vocab_size=64, hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=4,
                                       num_key_value_heads=2, frame_num_tokens=49, vit_hidden_size=64, vit_intermediate_size=64,
                                       vit_num_hidden_layers=2, vit_num_attention_heads=4)
    m = VideoHeadLiveLlavaQwenForCausalLM(cfg, torch_dtype=torch.float32, max_vit_batch=1, max_step_tokens=64)
    assert m.config.vit_image_size == 384
    yield m
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize('R', P.R_SWEEP_384)
def test_preprocess_at_the_true_width(model384, R):
    for family in ('noise', 'checker'):
        fr, u8, ref = _case(family, 1, R, 384)
        _same_pixels(_preprocess(model384, fr), u8, ref, f'preprocess {family} {R} -> 384')
