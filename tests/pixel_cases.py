"""The pixel front end's table of cases (uint8 frame -> letterbox -> Pillow-exact bicubic resample -> normalise -> patch-embed operand).  Plain data and seeded generators:
imports without a GPU and without PIL.  tests/test_pixel_taps_host.py asks mmduet_amd/csrc/pixel_taps.h about the tables on the host, tests/test_gpu_pixel_frontend.py runs
the same sizes and images on the device against the numpy restatement of Pillow's resampler (oracle/preprocess.py).

Source sizes R (square frames) into the 56 px test tower, chosen by what the tap tables do there (ksize = 2 ceil(2 max(R / 56, 1)) + 1 taps per output pixel):
  * 1, 2, 3 -- both bounds clip on every output pixel; 5, 8 -- strong upscales, most rows clipped on one side;
  * 27 | 28 | 29 and 55 | 56 | 57 -- either side of the exact 2x upscale and of the identity (56 itself takes the branch without tables);
  * 47, 48, 63, 70, 84 -- scales near 1 on both sides (ksize 5, 7);  111 | 112 | 113, 167 | 168 -- either side of the exact 2x downscale (ksize 9 -> 11) and up to the exact 3x one (13);
  * 140, 224, 225, 336, 400 -- 2.5x to 7.14x (224 | 225: ksize 17 -> 19 at the exact 4x), ksize up to 31: where letterboxed 720p and 768 px sources land relative to the tower.
... and into the true 384 px tower: the shipped 336, 383 | 385 around the identity, 448, and 768 | 769 around the exact 2x downscale."""
import numpy as np

SIZE = 56
R_SWEEP_56 = (1, 2, 3, 5, 8, 27, 28, 29, 47, 48, 55, 57, 63, 70, 84, 111, 112, 113, 140, 167, 168, 224, 225, 336, 400)          # (the device sweep adds the identity, 56)
R_SWEEP_384 = (336, 383, 385, 448, 768, 769)          # once, at T = 1, in the true-width test only

FAMILIES = ('noise', 'checker', 'binary', 'flat0', 'flat255', 'ramp', 'corners')


def ksize(R, size):
    """taps per table row, as Pillow sizes them"""
    return int(np.ceil(2.0 * max(R / size, 1.0))) * 2 + 1


def frames(family, T, R, seed=0):
    """-> uint8 [T,3,R,R]; every frame and every channel different (where R leaves room: a plane holds R^2 pixels), so a wrong plane index shows"""
    g = np.random.default_rng([seed, FAMILIES.index(family), T, R])
    y, x = np.mgrid[0:R, 0:R]
    out = np.zeros((T, 3, R, R), np.uint8)
    for t in range(T):
        for c in range(3):
            pl = 3 * t + c
            if family == 'noise':
                a = g.integers(0, 256, (R, R))
            elif family == 'checker':          # 0/255 at period 1, and at period 3 where R allows; one pixel, another in every plane, is flipped so that all planes differ
                p = 3 if (R >= 6 and pl % 2) else 1
                a = 255 * (((y + pl // 2) // p + x // p) % 2)
                i = (pl * max(1, R * R // (3 * T))) % (R * R)
                a[i // R, i % R] ^= 255
            elif family == 'binary':
                a = 255 * g.integers(0, 2, (R, R))
            elif family == 'flat0':          # flat at the low end: 0, 1, 2, ... per plane (plane 0 is the all-zero one)
                a = np.full((R, R), pl % 32)
            elif family == 'flat255':
                a = np.full((R, R), 255 - pl % 32)
            elif family == 'ramp':          # horizontal in channel 0, vertical in channel 1, diagonal in channel 2; the direction changes with the frame, the offset with the plane
                u = (x, y, x + y)[c]
                span = max(1, (R - 1) * (2 if c == 2 else 1))
                a = (u * 255) // span
                a = 255 - a - pl if t % 2 else a + pl
                a = np.clip(a, 0, 255)
            elif family == 'corners':          # zeros, 255 at the four corner pixels and at one other pixel, another in every plane (R <= 2 has none: the value changes instead)
                a = np.zeros((R, R), np.int64)
                a[0, 0] = a[0, R - 1] = a[R - 1, 0] = a[R - 1, R - 1] = 255 - (pl if R <= 2 else 0)
                rest = [i for i in range(R * R) if i not in (0, R - 1, R * R - R, R * R - 1)]
                if rest:
                    i = rest[(len(rest) // 2 + pl * max(1, len(rest) // (3 * T))) % len(rest)]
                    a[i // R, i % R] = 255
            else:
                raise KeyError(family)
            out[t, c] = a
    return out


# (R, T) calls on ONE model: the tap tables are cached per context, keyed on R alone, rebuilt when R changes; the scratch image only grows; ksize is carried over from the
# last resampled call.  The first sequence alternates R, passes through the identity size between two resampled sizes, shrinks and regrows T, and moves ksize from large to
# small and back; the second is the first reversed; the third starts at the identity (no table yet) and returns to it after each size.
_SEQ = [(48, 2), (70, 2), (48, 2), (56, 2), (70, 1), (140, 5), (48, 9), (3, 1), (400, 1), (56, 3), (48, 1)]
CACHE_SEQUENCES = {
    'alternating': _SEQ,
    'reversed': _SEQ[::-1],
    'identity_first': [(56, 1), (400, 2), (56, 4), (1, 3), (56, 1), (57, 9), (55, 9)],
}

# fused entry (mmd_vit_encode_frames) against preprocess -> visual_embed
FUSED_R = (1, 3, 28, 48, 55, 56, 57, 70, 113, 140, 400)
FUSED_FAMILIES = ('noise', 'checker', 'corners')

# letterbox -> preprocess: frames [H, W] letterboxed to R, then resampled to the tower's 56
LETTERBOX_HW = ((97, 131), (131, 97), (112, 112), (2, 3))
LETTERBOX_R = (48, 70, 112)
LETTERBOX_PAD = (9, 120, 255)

# mmd_normalize_frames with three different means and stds
NORM_R = (5, 37)
NORM_B = 3
NORM_MEAN = (0.1, 0.45, 0.8)
NORM_STD = (0.2, 0.5, 1.3)
NORM_RESCALE = 1 / 255

# host sweeps of the tap tables: every source size up to these, per output size
COEFF_SWEEPS = ((56, 800), (384, 1100))
CV_DST = (1, 2, 36, 56, 215, 216, 336, 384)
CV_SRC_MAX = 1300
GEOMETRY_R = (8, 56, 384)
GEOMETRY_MAX = 200
# (W, H, R, area2x): the exact-2x shortcut is taken when BOTH scales are exactly 2 -- (112, 80, 56): new_h = 40; (113, 80, 56): sx = 113 / 56; (224, 112, 112) both 2 again
AREA2X = ((112, 112, 56, 1), (112, 80, 56, 1), (113, 80, 56, 0), (112, 81, 56, 0), (111, 111, 56, 0), (224, 112, 112, 1), (768, 768, 384, 1), (769, 768, 384, 0), (56, 56, 56, 0), (2, 2, 1, 1))
