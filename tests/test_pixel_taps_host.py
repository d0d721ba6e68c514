"""The pixel front end's host arithmetic (mmduet_amd/csrc/pixel_taps.h) without a GPU: tests/pixel_taps_shim.cpp is compiled with the host C++ compiler into a temporary
directory, loaded with ctypes, and its tables compared with the restatements under oracle/ -- Pillow's bicubic taps for every source size of two sweeps, with the properties
the kernels rely on (no read past a row or a table row, taps that sum to one, an `int` accumulator that cannot overflow); OpenCV's bilinear taps for both axes; the letterbox
geometry and the exact-2x decision.  Then, where Pillow is installed, the numpy resampler the GPU tests use as their reference against Pillow itself on the case table's
images (tests/pixel_cases.py)."""
import ctypes as C
import json
import os
import shutil
import subprocess
import numpy as np
import pytest

import pixel_cases as P
from oracle import preprocess as op
from oracle import video_input as ov

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason='no host C++ compiler')
ONE = 1 << op.PRECISION_BITS          # a tap of 1.0


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('pixel_taps') / 'pixel_taps_shim.so')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', os.path.join(HERE, 'pixel_taps_shim.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.pixel_ksize_shim.argtypes = [C.c_int] * 2
    lib.pil_coeffs_shim.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong]
    lib.cv_linear_taps_shim.argtypes = [C.c_int] * 3 + [C.c_void_p]
    lib.letterbox_geom_shim.argtypes = [C.c_int] * 3 + [C.c_void_p]
    lib.letterbox_grid_shim.argtypes = [C.c_int] * 2 + [C.c_void_p]
    lib.letterbox_geom_shim.restype = lib.letterbox_grid_shim.restype = None

    class Ask:
        @staticmethod
        def coeffs(n_in, n_out):
            """-> (ksize, bounds [n_out, 2], taps [n_out, ksize]) int32"""
            ks = lib.pixel_ksize_shim(n_in, n_out)
            coef, bounds = np.full(n_out * ks, 0x55555555, np.int32), np.full(n_out * 2, 0x55555555, np.int32)
            assert lib.pil_coeffs_shim(n_in, n_out, coef.ctypes.data, coef.size, bounds.ctypes.data, bounds.size) == ks
            return ks, bounds.reshape(n_out, 2), coef.reshape(n_out, ks)

        @staticmethod
        def cv_taps(src, dst, x_axis):
            tab = np.full(dst * 4, 0x55555555, np.int32)
            assert lib.cv_linear_taps_shim(src, dst, int(x_axis), tab.ctypes.data) == 0
            return tab.reshape(dst, 4)

        @staticmethod
        def geom(W, H, R):
            out = np.zeros(7, np.int32)
            lib.letterbox_geom_shim(W, H, R, out.ctypes.data)
            return tuple(int(v) for v in out)

        @staticmethod
        def grid(n, R):
            out = np.zeros((n, n, 7), np.int32)
            lib.letterbox_grid_shim(n, R, out.ctypes.data)
            return out
    return Ask


# ---- Pillow's tap tables ---------------------------------------------------------------------------------------------------------------------------------------------
@needs_cxx
@pytest.mark.parametrize('n_out,n_max', P.COEFF_SWEEPS, ids=lambda v: str(v))
def test_pil_coeffs_equal_the_oracle_and_keep_the_kernels_in_bounds(shim, n_out, n_max):
    """Every source size 1..n_max: ksize, every bound and every int32 tap equal the oracle's.  Per table row:
      * xmin >= 0, xmin + xmax <= in and 0 <= xmax <= ksize -- the kernels read src[xmin .. xmin + xmax) and k[0 .. xmax): no read past an image row or a table row;
      * the taps sum to 2^22 within +- ksize / 2: Pillow divides the double taps by their sum (so they sum to 1 up to double rounding, ~1e-16 per tap, nothing at 2^22
        scale) and then rounds each of the at most ksize nonzero taps to the nearest integer, half a unit of error each -- the bound is that count times 1/2, not a fit;
      * 255 sum |tap| + 2^21 < 2^31: the kernels, like Pillow, accumulate in `int` from the rounding constant 2^21; the worst pixel row has 255 under every tap of one
        sign and 0 under the others, so this bounds every partial sum as well.  (The oracle accumulates in int64 and would not see an overflow.)"""
    worst_sum = worst_room = 0
    for n_in in range(1, n_max + 1):
        ks, b, k = shim.coeffs(n_in, n_out)
        ob, ok, oks = op.pil_bicubic_coeffs(n_in, n_out)
        assert ks == oks == P.ksize(n_in, n_out), n_in
        assert np.array_equal(b, np.asarray(ob)), n_in
        assert np.array_equal(k, ok), n_in
        xmin, xmax = b[:, 0].astype(np.int64), b[:, 1].astype(np.int64)
        assert (xmin >= 0).all() and (xmax >= 0).all() and (xmin + xmax <= n_in).all() and (xmax <= ks).all(), n_in
        assert (xmax >= 1).all(), n_in          # every output pixel has a source pixel under it
        k64 = k.astype(np.int64)
        assert (np.where(np.arange(ks)[None, :] >= xmax[:, None], k64, 0) == 0).all(), n_in          # nothing beyond the count
        dev = np.abs(k64.sum(1) - ONE)
        assert (2 * dev <= ks).all(), (n_in, int(dev.max()), ks)
        room = 255 * np.abs(k64).sum(1) + (1 << 21)
        assert (room < (1 << 31)).all(), (n_in, int(room.max()))
        worst_sum, worst_room = max(worst_sum, int(dev.max())), max(worst_room, int(room.max()))
    print(f'out {n_out}, in 1..{n_max}: max |sum - 2^22| = {worst_sum}, max 255 sum|tap| + 2^21 = {worst_room} = {worst_room / (1 << 31):.3f} x 2^31')


# ---- OpenCV's bilinear taps ------------------------------------------------------------------------------------------------------------------------------------------
@needs_cxx
@pytest.mark.parametrize('x_axis', [True, False], ids=['x', 'y'])
@pytest.mark.parametrize('dst', P.CV_DST)
def test_cv_linear_taps_equal_the_oracle(shim, dst, x_axis):
    for src in range(1, P.CV_SRC_MAX + 1):
        tab = shim.cv_taps(src, dst, x_axis)
        s0, s1, w0, w1 = ov.cv2_linear_taps(src, dst, x_axis)
        assert np.array_equal(tab, np.stack([s0, s1, w0, w1], 1)), (src, dst, x_axis)
        assert tab[:, :2].min() >= 0 and tab[:, :2].max() <= src - 1, (src, dst)          # the kernel reads rows / columns s0 and s1 of the frame


# ---- letterbox geometry and the exact-2x decision --------------------------------------------------------------------------------------------------------------------
def _area2x(W, H, nw, nh):
    """both scales exactly 2, as integers"""
    return int(2 * nw == W and 2 * nh == H)


@needs_cxx
@pytest.mark.parametrize('R', P.GEOMETRY_R)
def test_letterbox_geometry_and_area2x_equal_the_oracle_on_a_grid(shim, R):
    n = P.GEOMETRY_MAX
    got = shim.grid(n, R)
    hits = 0
    for W in range(1, n + 1):
        for H in range(1, n + 1):
            nw, nh, pads = ov.letterbox_geometry(W, H, R)
            want2x = _area2x(W, H, nw, nh) if nw > 0 and nh > 0 else -1
            assert tuple(int(v) for v in got[W - 1, H - 1]) == (nw, nh) + tuple(pads) + (want2x,), (W, H, R)
            hits += want2x == 1
    assert hits >= 1 or 2 * R > n          # the grid reaches exact-2x frames wherever 2R fits in it
    # ... and the oracle's own decision (the expression inside cv2_resize_linear_u8) is the integer one: its 2x2 box average on a frame the grid calls exact-2x
    if 2 * R <= n:
        img = np.random.default_rng(R).integers(0, 256, (2 * R, 2 * R, 3), dtype=np.uint8).astype(np.int64)
        box = ((img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2] + 2) >> 2).astype(np.uint8)
        assert got[2 * R - 1, 2 * R - 1, 6] == 1 and np.array_equal(ov.cv2_resize_linear_u8(img.astype(np.uint8), R, R), box)


@needs_cxx
def test_area2x_cases_and_the_recorded_runs(shim):
    for W, H, R, want in P.AREA2X:
        g = shim.geom(W, H, R)
        nw, nh, pads = ov.letterbox_geometry(W, H, R)
        assert g[:6] == (nw, nh) + tuple(pads), (W, H, R)
        assert g[6] == want == _area2x(W, H, nw, nh), (W, H, R, g)
    assert {w for *_, w in P.AREA2X} == {0, 1}
    runs = json.load(open(os.path.join(HERE, 'golden', 'video_input.json')))['runs']
    seen = 0
    for r in runs:
        if 'error' in r:
            continue
        p, R = r['props'], r['resolution']
        g = shim.geom(p['w'], p['h'], R)
        assert [g[0], g[1]] == r['resize_to'] and list(g[2:6]) == r['pads'], r['video']
        assert g[6] == _area2x(p['w'], p['h'], g[0], g[1])
        seen += 1
    assert seen >= 32


# ---- the case table, and the GPU tests' reference against Pillow -----------------------------------------------------------------------------------------------------------
def test_the_image_families_differ_in_every_frame_and_channel():
    assert set(P.FUSED_R) <= set(P.R_SWEEP_56) | {P.SIZE} and {R for seq in P.CACHE_SEQUENCES.values() for R, _ in seq} <= set(P.R_SWEEP_56) | {P.SIZE}
    assert P.CACHE_SEQUENCES['reversed'] == P.CACHE_SEQUENCES['alternating'][::-1]
    assert {P.ksize(R, 56) for R in P.R_SWEEP_56} >= {5, 7, 9, 11, 13, 17, 19, 25, 31}
    for fam in P.FAMILIES:
        for R in (1, 2, 3, 8, 57):
            fr = P.frames(fam, 3, R)
            assert fr.dtype == np.uint8 and fr.shape == (3, 3, R, R)
            assert np.array_equal(fr, P.frames(fam, 3, R))          # seeded
            planes = {pl.tobytes() for pl in fr.reshape(9, -1)}
            # the two-valued families have only 2^(R^2) images of R^2 pixels to choose 9 planes from, and 'corners' R^2 - 4 places for its fifth dot
            few = (fam in ('checker', 'binary') and R * R < 8) or (fam == 'corners' and 2 < R and R * R - 4 < 9)
            assert len(planes) == 9 or few, (fam, R, len(planes))
    for fam in ('checker', 'binary', 'corners'):
        assert set(np.unique(P.frames(fam, 3, 57))) == {0, 255} and set(np.unique(P.frames(fam, 3, 3))) == {0, 255}
    assert P.frames('flat0', 1, 8)[0, 0].max() == 0 and P.frames('flat255', 1, 8)[0, 0].min() == 255
    c = P.frames('corners', 3, 29)
    assert (c[:, :, [0, 0, -1, -1], [0, -1, 0, -1]] == 255).all() and (c.reshape(9, -1) == 255).sum(1).tolist() == [5] * 9
    r = P.frames('ramp', 1, 29)[0]
    assert (r[0] == r[0][:1]).all() and (r[1] == r[1][:, :1]).all() and (r[2] == r[2].T).all() and r[0, 0, 0] == 0 and r[0, 0, -1] == r[1, -1, 0] == r[2, -1, -1] == 255


def test_numpy_resampler_equals_pillow_on_the_case_table():
    """The reference of tests/test_gpu_pixel_frontend.py against the library it restates.  Skipped only where PIL cannot be imported."""
    Image = pytest.importorskip('PIL.Image')
    for R in P.R_SWEEP_56:
        for fam in ('noise', 'checker', 'binary'):
            for fr in P.frames(fam, 2, R):
                img = np.ascontiguousarray(fr.transpose(1, 2, 0))
                want = np.asarray(Image.fromarray(img).resize((P.SIZE, P.SIZE), resample=Image.BICUBIC))
                got = op.pil_resize_bicubic_u8(img, P.SIZE)
                assert np.array_equal(got, want), (R, fam, int(np.abs(got.astype(int) - want).max()))
