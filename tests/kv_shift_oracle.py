"""mmd_kv_drop_shift stated on the host in numpy, for tests/test_kv_shift_host.py (CPU), tests/test_gpu_kv_shift.py and tests/test_gpu_kv_shift_trueshape.py.

Canonical K, V [layers][nkv][n][d] (any leading dims).  Tokens [frm, to) leave; V's rows behind them move down unchanged; K's rows behind them move down turned back
by delta = to - frm positions: dims (e, e + d/2) with frequency e, the pairing rope_append_kernel writes with.  The ANGLE is the fp32 product
np.float32(delta) * inv_freq32 -- the same IEEE product the device forms --; cos / sin and the rotation are float64, so the result is exact to float64 rounding and the
tests hold the device against it under a derived bound (`bound`)."""
import numpy as np


def angles(delta, inv_freq32):
    """the d/2 angles of a shift by delta positions, as the device forms them: one fp32 product each -> float64"""
    a = np.float32(delta) * np.asarray(inv_freq32, dtype=np.float32)
    assert a.dtype == np.float32
    return a.astype(np.float64)


def turn_back(K, delta, inv_freq32):
    """K [..., d] (float64) turned back by delta positions: x1' = x1 c + x2 s, x2' = x2 c - x1 s over the pairs (e, e + d/2)"""
    K = np.asarray(K, dtype=np.float64)
    half = K.shape[-1] // 2
    a = angles(delta, inv_freq32)
    assert a.shape == (half,)
    c, s = np.cos(a), np.sin(a)
    x1, x2 = K[..., :half], K[..., half:]
    return np.concatenate([x1 * c + x2 * s, x2 * c - x1 * s], -1)


def drop_shift(K, V, frm, to, inv_freq32):
    """-> (K' float64 [..., n - delta, d], V' [..., n - delta, d] with V's own dtype and bits)"""
    K, V = np.asarray(K, dtype=np.float64), np.asarray(V)
    n = K.shape[-2]
    assert 0 <= frm <= to <= n and V.shape == K.shape
    Kn = np.concatenate([K[..., :frm, :], turn_back(K[..., to:, :], to - frm, inv_freq32) if to > frm else K[..., to:, :]], -2)
    Vn = np.concatenate([V[..., :frm, :], V[..., to:, :]], -2)
    return Kn, Vn


def pair_norm(K):
    """hypot(x1, x2) of every element's pair, in K's shape (float64)"""
    K = np.asarray(K, dtype=np.float64)
    half = K.shape[-1] // 2
    h = np.hypot(K[..., :half], K[..., half:])
    return np.concatenate([h, h], -1)


# One rounding to the storage type (u: bf16 keeps 8 significant bits, so half an ulp is up to 2^-8 of the value -- the bound is met, not just approached; fp32's half ulp
# is 2^-24, under u = 2^-23) and the fp32 evaluation in units of 2^-24 hypot(x1, x2):
# two products (|x1 c| + |x2 s| <= hypot: 1), one sum (1), and cosf / sinf at k ulp each (k sqrt(2), an ulp of a value below 1 being at most 2^-24).  8 covers k = 4,
# the bound of OpenCL's full profile for sin / cos, which the device library's sinf / cosf are built to meet (HIP's own table of ulp figures was not at hand when this was
# written: the constant is held against that published bound, not against a measurement; 2 ulp would need 4.9 of the 8).
U = {'bf16': 2.0 ** -8, 'fp32': 2.0 ** -23}
EVAL = 8 * 2.0 ** -24


def bound(exact, source_pair_norm, kind):
    """the allowed |got - exact| per element: exact = the oracle's rotated keys, source_pair_norm = pair_norm of the keys before the rotation (the rotation keeps it)"""
    return U[kind] * np.abs(exact) + EVAL * source_pair_norm
