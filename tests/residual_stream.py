"""The rounding points of the residual stream, restated on the host (plain torch; imports and runs without a GPU).

Between two GEMMs of a decoder layer a step writes the bf16 residual stream h and its RMSNorm image.  Three pieces of code do that, by schedule:
  tile    the EPI_RESID epilogue of the tile / ring / big GEMMs, then rmsnorm_kernel / rmsnorm_rows_kernel          (tests/test_gpu_ops.py, tests/test_gpu_stress_gemm.py)
  slabs   slab_resid_rmsnorm_kernel<4 / 8 / 16>, with or without wscale                                              (mmd_op_slab_resid_rmsnorm)
  chain   producer side of gemm_gemv16_kernel<.., CHAIN> (h, ssq), consumer side of the same kernel (per lane)    (mmd_op_gemv_chain)
All of them are specified as

    h  = rnd(rnd(gemm * wscale) + h)              gemm: fp32, K slabs summed 0, 1, 2, ... one add at a time
    xn = rnd(gamma * rnd(h * inv)),               inv = rsqrt(mean(h^2) + eps)        (Qwen2RMSNorm's rounding points)

tests/test_gpu_residual_stream.py holds the second and third row to the functions below; tests/test_residual_stream_host.py checks the restatement itself.  The case
lists of the GPU tests live here too, so that the host test can check what they cover."""
import math
import torch

BF = torch.bfloat16
U = 2.0 ** -8                 # bf16's relative rounding error (half an ulp)
TIE = 2.0 ** -20              # how close (relative) to a rounding tie the float64 value may lie before either neighbour is accepted; also the floor, x max|gamma|
SSQ_REL = 2.0 ** -19          # a tile's sum of squares: 16 non-negative fp32 products and 15 adds, contracted or not: (1 + 2^-24)^16 - 1 < 2^-20, and the reference's own fp32 rounding
SSQ_STRIDE, CHAIN_ROWS = 256, 4          # GEMV_SSQ_STRIDE, GEMV_CHAIN_ROWS of csrc/gemm_plan.h
OP_PLAN_SLAB_RESID = 32                  # csrc/common.h: what mmd_op_gemm_last_plan reports first after mmd_op_slab_resid_rmsnorm


# ---- h ----------------------------------------------------------------------------------------------------------------------------------------------------
def slab_resid(slabs, resid, wscale=None, order=None):
    """h = rnd(rnd((slab 0 + slab 1 + ...) * wscale) + resid): fp32 adds one at a time in `order` (default 0, 1, 2, ...), one fp32 multiply, a rounding to bf16, one fp32 add, a
    rounding.  Every step is a single IEEE operation and the rounding sits between the multiply and the add (nothing can contract), so a kernel's h equals this bit for bit.
    slabs fp32 [splits, M, H], resid bf16 [M, H], wscale fp32 [H] or None."""
    order = list(range(slabs.shape[0])) if order is None else list(order)
    acc = slabs[order[0]].float().clone()
    for s in order[1:]:
        acc = acc + slabs[s].float()
    if wscale is not None:
        acc = acc * wscale.float()
    return (acc.to(BF).float() + resid.float()).to(BF)


# ---- the RMSNorm image ------------------------------------------------------------------------------------------------------------------------------------
def rms_candidates(x, gamma, eps, rounded=True):
    """float64 gamma * rnd(x * inv) with inv in float64, for the value itself and for the value moved by -+ TIE (relative) before the rounding: where the float64 value lies
    within TIE of a rounding tie the three differ, and either neighbour is right.  rounded=False (fp32 kernels): no inner rounding, three equal candidates."""
    xd, wd = x.double(), gamma.double()
    xn = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)
    return [wd * ((xn * (1 + s * TIE)).to(BF).double() if rounded else xn) for s in (-1, 0, 1)]


def rms_excess(y, cands, rel, floor):
    """element-wise |y - c| - (rel |c| + floor), for the candidate c that suits y best: y is right where this is <= 0"""
    y = y.double()
    return torch.stack([(y - c).abs() - (rel * c.abs() + floor) for c in cands]).amin(0)


def rms_image(h, gamma, eps):
    """-> (ref, tol) for a bf16 kernel's rnd(gamma * rnd(h * inv)): ref = gamma * rnd(h * inv) in float64, tol = 2^-8 |ref| + 2^-20 max|gamma|.  (Elements near a tie of the inner
    rounding have a second right answer: rms_ties flags them, rms_image_excess accepts both.)"""
    ref = rms_candidates(h, gamma, eps)[1]
    return ref, U * ref.abs() + TIE * gamma.double().abs().max().item()


def rms_ties(h, gamma, eps):
    """bool [M, H]: the float64 value of h * inv lies within TIE of a bf16 rounding tie"""
    lo, mid, hi = rms_candidates(h, gamma, eps)
    return (lo != mid) | (hi != mid)


def rms_image_excess(y, h, gamma, eps):
    """rms_image's rule with the tie allowance, element-wise: y is right where this is <= 0"""
    return rms_excess(y, rms_candidates(h, gamma, eps), U, TIE * gamma.double().abs().max().item())


# ---- the chain's sums of squares --------------------------------------------------------------------------------------------------------------------------
def tile_ssq(h, N=None):
    """fp32 [M, N / 16]: sum of h^2 per 16-column tile, summed in float64"""
    N = h.shape[1] if N is None else N
    return h[:, :N].double().pow(2).view(h.shape[0], N // 16, 16).sum(-1).float()


def wave_k(K, splits, fp8):
    """K elements per wave of a consumer GEMV as the kernel divides them: k-tiles of 32 (fp8: pairs of tiles) over the K splits, then over the 4 waves, both rounded up"""
    kg = 2 if fp8 else 1
    cdiv = lambda a, b: -(-a // b)
    return cdiv(cdiv(K // 32 // kg, splits), 4) * 32 * kg


def ragged(K, splits, fp8):
    """the last wave's K range is shorter than the others' (or empty)"""
    return (K // 32 // (2 if fp8 else 1)) % (4 * splits) != 0


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------
def order_sensitive_slabs(splits, M, H, seed, device='cpu'):
    """fp32 [splits, M, H]: 0.7 randn everywhere; slabs 0 .. 2 ((splits - 1) // 2) - 1 carry (-1)^s 1e4 on top -- an even number of them, so that neighbouring large terms
    cancel and the sum is O(1) -- and the last slab (with an even count, the last two) only the small values.  Summed 0, 1, 2, ... the large pairs cancel first and the small
    terms keep their low bits; in any other order small terms are added to 1e4 (ulp 2^-10) and lose them: the order decides the low bits of the sum, hence roundings of h."""
    g = torch.Generator(device=device).manual_seed(seed)
    s = 0.7 * torch.randn(splits, M, H, generator=g, device=device)
    for i in range(2 * ((splits - 1) // 2)):
        s[i] += 1e4 * (-1) ** i
    return s


def slab_inputs(splits, M, H, seed, device='cpu'):
    """-> (slabs, resid bf16 [M, H] at scale 3, gamma bf16 [H] = 1 + 0.1 randn, wscale fp32 [H] in 2^-9 .. 2^-5).  From three rows on, row 1 carries one element at 1e4 and
    row 2 is all zeros (slabs and residual): eps decides its norm."""
    g = torch.Generator(device=device).manual_seed(seed + 1)
    slabs = order_sensitive_slabs(splits, M, H, seed, device)
    resid = 3 * torch.randn(M, H, generator=g, device=device)
    gamma = 1 + 0.1 * torch.randn(H, generator=g, device=device)
    wscale = 2.0 ** -9 * (1 + 15 * torch.rand(H, generator=g, device=device))
    if M >= 3:
        resid[1, (977 + 5) % H] = 1e4
        slabs[:, 2] = 0; resid[2] = 0
    return slabs, resid.to(BF), gamma.to(BF), wscale


ROW_SCALES = (1e-2, 1.0, 30.0, 1e3)          # rows of a consumer's h: a 1/rms taken from another row is off by 30 x at least


def chain_h(M, K, seed, device='cpu'):
    """-> (h bf16 [M, K] with row r at ROW_SCALES[r], gamma bf16 [K] = 1 + 0.1 randn)"""
    g = torch.Generator(device=device).manual_seed(seed)
    h = torch.randn(M, K, generator=g, device=device) * torch.tensor(ROW_SCALES[:M], device=device)[:, None]
    gamma = 1 + 0.1 * torch.randn(K, generator=g, device=device)
    return h.to(BF), gamma.to(BF)


# ---- the cases of tests/test_gpu_residual_stream.py ----------------------------------------------------------------------------------------------------------
SLAB_SPLITS = (1, 2, 4, 5, 8, 9, 16)          # both sides of 4 | 5 and 8 | 9, the top of <16>
SLAB_MAXS = {1: 4, 2: 4, 4: 4, 5: 8, 8: 8, 9: 16, 16: 16}          # the instantiation each must launch (last_plan)
SLAB_MS = (1, 3, 64)
SLAB_HS = (72, 1024, 1028, 3584, 4096)        # under one column group of 1024, exactly one, one plus 4 columns, the model's, the kernel's limit
SLAB_REFUSED = (dict(splits=17), dict(H=4100), dict(H=70), dict(splits=0))

PRODUCER_MS = (1, 2, 4)
# (name, N, K, fp8, X): o_proj, down_proj, the ssq limit (256 n-tiles) with a K shorter than the 16 waves (2 k-tiles: 14 waves idle), a single tile
PRODUCER_CASES = [('o', 3584, 3584, False, 'outlier'), ('o_w8', 3584, 3584, True, 'outlier'), ('down', 3584, 18944, False, 'randn'), ('down_w8', 3584, 18944, True, 'randn'),
                  ('ssq_limit', 4096, 64, False, 'randn'), ('one_tile', 16, 2048, False, 'randn')]

CONSUMER_MS = (1, 3, 4)
# (name, epi, N, K, fp8, room for slabs) -> (K splits, K per wave, ragged) that last_plan must report / imply.  Split counts 1 and 2; per-wave ranges below 512 (one pass of
# the prologue), above 512 (the second pass runs partly), exactly 1024 (both passes full: the kernel's limit); ragged ranges (the last wave short).  The qkv form runs on one K
# split when its caller has room for one slab only (the planner's own workspace rule; what MMDUET_GEMV_KSPLIT_SHORT=1 makes of the step).
CONSUMER_CASES = {
    ('qkv', 'none', 4608, 3584, False, 4): (2, 448, False),
    ('qkv_w8', 'none', 4608, 3584, True, 4): (2, 448, False),
    ('qkv_k4096', 'none', 512, 4096, False, 4): (2, 512, False),
    ('qkv_k4096_one_slab', 'none', 512, 4096, False, 1): (1, 1024, False),
    ('qkv_k96', 'none', 16, 96, False, 4): (2, 32, True),
    ('gate_up', 'swiglu', 37888, 3584, False, 0): (1, 896, False),
    ('gate_up_w8', 'swiglu', 37888, 3584, True, 0): (1, 896, False),
    ('gate_up_k4096', 'swiglu', 64, 4096, False, 0): (1, 1024, False),
    ('gate_up_k1056', 'swiglu', 32, 1056, False, 0): (1, 288, True),
}
# refused before a launch: (role, M, N, K, room for slabs)
CHAIN_REFUSED = {'consumer_m5': (1, 5, 512, 3584, 4), 'consumer_k8192_one_split': (1, 1, 512, 8192, 1), 'consumer_k4128_one_split': (1, 1, 512, 4128, 1),
                 'producer_n4112': (2, 1, 4112, 3584, 0)}
