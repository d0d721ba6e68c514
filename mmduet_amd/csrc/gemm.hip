// gemm.hip -- Y[M,N] = epilogue(X[M,K] . W[N,K]^T + bias) on MFMA (gfx950), bf16 and fp32.
//
// Stands in for every nn.Linear of the path: Qwen2 q/k/v/o/gate/up/down (transformers qwen2/modeling_qwen2.py:36-48,
// 200-240), lm_head / informative_head / relevance_head (models/live_llava/video_head_live_llava_qwen.py:76-78), SigLIP
// q/k/v/out/fc1/fc2 + the patch-embed conv as im2col GEMM (siglip/modeling_siglip.py:124-186, 250-322) and the
// mm_projector.  W keeps the checkpoint's [out,in] layout, so both operands are K-contiguous ("B^T input").
//
// Operand order is swapped (acc = mfma(W_frag, X_frag)): a lane then owns 4 CONSECUTIVE n for one m, so the epilogue
// reads bias/residual and writes the result as one 8-byte (bf16) / 16-byte (fp32) access per 16x16 tile.
//
// Rounding points follow eager bf16 execution of the reference: linear output rounded to the storage type before the
// activation / residual add / gate*up product (no-ops in fp32).
#include "common.h"
#include <type_traits>

#include "gemm_ring.h"

template <typename T> struct Frag;
template <> struct Frag<bf16_t> { using type = bf16x8_t; static constexpr int KSTEP = 32; };
template <> struct Frag<float> { using type = float; static constexpr int KSTEP = 4; };

template <typename T, int BM, int BN> struct TileCfg {
    static constexpr int BK = 32;
    static constexpr int PAD = sizeof(T) == 2 ? 8 : 1;
    static constexpr int LD = BK + PAD;
    static constexpr int WM = BM / 2, WN = BN / 2;      // 2x2 waves
    static constexpr int TM = WM / 16, TN = WN / 16;
};

// cooperative, bounds-checked load of a [ROWS][32] tile (rows r0.., cols k0..) into LDS (zero-filled outside)
template <typename T, int ROWS, int LD>
__device__ __forceinline__ void stage_tile(T* __restrict__ lds, const T* __restrict__ g, long long ld, int r0, int nrows, int k0, int kend,
                                           int vec, int tid) {
    if constexpr (sizeof(T) == 2) {
        // 4 chunks of 8 elements per row
        for (int i = tid; i < ROWS * 4; i += 256) {
            int r = i >> 2, c = (i & 3) * 8;
            s16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
            int gr = r0 + r, gk = k0 + c;
            if (gr < nrows && gk < kend) {
                const T* src = g + (long long)gr * ld + gk;
                if (vec && gk + 8 <= kend) {
                    v = *reinterpret_cast<const s16x8_t*>(src);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) if (gk + e < kend) v[e] = (short)src[e];
                }
            }
            *reinterpret_cast<s16x8_t*>(lds + r * LD + c) = v;
        }
    } else {
        for (int i = tid; i < ROWS * 32; i += 256) {
            int r = i >> 5, c = i & 31;
            int gr = r0 + r, gk = k0 + c;
            T v = 0;
            if (gr < nrows && gk < kend) v = g[(long long)gr * ld + gk];
            lds[r * LD + c] = v;
        }
    }
}

template <typename T>
__device__ __forceinline__ void store4(const GemmP& p, int m, int n, const float (&v)[4]) {
    // v = acc (+bias) for columns n..n+3 of row m, epilogues except SWIGLU
    if (m >= p.M) return;
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float x = v[r];
        if (n + r < p.N && p.wscale) x *= p.wscale[n + r];
        if (n + r < p.N && p.bias) x += to_f<T>(((const T*)p.bias)[n + r]);
        if (p.epi == EPI_GELU_TANH) x = gelu_tanh_t<T>(rnd<T>(x));
        else if (p.epi == EPI_GELU_ERF) x = gelu_erf_t<T>(rnd<T>(x));
        else if (p.epi == EPI_RESID) { if (n + r < p.N) x = rnd<T>(x) + to_f<T>(((const T*)p.R)[(long long)m * p.ldr + n + r]); }
        o[r] = x;
    }
    if (p.out_f32) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = rnd<T>(o[r]);
        float* y = (float*)p.Y + (long long)m * p.ldy + n;
        if (n + 3 < p.N && ((p.ldy & 3) == 0)) *reinterpret_cast<f32x4_t*>(y) = f32x4_t{o[0], o[1], o[2], o[3]};
        else { for (int r = 0; r < 4; ++r) if (n + r < p.N) y[r] = o[r]; }
    } else {
        T* y = (T*)p.Y + (long long)m * p.ldy + n;
        if (n + 3 < p.N && ((p.ldy & 3) == 0)) {
            if constexpr (sizeof(T) == 2) {
                s16x4_t pk = {(short)f2bf(o[0]), (short)f2bf(o[1]), (short)f2bf(o[2]), (short)f2bf(o[3])};
                *reinterpret_cast<s16x4_t*>(y) = pk;
            } else {
                *reinterpret_cast<f32x4_t*>(y) = f32x4_t{o[0], o[1], o[2], o[3]};
            }
        } else { for (int r = 0; r < 4; ++r) if (n + r < p.N) y[r] = from_f<T>(o[r]); }
    }
}

template <typename T>
__device__ __forceinline__ void store4_swiglu(const GemmP& p, int m, int n_gate, const float (&g)[4], const float (&u)[4]) {
    // interleaved layout: columns [32j, 32j+16) = gate rows 16j.., [32j+16, 32j+32) = up rows 16j..
    if (m >= p.M) return;
    int oc = (n_gate >> 5) * 16 + (n_gate & 15);
    int NO = p.N >> 1;
    T* y = (T*)p.Y + (long long)m * p.ldy + oc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (oc + r < NO) {
            float gs = g[r], us = u[r];
            if (p.wscale) { gs *= p.wscale[n_gate + r]; us *= p.wscale[n_gate + 16 + r]; }
            float gg = rnd<T>(gs), uu = rnd<T>(us);
            float s = rnd<T>(silu_t<T>(gg));
            y[r] = from_f<T>(s * uu);
        }
    }
}

template <typename T, int BM, int BN>
__global__ __launch_bounds__(256) void gemm_tile_kernel(GemmP p) {
    using C = TileCfg<T, BM, BN>;
    using F = Frag<T>;
    __shared__ __attribute__((aligned(16))) T Xs[BM * C::LD];
    __shared__ __attribute__((aligned(16))) T Ws[BN * C::LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * C::WM, wn = (wave & 1) * C::WN;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int kbeg = blockIdx.z * p.kper;
    const int kend = min(p.K, kbeg + p.kper);
    const int lr = lane & 15, lq = lane >> 4;

    f32x4_t acc[C::TM][C::TN];
#pragma unroll
    for (int i = 0; i < C::TM; ++i)
#pragma unroll
        for (int j = 0; j < C::TN; ++j) acc[i][j] = f32x4_t{0, 0, 0, 0};

    for (int k0 = kbeg; k0 < kend; k0 += C::BK) {
        __syncthreads();
        stage_tile<T, BM, C::LD>(Xs, (const T*)p.X, p.ldx, m0, p.M, k0, kend, p.vec, tid);
        stage_tile<T, BN, C::LD>(Ws, (const T*)p.W, p.ldw, n0, p.N, k0, kend, p.vec, tid);
        __syncthreads();
        if constexpr (sizeof(T) == 2) {
            bf16x8_t xf[C::TM], wf[C::TN];
#pragma unroll
            for (int i = 0; i < C::TM; ++i) xf[i] = *reinterpret_cast<const bf16x8_t*>(Xs + (wm + i * 16 + lr) * C::LD + lq * 8);
#pragma unroll
            for (int j = 0; j < C::TN; ++j) wf[j] = *reinterpret_cast<const bf16x8_t*>(Ws + (wn + j * 16 + lr) * C::LD + lq * 8);
#pragma unroll
            for (int i = 0; i < C::TM; ++i)
#pragma unroll
                for (int j = 0; j < C::TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[i], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
            for (int kk = 0; kk < C::BK; kk += 4) {
                float xf[C::TM], wf[C::TN];
#pragma unroll
                for (int i = 0; i < C::TM; ++i) xf[i] = Xs[(wm + i * 16 + lr) * C::LD + kk + lq];
#pragma unroll
                for (int j = 0; j < C::TN; ++j) wf[j] = Ws[(wn + j * 16 + lr) * C::LD + kk + lq];
#pragma unroll
                for (int i = 0; i < C::TM; ++i)
#pragma unroll
                    for (int j = 0; j < C::TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[j], xf[i], acc[i][j], 0, 0, 0);
            }
        }
    }

    // epilogue: lane holds C[m = .. + lr][n = .. + lq*4 + r]
    if (gridDim.z > 1) {
        float* ws = p.ws + (long long)blockIdx.z * p.M * p.N;
#pragma unroll
        for (int i = 0; i < C::TM; ++i)
#pragma unroll
            for (int j = 0; j < C::TN; ++j) {
                int m = m0 + wm + i * 16 + lr, n = n0 + wn + j * 16 + lq * 4;
                if (m < p.M) {
                    float* y = ws + (long long)m * p.N + n;
                    if (n + 3 < p.N && (p.N & 3) == 0) *reinterpret_cast<f32x4_t*>(y) = acc[i][j];
                    else for (int r = 0; r < 4; ++r) if (n + r < p.N) y[r] = acc[i][j][r];
                }
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < C::TM; ++i) {
        int m = m0 + wm + i * 16 + lr;
        if (p.epi == EPI_SWIGLU) {
#pragma unroll
            for (int j = 0; j < C::TN; j += 2) {
                int n = n0 + wn + j * 16 + lq * 4;
                float g[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                float u[4] = {acc[i][j + 1][0], acc[i][j + 1][1], acc[i][j + 1][2], acc[i][j + 1][3]};
                store4_swiglu<T>(p, m, n, g, u);
            }
        } else {
#pragma unroll
            for (int j = 0; j < C::TN; ++j) {
                int n = n0 + wn + j * 16 + lq * 4;
                float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                store4<T>(p, m, n, v);
            }
        }
    }
}

// sums split-K slabs and applies the epilogue; one thread per 4 consecutive columns
template <typename T>
__global__ void splitk_reduce_kernel(GemmP p, int splits) {
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int n4 = (p.N + 3) / 4;
    if (idx >= (long long)p.M * n4) return;
    int m = (int)(idx / n4), n = (int)(idx % n4) * 4;
    if (p.epi == EPI_SWIGLU) {
        // handle a gate quad; its up partner sits 16 columns further
        if ((n & 16) != 0) return;
        float g[4] = {0, 0, 0, 0}, u[4] = {0, 0, 0, 0};
        for (int s = 0; s < splits; ++s) {
            const float* w = p.ws + ((long long)s * p.M + m) * p.N + n;
            for (int r = 0; r < 4; ++r) { if (n + r < p.N) g[r] += w[r]; if (n + 16 + r < p.N) u[r] += w[16 + r]; }
        }
        store4_swiglu<T>(p, m, n, g, u);
        return;
    }
    float v[4] = {0, 0, 0, 0};
    for (int s = 0; s < splits; ++s) {
        const float* w = p.ws + ((long long)s * p.M + m) * p.N + n;
        for (int r = 0; r < 4; ++r) if (n + r < p.N) v[r] += w[r];
    }
    store4<T>(p, m, n, v);
}

// ------------------------------------------------------------------------------------------------------------------
// Weight-streaming GEMM for M <= 16*MT rows (the per-frame LLM step, M ~ 49, and M = 1 decoding): HBM-bound, every
// weight byte is read exactly once.
//   * W is stored MFMA-fragment-major ("packed", pack_w16x32_kernel): tile (nt, kt) = 16 rows x 32 k is one contiguous
//     1 KiB block whose 16-byte piece `lane` is exactly that lane's A operand.  A wave streams its n-tile along K with
//     one fully coalesced 1 KiB non-temporal load per MFMA k-step, straight into VGPRs (no LDS round trip for the
//     operand that is used once).
//   * X [M,K] (L2-resident, re-read by every block) is staged through LDS once per block in full 256-byte row pieces
//     and shared by the 4 waves; the LDS image is fragment-ordered with an XOR on the row index so that both the
//     row-contiguous ds_write_b128 and the fragment ds_read_b128 are bank-conflict-free.
//   * 4 waves = 4*NT n-tiles per block; K is split over grid.y into fp32 slabs when N alone cannot fill 256 CUs
//     (deterministic slab reduce, no atomics).
// ------------------------------------------------------------------------------------------------------------------
__global__ void pack_w16x32_kernel(const bf16_t* __restrict__ W, long long ldw, int N, int K, bf16_t* __restrict__ out) {
    // one thread per 16-byte piece: out[((nt*KT + kt)*64 + lane)*8 + e] = W[nt*16 + (lane&15)][kt*32 + (lane>>4)*8 + e]
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int KT = K >> 5;
    long long pieces = (long long)(N >> 4) * KT * 64;
    if (i >= pieces) return;
    int lane = (int)(i & 63);
    long long tile = i >> 6;
    int kt = (int)(tile % KT);
    long long nt = tile / KT;
    const bf16_t* src = W + (nt * 16 + (lane & 15)) * ldw + kt * 32 + (lane >> 4) * 8;
    *reinterpret_cast<s16x8_t*>(out + i * 8) = *reinterpret_cast<const s16x8_t*>(src);
}

hipError_t launch_pack_w(const void* W, int64_t ldw, int N, int K, void* out, hipStream_t st) {
    long long pieces = (long long)(N >> 4) * (K >> 5) * 64;
    if (pieces <= 0) return hipSuccess;
    hipLaunchKernelGGL(pack_w16x32_kernel, dim3(cdiv(pieces, 256)), dim3(256), 0, st, (const bf16_t*)W, (long long)ldw, N, K, (bf16_t*)out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// fp8 e4m3 (OCP e4m3fn) weight path (BASELINE configs[4]: "fp8 MFMA weights"; SURVEY.md section 8d row 5: per-channel-scaled
// weights, bf16 activations, fp32 accumulate).  gfx950's plain fp8 MFMA runs at the bf16 rate and would need fp8 ACTIVATIONS, so the
// gain is bytes, not FLOPs: the weight-streaming kernels (M <= 64: decode GEMV, per-frame steps) read the 1-byte copy and widen it to
// bf16 in registers (v_cvt_scalef32_pk_bf16_fp8, exact), the MFMA-bound tile kernels keep reading a bf16 copy of the SAME values q.
// Every regime computes (sum_k x_k q_nk) * scale_n with exact products and fp32 accumulation, so the chunked and the per-frame schedule
// still agree up to accumulation order.  scale_n = amax_n / 448, q = round-to-nearest-even(W / scale_n) (v_cvt_pk_fp8_f32).
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void quantize_fp8_rows_kernel(bf16_t* __restrict__ W, int K, uint8_t* __restrict__ q8, float* __restrict__ scale) {
    __shared__ float red[4];
    const long long row = blockIdx.x;
    bf16_t* w = W + row * K;
    float amax = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) amax = fmaxf(amax, fabsf(bf2f(w[k])));
    amax = wave_max(amax);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float sc = amax > 0.f ? amax / 448.0f : 1.0f;
    if (threadIdx.x == 0) scale[row] = sc;
    for (int k = threadIdx.x * 2; k < K; k += 512) {                // K is even
        const float a = bf2f(w[k]) / sc, b = bf2f(w[k + 1]) / sc;   // true division: the host reference does W / scale
        const int pk = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
        q8[row * K + k] = (uint8_t)(pk & 0xff); q8[row * K + k + 1] = (uint8_t)((pk >> 8) & 0xff);
        const auto back = __builtin_amdgcn_cvt_pk_f32_fp8(pk, false);
        w[k] = f2bf(back[0]); w[k + 1] = f2bf(back[1]);             // e4m3 has 3 mantissa bits: exact in bf16
    }
}
hipError_t launch_quantize_fp8_rows(void* W, int N, int K, uint8_t* q8, float* scale, hipStream_t st) {
    if (N <= 0 || (K & 1)) return N <= 0 ? hipSuccess : hipErrorInvalidValue;
    hipLaunchKernelGGL(quantize_fp8_rows_kernel, dim3(N), dim3(256), 0, st, (bf16_t*)W, K, q8, scale);
    return hipGetLastError();
}
// fragment-major fp8 layout: block (nt, kp) = 16 rows x 64 k = 1 KiB; lane l's 16 bytes = row (l & 15), k = kp*64 + (l >> 4)*8 + {0..7} (the
// A operand of k-step 2kp) followed by k = kp*64 + 32 + (l >> 4)*8 + {0..7} (k-step 2kp + 1): one coalesced 1 KiB load feeds two MFMAs
__global__ void pack_w8_kernel(const uint8_t* __restrict__ q8, int N, int K, uint8_t* __restrict__ out) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int KP = K >> 6;
    const long long pieces = (long long)(N >> 4) * KP * 64;
    if (i >= pieces) return;
    const int lane = (int)(i & 63);
    const long long blk = i >> 6;
    const int kp = (int)(blk % KP);
    const long long nt = blk / KP;
    const uint8_t* src = q8 + (nt * 16 + (lane & 15)) * (long long)K + kp * 64 + (lane >> 4) * 8;
    uint2 lo = *reinterpret_cast<const uint2*>(src), hi = *reinterpret_cast<const uint2*>(src + 32);
    *reinterpret_cast<uint4*>(out + i * 16) = uint4{lo.x, lo.y, hi.x, hi.y};
}
hipError_t launch_pack_w8(const uint8_t* q8, int N, int K, void* out, hipStream_t st) {
    const long long pieces = (long long)(N >> 4) * (K >> 6) * 64;
    if (pieces <= 0) return hipSuccess;
    hipLaunchKernelGGL(pack_w8_kernel, dim3(cdiv(pieces, 256)), dim3(256), 0, st, q8, N, K, (uint8_t*)out);
    return hipGetLastError();
}
// 8 fp8 (two dwords) -> 8 bf16, exact
__device__ __forceinline__ bf16x8_t fp8x8_to_bf16(unsigned lo, unsigned hi) {
    typedef __attribute__((ext_vector_type(2))) __bf16 b2;
    const b2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)lo, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)lo, 1.0f, true);
    const b2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)hi, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)hi, 1.0f, true);
    return bf16x8_t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

__device__ __forceinline__ int xs_slot(int ktl, int kq, int r) { return kq * 16 + (r ^ (kq + 4 * (ktl & 1))); }

template <int MT, int NT, bool W8 = false>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(GemmP p, int KT, int kt_per_split) {
    constexpr int KS = 4;                                   // k-tiles (of 32) per pipeline step
    __shared__ __attribute__((aligned(16))) bf16_t Xs[2][MT * KS * 64 * 8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ntiles = p.N >> 4;
    const int nt0 = (blockIdx.x * 4 + wave) * NT;
    const int kt_beg = blockIdx.y * kt_per_split;
    const int kt_end = min(KT, kt_beg + kt_per_split);
    const bf16_t* X = (const bf16_t*)p.X;
    const bf16_t* Wp = (const bf16_t*)p.W;

    f32x4_t acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4_t{0, 0, 0, 0};

    bf16x8_t wc[NT][KS], wn[NT][KS];
    s16x8_t xr[MT];

    auto load_w = [&](bf16x8_t (&w)[NT][KS], int kt) {
        if constexpr (W8) {
            // fp8 copy: one 16-byte piece per lane = the operands of two k-steps (kt is a multiple of 4 here, K % 64 == 0)
            const uint8_t* W8p = (const uint8_t*)p.W;
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int s = 0; s < KS; s += 2) {
                    u32x4_t v = {0, 0, 0, 0};
                    if (nt0 + j < ntiles && kt + s < kt_end)
                        v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(W8p + (((long long)(nt0 + j) * (KT >> 1) + ((kt + s) >> 1)) * 64 + lane) * 16));
                    w[j][s] = fp8x8_to_bf16(v[0], v[1]); w[j][s + 1] = fp8x8_to_bf16(v[2], v[3]);
                }
            return;
        }
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                s16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (nt0 + j < ntiles && kt + s < kt_end)
                    v = __builtin_nontemporal_load(reinterpret_cast<const s16x8_t*>(Wp + (((long long)(nt0 + j) * KT + kt + s) * 64 + lane) * 8));
                w[j][s] = __builtin_bit_cast(bf16x8_t, v);
            }
    };
    auto load_x = [&](int kt) {
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            int i = tid + 256 * j, m = i >> 4, c = i & 15;
            s16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (m < p.M && kt + (c >> 2) < kt_end) v = *reinterpret_cast<const s16x8_t*>(X + (long long)m * p.ldx + kt * 32 + c * 8);
            xr[j] = v;
        }
    };
    auto write_x = [&](int buf) {
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            int i = tid + 256 * j, m = i >> 4, c = i & 15;
            int mt = m >> 4, r = m & 15, ktl = c >> 2, kq = c & 3;
            *reinterpret_cast<s16x8_t*>(&Xs[buf][((mt * KS + ktl) * 64 + xs_slot(ktl, kq, r)) * 8]) = xr[j];
        }
    };

    load_w(wc, kt_beg);
    load_x(kt_beg);
    write_x(0);
    __syncthreads();
    int cur = 0;
    for (int kt = kt_beg; kt < kt_end; kt += KS) {
        const bool more = kt + KS < kt_end;
        if (more) { load_w(wn, kt + KS); load_x(kt + KS); }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if (kt + s < kt_end) {
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    bf16x8_t xf = *reinterpret_cast<const bf16x8_t*>(&Xs[cur][((i * KS + s) * 64 + xs_slot(s, lq, lr)) * 8]);
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wc[j][s], xf, acc[i][j], 0, 0, 0);
                }
            }
        }
        if (more) write_x(cur ^ 1);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int s = 0; s < KS; ++s) wc[j][s] = wn[j][s];
        cur ^= 1;
    }

    if (gridDim.y > 1 || p.slabs) {
        float* ws = p.ws + (long long)blockIdx.y * p.M * p.N;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                int m = i * 16 + lr, n = (nt0 + j) * 16 + lq * 4;
                if (m < p.M && nt0 + j < ntiles) {
                    f32x4_t v = acc[i][j];
                    if (p.slabs && p.wscale) v *= *reinterpret_cast<const f32x4_t*>(p.wscale + n);      // the fused slab consumers know no scale (split-K reduce applies it itself)
                    *reinterpret_cast<f32x4_t*>(ws + (long long)m * p.N + n) = v;
                }
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        int m = i * 16 + lr;
        if (p.epi == EPI_SWIGLU) {
            if constexpr (NT >= 2) {
#pragma unroll
                for (int j = 0; j < NT; j += 2) {
                    if (nt0 + j + 1 < ntiles) {
                        int n = (nt0 + j) * 16 + lq * 4;
                        float g[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                        float u[4] = {acc[i][j + 1][0], acc[i][j + 1][1], acc[i][j + 1][2], acc[i][j + 1][3]};
                        store4_swiglu<bf16_t>(p, m, n, g, u);
                    }
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if (nt0 + j < ntiles) {
                    int n = (nt0 + j) * 16 + lq * 4;
                    float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                    store4<bf16_t>(p, m, n, v);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// M <= 16 (decode, M = 1): pure weight streaming.  A block owns NT n-tiles; its 4 waves split K four ways and each
// wave streams its part of the packed W with U independent 1 KiB non-temporal loads in flight (no LDS, no barrier in
// the loop -- "GEMV: load straight to VGPRs, deep unroll, late wait").  X rows (<= 16, L2-resident) are read as MFMA
// operands directly.  The four partial accumulators meet in LDS once; wave 0 applies the epilogue (or leaves ONE fp32
// slab for the fused consumer): no split-K slabs, no reduce launch.
// ------------------------------------------------------------------------------------------------------------------
// x fragment of the decode chain: rnd(gamma * rnd(h * inv)) (Qwen2RMSNorm's rounding points)
__device__ __forceinline__ s16x8_t chain_norm8(const s16x8_t& h, const s16x8_t& g, float inv) {
    s16x8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (short)f2bf(bf2f((bf16_t)g[e]) * bf2f(f2bf(bf2f((bf16_t)h[e]) * inv)));
    return o;
}

template <int NT, int U, bool W8 = false, bool CHAIN = false, int WAVES = 4>
__global__ __launch_bounds__(WAVES * 64) void gemm_gemv16_kernel(GemmP p, int KT, GemvChain ch) {
    __shared__ __attribute__((aligned(16))) float red[WAVES - 1][NT][64][4];
    // consumer side of the decode chain: each wave keeps the normalised activation of ITS K range here (rows <= GEMV_CHAIN_ROWS, <= 1024 k per wave)
    constexpr int XW = 1024;
    __shared__ __attribute__((aligned(16))) bf16_t xs[(CHAIN && WAVES == 4) ? WAVES * GEMV_CHAIN_ROWS * XW : 8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int nt0 = blockIdx.x * NT;
    // K range of this block (grid.y splits K into slabs when N alone gives too few blocks), then of this wave; in k-tiles of 32 (fp8: pairs of tiles)
    constexpr int KG = W8 ? 2 : 1;
    const int KTg = KT / KG;
    const int ktb = (KTg + gridDim.y - 1) / gridDim.y;
    const int blk_beg = blockIdx.y * ktb, blk_end = min(KTg, blk_beg + ktb);
    const int ktw = (blk_end - blk_beg + WAVES - 1) / WAVES;
    const int kt_beg = blk_beg + wave * ktw, kt_end = min(blk_end, kt_beg + ktw);      // units of KG k-tiles
    const bool xn = CHAIN && WAVES == 4 && ch.xn_h != nullptr;        // X built from the residual stream (see GemvChain)
    const bf16_t* xrow = (const bf16_t*)p.X + (long long)lr * p.ldx + lq * 8;
    const bf16_t* xl = xs + (wave * GEMV_CHAIN_ROWS + lr) * XW + lq * 8 - kt_beg * (32 * KG);     // + k: this wave's copy of row lr
    const bool row_ok = lr < p.M;

    f32x4_t acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4_t{0, 0, 0, 0};

    // chain prologue, run by each wave AFTER its first weight loads are issued: 1/rms of every row from the producer's per-n-tile partial sums
    // (lane l takes entries 4l..4l+3; fixed order), then rnd(gamma * rnd(h * inv)) of the wave's K range into LDS
    auto chain_prologue = [&]() {
        const int k0 = kt_beg * (32 * KG), kn = (kt_end - kt_beg) * (32 * KG);
        for (int r = 0; r < p.M; ++r) {
            const f32x4_t q = *reinterpret_cast<const f32x4_t*>(ch.xn_ssq + r * GEMV_SSQ_STRIDE + lane * 4);
            s16x8_t hv[2], gv[2];
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                const int k = ps * 512 + lane * 8;
                hv[ps] = s16x8_t{0, 0, 0, 0, 0, 0, 0, 0}; gv[ps] = hv[ps];
                if (k < kn) {
                    hv[ps] = *reinterpret_cast<const s16x8_t*>((const bf16_t*)ch.xn_h + (long long)r * p.K + k0 + k);
                    gv[ps] = *reinterpret_cast<const s16x8_t*>((const bf16_t*)ch.xn_gamma + k0 + k);
                }
            }
            const float inv = rsqrtf(wave_sum((q[0] + q[1]) + (q[2] + q[3])) / (float)p.K + ch.xn_eps);
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                const int k = ps * 512 + lane * 8;
                if (k < kn) *reinterpret_cast<s16x8_t*>(xs + (wave * GEMV_CHAIN_ROWS + r) * XW + k) = chain_norm8(hv[ps], gv[ps], inv);
            }
        }
    };

    if constexpr (W8) {
        // fp8 weights: K ranges are in 64-k pairs; a 1 KiB load feeds two MFMAs; U/2 loads per n-tile in flight
        const uint8_t* W8p = (const uint8_t*)p.W;
        const int KP = KT >> 1;
        constexpr int UP = U / 2;
        auto iter = [&](int kp0, auto first) {
            u32x4_t wv[NT][UP]; bf16x8_t x[UP][2];
#pragma unroll
            for (int u = 0; u < UP; ++u) {
                const int kp = kp0 + u;
                s16x8_t x0 = {0, 0, 0, 0, 0, 0, 0, 0}, x1 = x0;
                if (kp < kt_end) {
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        wv[j][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(W8p + (((long long)(nt0 + j) * KP + kp) * 64 + lane) * 16));
                    if (!xn && row_ok) { x0 = *reinterpret_cast<const s16x8_t*>(xrow + kp * 64); x1 = *reinterpret_cast<const s16x8_t*>(xrow + kp * 64 + 32); }
                } else {
#pragma unroll
                    for (int j = 0; j < NT; ++j) wv[j][u] = u32x4_t{0, 0, 0, 0};
                }
                x[u][0] = __builtin_bit_cast(bf16x8_t, x0); x[u][1] = __builtin_bit_cast(bf16x8_t, x1);
            }
            if constexpr (CHAIN) if (xn) {
                if constexpr (decltype(first)::value) chain_prologue();
#pragma unroll
                for (int u = 0; u < UP; ++u) if (row_ok && kp0 + u < kt_end) {
                    x[u][0] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const s16x8_t*>(xl + (kp0 + u) * 64));
                    x[u][1] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const s16x8_t*>(xl + (kp0 + u) * 64 + 32));
                }
            }
#pragma unroll
            for (int u = 0; u < UP; ++u)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8_to_bf16(wv[j][u][0], wv[j][u][1]), x[u][0], acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8_to_bf16(wv[j][u][2], wv[j][u][3]), x[u][1], acc[j], 0, 0, 0);
                }
        };
        if (kt_beg < kt_end) {
            iter(kt_beg, std::true_type{});
            for (int kp0 = kt_beg + UP; kp0 < kt_end; kp0 += UP) iter(kp0, std::false_type{});
        }
    } else {
        const bf16_t* Wp = (const bf16_t*)p.W;
        auto iter = [&](int kt0, auto first) {
            bf16x8_t w[NT][U], x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kt = kt0 + u;
                s16x8_t xv = {0, 0, 0, 0, 0, 0, 0, 0};
                if (kt < kt_end) {
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        w[j][u] = __builtin_bit_cast(bf16x8_t, __builtin_nontemporal_load(reinterpret_cast<const s16x8_t*>(Wp + (((long long)(nt0 + j) * KT + kt) * 64 + lane) * 8)));
                    if (!xn && row_ok) xv = *reinterpret_cast<const s16x8_t*>(xrow + kt * 32);
                } else {
#pragma unroll
                    for (int j = 0; j < NT; ++j) w[j][u] = __builtin_bit_cast(bf16x8_t, xv);
                }
                x[u] = __builtin_bit_cast(bf16x8_t, xv);
            }
            if constexpr (CHAIN) if (xn) {
                if constexpr (decltype(first)::value) chain_prologue();
#pragma unroll
                for (int u = 0; u < U; ++u) if (row_ok && kt0 + u < kt_end) x[u] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const s16x8_t*>(xl + (kt0 + u) * 32));
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[j][u], x[u], acc[j], 0, 0, 0);
        };
        if (kt_beg < kt_end) {
            iter(kt_beg, std::true_type{});
            for (int kt0 = kt_beg + U; kt0 < kt_end; kt0 += U) iter(kt0, std::false_type{});
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < NT; ++j) *reinterpret_cast<f32x4_t*>(&red[wave - 1][j][lane][0]) = acc[j];
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int w2 = 0; w2 < WAVES - 1; ++w2) acc[j] += *reinterpret_cast<const f32x4_t*>(&red[w2][j][lane][0]);
    const int m = lr;
    if constexpr (CHAIN) if (ch.fin_h) {
        // producer side of the decode chain: the block owns its n-tile over ALL of K (grid.y == 1; the K split is over the block's waves), so the
        // residual add and the tile's sum of squares need no other block -- cross-block hand-over inside a kernel costs an L2 write-back on this part
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            float ss = 0.f;
            if (m < p.M) {
                f32x4_t v = acc[j];
                if (p.wscale) v *= *reinterpret_cast<const f32x4_t*>(p.wscale + (nt0 + j) * 16 + lq * 4);
                bf16_t* hp = (bf16_t*)ch.fin_h + (long long)m * p.N + (nt0 + j) * 16 + lq * 4;
                const s16x4_t r = *reinterpret_cast<const s16x4_t*>(hp);
                s16x4_t o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float hv = bf2f(f2bf(bf2f(f2bf(v[e])) + bf2f((bf16_t)r[e])));      // rnd(rnd(gemm) + residual)
                    ss += hv * hv; o[e] = (short)f2bf(hv);
                }
                *reinterpret_cast<s16x4_t*>(hp) = o;
            }
            ss += __shfl_xor(ss, 16, 64); ss += __shfl_xor(ss, 32, 64);
            if (lq == 0 && m < p.M) ch.fin_ssq[m * GEMV_SSQ_STRIDE + nt0 + j] = ss;
        }
        return;
    }
    if (m >= p.M) return;
    if (p.slabs) {
        float* ws = p.ws + (long long)blockIdx.y * p.M * p.N;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            f32x4_t v = acc[j];
            if (p.wscale) v *= *reinterpret_cast<const f32x4_t*>(p.wscale + (nt0 + j) * 16 + lq * 4);       // slabs feed the fused consumers, which know no scale
            *reinterpret_cast<f32x4_t*>(ws + (long long)m * p.N + (nt0 + j) * 16 + lq * 4) = v;
        }
        return;
    }
    if (p.epi == EPI_SWIGLU) {
        if constexpr (NT >= 2) {
#pragma unroll
            for (int j = 0; j < NT; j += 2) {
                float g[4] = {acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
                float u[4] = {acc[j + 1][0], acc[j + 1][1], acc[j + 1][2], acc[j + 1][3]};
                store4_swiglu<bf16_t>(p, m, (nt0 + j) * 16 + lq * 4, g, u);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            float v[4] = {acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
            store4<bf16_t>(p, m, (nt0 + j) * 16 + lq * 4, v);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// gemm_stream_kernel<MT, NT, WK, KS, NB>: the weight-streaming GEMM of the 16 < M <= 256 regime (round 4) -- the reference's own
// per-frame schedule (M = 49 + prefix, test/inference.py:221-246), the demo path (demo/liveinfer.py:69-105), short chunks and the remainders behind a response.
// Up to M = 256 a forward is bound by the 466 MB of weights a layer streams (16 MFMAs per 1 KB weight tile fill the CU's four SIMDs only at M = 256), yet
// gemm_skinny_kernel reads 3.3-4.6 TB/s at M = 49 and 64 < M <= 256 fell to the 128-row tile kernel (2.4-3.0 x the weight-stream time).  Measured causes
// (profiles/r04_step49_kernels_before.txt): X staged through registers behind the weight loads (waiting for X = vmcnt(0): nothing stays in flight across the step
// barrier), one step of lookahead, and 296 four-wave blocks for gate_up -- most CUs hold 4 waves x 8 KB in flight, below what 25 GB/s per CU needs.
//
//   * block = 4 x WK waves: wave (wn, wk) owns NT n-tiles (16 columns each) and the k-tiles wk * KS .. of every step (the block's K range advances KSB = WK * KS
//     k-tiles per step); all MT m-tiles (M <= 16 MT rows).  The WK partial sums meet in LDS once at the end.
//   * W: packed fragment tiles straight into registers by inline-asm non-temporal loads, LA = NB - 1 steps ahead through NB register buffers (NT * KS KB per wave
//     and step): LA * NT * KS KB in flight per wave at all times.
//   * X: the step's [16 MT rows][32 KSB k] slab by LDS-DMA into an NB-slot ring, in the ring GEMM's piece format (16 rows x 64 B pieces, 16-byte chunk XOR-swizzled:
//     conflict-free b128 fragment reads), issued LA steps ahead like W; every wave reads the fragments of its own k-tiles at use.
//   * ONE hand-counted `s_waitcnt vmcnt((LA - 1) * (NT * KS + XP))` + raw s_barrier per step (W (s) and X (s) were both issued in step s - LA; the LA - 1 steps behind
//     them stay in flight); hipcc sees none of the W loads (inline asm) and never waits for them.
//   * epilogue: fp32 slabs for the fused consumers (reduce + bias + RoPE + append / reduce + residual + RMSNorm), or the SwiGLU / plain epilogues in place.
// ------------------------------------------------------------------------------------------------------------------
template <int N_, typename F> __device__ __forceinline__ void stream_static_for(F&& f) {
    if constexpr (N_ > 0) { stream_static_for<N_ - 1>(f); f(std::integral_constant<int, N_ - 1>{}); }
}

template <int MT, int NT, int WK, int KS, int NB, int WN = 4>
__global__ __launch_bounds__(64 * WN * WK) void gemm_stream_kernel(GemmP p, int KT, int kt_per_block) {
    constexpr int NWAVE = WN * WK, KSB = WK * KS;
    constexpr int XPIECES = MT * KSB;                        // 1 KB pieces of the step's X slab
    constexpr int XP = (XPIECES + NWAVE - 1) / NWAVE;        // LDS-DMAs per wave and step: the SAME count for every wave (the hand-counted waits need that): where the
                                                             // pieces do not divide evenly, the surplus DMAs re-load pieces 0.. (same bytes to the same place)
    constexpr int NWL = NT * KS;                             // W loads per wave and step
    constexpr int LA = NB - 1;
    constexpr int ISSUE = NWL + XP;
    constexpr int VM_STEP = (LA - 1) * ISSUE;
    constexpr int XSLOT = XPIECES * 512;                     // elements per ring slot
    static_assert(VM_STEP <= 63, "vmcnt is a 6-bit counter");
    extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int wn = wave % WN, wk = wave / WN;
    const int ntiles = p.N >> 4;
    const int nt0 = (blockIdx.x * WN + wn) * NT;          // (a wave whose n-tiles lie beyond N streams the last tile again and stores nothing)
    const int kt_beg = blockIdx.y * kt_per_block;
    const int kt_end = min(KT, kt_beg + kt_per_block);
    const int nsteps = (kt_end - kt_beg) / KSB;              // (dispatch condition: every block's K range is a whole number of steps)
    const bf16_t* X = (const bf16_t*)p.X;
    const bf16_t* Wp = (const bf16_t*)p.W;

    // X piece pi = (m-tile pi / KSB, k-tile pi % KSB of the step): lane -> row srow, 16-byte chunk spos ^ sswz (the ring GEMM's piece image)
    const int srow = lane >> 2, spos = lane & 3;
    const int sswz = (0x1230 >> (((srow >> 2) & 3) * 4)) & 3;
    unsigned xo[XP];
#pragma unroll
    for (int j = 0; j < XP; ++j) {
        const int pi = (wave + NWAVE * j) % XPIECES;
        int row = (pi / KSB) * 16 + srow; row = row < p.M ? row : p.M - 1;
        xo[j] = (unsigned)(row * (int)p.ldx + (pi % KSB) * 32 + ((spos ^ sswz) * 8)) * 2u;
    }
    long long wo[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) { int nt = nt0 + j; nt = nt < ntiles ? nt : ntiles - 1; wo[j] = ((long long)nt * KT + kt_beg + wk * KS) * 1024; }
    const unsigned wlane = lane * 16;
    auto dma_x = [&](int slot, int step, int j) {
        const char* ub = (const char*)X + ((long long)kt_beg + (long long)step * KSB) * 64;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ub + xo[j]),
                                         (__attribute__((address_space(3))) void*)(lds + slot * XSLOT + ((wave + NWAVE * j) % XPIECES) * 512), 16, 0, 0);
    };
    auto load_w = [&](bf16x8_t& dst, int j, int ks, int step) {
        const unsigned long long ua = (unsigned long long)(uintptr_t)((const char*)Wp + wo[j] + ((long long)step * KSB + ks) * 1024);
        // (under SGPR pressure hipcc parks uniform values in VGPR lanes; an asm "s" operand cannot take them back -- readfirstlane can)
        const unsigned long long ub = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(ua >> 32)) << 32) |
                                      (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)ua);          // (the builtin returns int: widen as UNSIGNED)
        asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(dst) : "v"(wlane), "s"(ub) : "memory");
    };
    const int rswz = (0x1230 >> (((lr >> 2) & 3) * 4)) & 3;
    const int aoff = lr * 32 + ((lq ^ rswz) * 8);

    f32x4_t acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4_t{0, 0, 0, 0};
    bf16x8_t wb[NB][NT][KS];

    auto issue = [&](int step, auto buf_c) {          // everything step `step` needs, into register buffer / ring slot `buf`
        constexpr int buf = decltype(buf_c)::value;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) load_w(wb[buf][j][ks], j, ks, step);
#pragma unroll
        for (int j = 0; j < XP; ++j) dma_x(buf, step, j);
    };
    // prologue: steps 0 .. LA - 1
    stream_static_for<LA>([&](auto uc) { constexpr int u = decltype(uc)::value; if (u < nsteps) issue(u, std::integral_constant<int, u>{}); });

    auto step = [&](int s, auto buf_c, bool steady) {
        constexpr int cur = decltype(buf_c)::value, nxt = (cur + LA) % NB;
        if (steady) asm volatile("s_waitcnt vmcnt(%0)" :: "i"(VM_STEP) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // tail: the steps behind this one issued less than a full set
        MMD_BAR();
        __builtin_amdgcn_sched_barrier(0);
        if (s + LA < nsteps) issue(s + LA, std::integral_constant<int, nxt>{});
        __builtin_amdgcn_sched_barrier(0);
        const bf16_t* xs = lds + cur * XSLOT;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int ktl = wk * KS + ks;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const bf16x8_t xf = *reinterpret_cast<const bf16x8_t*>(xs + (i * KSB + ktl) * 512 + aoff);
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[cur][j][ks], xf, acc[i][j], 0, 0, 0);
            }
        }
    };
    int s = 0;
    for (; s + NB + LA <= nsteps; s += NB)          // steady periods: every step of the period and the LA - 1 steps behind each issue a full set
        stream_static_for<NB>([&](auto uc) { constexpr int u = decltype(uc)::value; step(s + u, std::integral_constant<int, u>{}, true); });
    for (; s < nsteps; )
        stream_static_for<NB>([&](auto uc) { constexpr int u = decltype(uc)::value; if (s < nsteps) { step(s, std::integral_constant<int, u>{}, s + LA < nsteps); ++s; } });

    // the WK partial sums of a column group meet in LDS (the ring is dead: every wave has read its last slot behind the barrier below)
    if constexpr (WK > 1) {
        __syncthreads();
        float* red = reinterpret_cast<float*>(lds);
        if (wk > 0) {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) *reinterpret_cast<f32x4_t*>(red + ((((wk - 1) * WN + wn) * MT + i) * NT + j) * 256 + lane * 4) = acc[i][j];
        }
        __syncthreads();
        if (wk > 0) return;
#pragma unroll
        for (int w2 = 0; w2 < WK - 1; ++w2)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] += *reinterpret_cast<const f32x4_t*>(red + (((w2 * WN + wn) * MT + i) * NT + j) * 256 + lane * 4);
    }
    if (gridDim.y > 1 || p.slabs) {
        float* ws = p.ws + (long long)blockIdx.y * p.M * p.N;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int m = i * 16 + lr, n = (nt0 + j) * 16 + lq * 4;
                if (m < p.M && nt0 + j < ntiles) {
                    f32x4_t v = acc[i][j];
                    if (p.slabs && p.wscale) v *= *reinterpret_cast<const f32x4_t*>(p.wscale + n);
                    *reinterpret_cast<f32x4_t*>(ws + (long long)m * p.N + n) = v;
                }
            }
        return;
    }
    // (the row loops below are compile-time recursions, not `#pragma unroll`: at MT = 16 the unrolled epilogue passes hipcc's pragma-unroll size limit, the loop stays rolled and `acc` moves to scratch for the whole kernel)
    if (p.epi == EPI_SWIGLU) {
        if constexpr (NT >= 2) {
            stream_static_for<MT>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                const int m = i * 16 + lr;
#pragma unroll
                for (int j = 0; j < NT; j += 2) {
                    if (m < p.M && nt0 + j + 1 < ntiles) {
                        const int n_gate = (nt0 + j) * 16 + lq * 4;
                        *reinterpret_cast<s16x4_t*>((bf16_t*)p.Y + (long long)m * p.ldy + (n_gate >> 5) * 16 + (n_gate & 15)) = big_value_swiglu(acc[i][j], acc[i][j + 1], p.wscale, n_gate);
                    }
                }
            });
        }
        return;
    }
    stream_static_for<MT>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const int m = i * 16 + lr;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            if (nt0 + j < ntiles) {
                float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                store4<bf16_t>(p, m, (nt0 + j) * 16 + lq * 4, v);
            }
        }
    });
}

// ---- launchers ---------------------------------------------------------------------------------------------------
// Each maps a GemmPlan (gemm_plan.h: every split, tile count, grid and instantiation is decided there) to a template instantiation and launches it.
static void launch_reduce(void (*kernel)(GemmP, int), const GemmP& p, int splits, hipStream_t st) {          // the serial slab reduce (slab 0, 1, 2, ... -- the fused consumers' order) applies the epilogue
    long long work = (long long)p.M * ((p.N + 3) / 4);
    hipLaunchKernelGGL(kernel, dim3(cdiv(work, 256)), dim3(256), 0, st, p, splits);
}
static void launch_gemv16(const GemmP& p, const GemmPlan& pl, const GemvChain* chain, hipStream_t st) {
    const int KT = p.K >> 5;
    const GemvChain none;
    const GemvChain& ch = pl.chain != GEMV_PLAIN ? *chain : none;
    const bool w8 = pl.w_from == GEMM_W_PACKED8, two = pl.nt == 2, chained = pl.chain != GEMV_PLAIN;
    if (pl.chain == GEMV_PRODUCER) {
        // producer: one 16-wave block per n-tile, K split over the waves (no slabs, no second kernel)
        GemmP q = p; q.slabs = 0;
        if (w8) hipLaunchKernelGGL((gemm_gemv16_kernel<1, 8, true, true, 16>), dim3(pl.gx), dim3(1024), 0, st, q, KT, ch);
        else hipLaunchKernelGGL((gemm_gemv16_kernel<1, 8, false, true, 16>), dim3(pl.gx), dim3(1024), 0, st, q, KT, ch);
        return;
    }
    const dim3 grid(pl.gx, pl.splits);
#define GEMV16_GO(NT_, W8_, CH_) hipLaunchKernelGGL((gemm_gemv16_kernel<NT_, 8, W8_, CH_>), grid, dim3(256), 0, st, p, KT, ch)
    if (w8) { if (two) { if (chained) GEMV16_GO(2, true, true); else GEMV16_GO(2, true, false); } else { if (chained) GEMV16_GO(1, true, true); else GEMV16_GO(1, true, false); } }
    else    { if (two) { if (chained) GEMV16_GO(2, false, true); else GEMV16_GO(2, false, false); } else { if (chained) GEMV16_GO(1, false, true); else GEMV16_GO(1, false, false); } }
#undef GEMV16_GO
}

template <int MT, int NT, int WK, int KS, int NB, int WN>
static void launch_stream_t(const GemmP& p, const GemmPlan& pl, hipStream_t st) {
    constexpr int KSB = WK * KS;
    constexpr size_t ring = (size_t)NB * MT * KSB * 1024, red = (size_t)(WK - 1) * WN * MT * NT * 1024;
    constexpr size_t smem = ring > red ? ring : red;
    static bool attr_set[64] = {};
    int adev = 0; hipGetDevice(&adev);
    if (smem > 65536 && adev >= 0 && adev < 64 && !attr_set[adev]) {
        hipFuncSetAttribute((const void*)gemm_stream_kernel<MT, NT, WK, KS, NB, WN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        attr_set[adev] = true;
    }
    hipLaunchKernelGGL((gemm_stream_kernel<MT, NT, WK, KS, NB, WN>), dim3(pl.gx, pl.splits), dim3(64 * WN * WK), smem, st, p, p.K >> 5, pl.kt_per_block);
    if (pl.reduce) launch_reduce(splitk_reduce_kernel<bf16_t>, p, pl.splits, st);
}
template <int MT, int NT, int WK, int KS, int NB>
static void launch_stream_wn(const GemmP& p, const GemmPlan& pl, hipStream_t st) {
    switch (pl.wn) {
        case 5: return launch_stream_t<MT, NT, WK, KS, NB, 5>(p, pl, st);
        case 6: return launch_stream_t<MT, NT, WK, KS, NB, 6>(p, pl, st);
        case 7: return launch_stream_t<MT, NT, WK, KS, NB, 7>(p, pl, st);
        case 8: return launch_stream_t<MT, NT, WK, KS, NB, 8>(p, pl, st);
        default: return launch_stream_t<MT, NT, WK, KS, NB, 4>(p, pl, st);
    }
}
static void launch_stream(const GemmP& p, const GemmPlan& pl, hipStream_t st) {          // (MT, NT) -> the steps WK x KS (plan_stream's KSB) and the ring depth NB of the instantiation
    const bool two = pl.nt == 2;
    if (pl.mt == 4) return two ? launch_stream_wn<4, 2, 1, 4, 3>(p, pl, st) : launch_stream_wn<4, 1, 1, 4, 3>(p, pl, st);
    if (pl.mt == 8) return two ? launch_stream_wn<8, 2, 1, 2, 4>(p, pl, st) : launch_stream_wn<8, 1, 1, 4, 3>(p, pl, st);
    return two ? launch_stream_wn<16, 2, 1, 1, 4>(p, pl, st) : launch_stream_wn<16, 1, 1, 2, 4>(p, pl, st);
}

template <int MT>
static void launch_skinny_mt(const GemmP& p, const GemmPlan& pl, hipStream_t st) {
    const int KT = p.K >> 5;
    const dim3 grid(pl.gx, pl.splits);
    if (pl.w_from == GEMM_W_PACKED8) {
        if (pl.nt == 2) hipLaunchKernelGGL((gemm_skinny_kernel<MT, 2, true>), grid, dim3(256), 0, st, p, KT, pl.kt_per_block);
        else hipLaunchKernelGGL((gemm_skinny_kernel<MT, 1, true>), grid, dim3(256), 0, st, p, KT, pl.kt_per_block);
    } else if (pl.nt == 2) hipLaunchKernelGGL((gemm_skinny_kernel<MT, 2>), grid, dim3(256), 0, st, p, KT, pl.kt_per_block);
    else hipLaunchKernelGGL((gemm_skinny_kernel<MT, 1>), grid, dim3(256), 0, st, p, KT, pl.kt_per_block);
    if (pl.reduce) launch_reduce(splitk_reduce_kernel<bf16_t>, p, pl.splits, st);
}

// ------------------------------------------------------------------------------------------------------------------
// MFMA-bound GEMM for M >= 128 rows (ViT tower / projector at M = 32 x 729, multi-frame LLM chunks at M = 49k).
// 128 x BN block tile, 4 waves (2 x 2), BK = 64, two LDS buffers filled by direct-to-LDS DMA (global_load_lds, 16 B per
// lane) one K-tile ahead of the MFMAs, ONE barrier per K-tile.
//   * W (packed, fragment-major): each 16x32 fragment tile is a contiguous 1 KiB piece -> one DMA instruction per piece,
//     the LDS image is already in fragment order (ds_read_b128 at lane*16: conflict-free, no swizzle).
//   * X (row-major): DMA pieces of 8 rows x 128 B (full cache lines); the 16-byte chunk index is XOR-ed with the row on
//     the SOURCE address and again on the fragment read (LDS destination of the DMA is lane-linear by construction),
//     which makes the row-strided fragment reads bank-conflict-free.
//   * rows beyond M are clamped on load and masked at the store; N % BN == 0 and K % 64 == 0 are dispatch conditions.
// ------------------------------------------------------------------------------------------------------------------
template <int BN, int EPI, bool F16 = false, int BM = 128>          // BM = 160 (round 5): 1274 rows x 56 column tiles = 448 blocks, two per CU in ONE round, instead of 560 (three rounds on 48 CUs)
__global__ __launch_bounds__(256) void gemm_big_kernel(GemmP p, int KT) {
    constexpr int BK = 64;
    static_assert(BM % 32 == 0, "two wave rows of whole 16-row tiles");
    constexpr int TM = BM / 32, TN = BN / 32;                // 16x16 tiles per wave (wave tile BM/2 x BN/2)
    constexpr int XE = BM * BK, WE = BN * BK;                // elements per buffer image
    __shared__ __attribute__((aligned(16))) bf16_t lds[2 * (XE + WE)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int wm = (wave >> 1) * (BM / 2), wn = (wave & 1) * (BN / 2);
    // XCD-aware tile order: consecutive block ids round-robin over the 8 XCDs; give each XCD a contiguous run of
    // n-tiles of one m-panel so the X panel stays in that XCD's L2
    const int nbx = gridDim.x, nby = gridDim.y;
    int bid = blockIdx.y * nbx + blockIdx.x;
    const int nblk = nbx * nby;
    {   // bijective for any grid size: XCD x owns a contiguous run of q (+1 for the first r XCDs) tile ids
        const int xcd = bid & 7, q = nblk >> 3, r = nblk & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    // tile order inside an XCD's run: sweep the dimension whose operand is SMALLER fastest, so the larger operand's panel
    // is fetched from HBM once and the smaller one is re-read from L2 / Infinity Cache.  ViT (M >> N): n fastest, the X
    // panel stays put; LLM chunks (N >> M, W = 270 MB > 256 MB Infinity Cache): m fastest, every W panel is streamed once
    // (measured FETCH_SIZE for gate_up at M = 980: 2.1 GB with n-fastest order = 8 x the weights).
    int mt, nt;
    if (p.N > p.M) { nt = bid / nby; mt = bid % nby; } else { mt = bid / nbx; nt = bid % nbx; }
    const int m0 = mt * BM, n0 = nt * BN;
    const bf16_t* X = (const bf16_t*)p.X;
    const bf16_t* Wp = (const bf16_t*)p.W;
    const int nsteps = p.K / BK;

    auto stage = [&](int buf, int step) {
        bf16_t* xs = lds + buf * (XE + WE);
        bf16_t* ws = xs + XE;
        const int k0 = step * BK;
#pragma unroll
        for (int j = 0; j < BM / 32; ++j) {                  // X: pieces of 8 rows x 64 k
            const int pi = wave + 4 * j;
            int row = m0 + pi * 8 + (lane >> 3);
            row = row < p.M ? row : p.M - 1;
            const int chunk = (lane & 7) ^ (lane >> 3);
            const bf16_t* src = X + (long long)row * p.ldx + k0 + chunk * 8;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(xs + pi * 512), 16, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < BN / 32; ++j) {                  // W: (n-tile, k-tile) fragment pieces
            const int wi = wave + 4 * j;
            const bf16_t* src = Wp + (((long long)(n0 / 16 + (wi >> 1)) * KT + (k0 >> 5) + (wi & 1)) * 64 + lane) * 8;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(ws + wi * 512), 16, 0, 0);
        }
    };

    f32x4_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4_t{0, 0, 0, 0};

    // optional split-K over grid.z (medium M with few tiles: fills the CUs; fp32 slabs reduced by splitk_reduce_kernel)
    const int zsteps = (nsteps + gridDim.z - 1) / gridDim.z;
    const int t0 = blockIdx.z * zsteps, t1 = min(nsteps, t0 + zsteps);
    if (t0 < t1) stage(0, t0);
    int cur = 0;
    for (int t = t0; t < t1; ++t) {
        __syncthreads();                                     // (compiler drains the DMA queue here: vmcnt(0))
        if (t + 1 < t1) stage(cur ^ 1, t + 1);
        const bf16_t* xs = lds + cur * (XE + WE);
        const bf16_t* ws = xs + XE;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            bf16x8_t xf[TM], wf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int mt = (wm >> 4) + i;
                const int c = kt * 4 + lq;
                xf[i] = *reinterpret_cast<const bf16x8_t*>(xs + (mt * 2 + (lr >> 3)) * 512 + (lr & 7) * 64 + ((c ^ (lr & 7)) * 8));
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) wf[j] = *reinterpret_cast<const bf16x8_t*>(ws + (((wn >> 4) + j) * 2 + kt) * 512 + lane * 8);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = mfma16<F16>(wf[j], xf[i], acc[i][j]);
        }
        cur ^= 1;
    }

    if (gridDim.z > 1) {
        float* ws = p.ws + (long long)blockIdx.z * p.M * p.N;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m0 + wm + i * 16 + lr;
            if (m < p.M) {
#pragma unroll
                for (int j = 0; j < TN; ++j) *reinterpret_cast<f32x4_t*>(ws + (long long)m * p.N + n0 + wn + j * 16 + lq * 4) = acc[i][j];
            }
        }
        return;
    }
    // operands of the epilogue, fetched in ONE batch: per-column scale / bias quads (once per tile) and every residual quad of the wave's TM x TN tiles
    // (left to the compiler, each quad was loaded right before its use behind a full vmcnt(0): up to 24 serial round trips per tile)
    [[maybe_unused]] f32x4_t scq[TN]; [[maybe_unused]] s16x4_t biq[TN]; [[maybe_unused]] s16x4_t rq[TM][TN];
    const bool has_sc = p.wscale != nullptr, has_bi = p.bias != nullptr;
    if constexpr (EPI != EPI_SWIGLU) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn + j * 16 + lq * 4;
            scq[j] = has_sc ? *reinterpret_cast<const f32x4_t*>(p.wscale + n) : f32x4_t{1, 1, 1, 1};
            biq[j] = has_bi ? *reinterpret_cast<const s16x4_t*>((const bf16_t*)p.bias + n) : s16x4_t{0, 0, 0, 0};
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                rq[i][j] = s16x4_t{0, 0, 0, 0};
                if constexpr (EPI == EPI_RESID) rq[i][j] = *reinterpret_cast<const s16x4_t*>((const bf16_t*)p.R + (long long)min(m0 + wm + i * 16 + lr, p.M - 1) * p.ldr + n0 + wn + j * 16 + lq * 4);
            }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + wm + i * 16 + lr;
        [[maybe_unused]] const int mc = m < p.M ? m : p.M - 1;                      // rows past M compute on a valid row and are not stored
        if constexpr (EPI == EPI_SWIGLU) {
            if constexpr (TN == 4) {                                                // two output tiles: row-contiguous 16-byte stores (pair_to_row8)
                const int nb = n0 + wn, ob = (nb >> 5) * 16;
                const s16x8_t v = pair_to_row8(big_value_swiglu(acc[i][0], acc[i][1], p.wscale, nb + lq * 4), big_value_swiglu(acc[i][2], acc[i][3], p.wscale, nb + 32 + lq * 4));
                if (m < p.M) *reinterpret_cast<s16x8_t*>((bf16_t*)p.Y + (long long)m * p.ldy + ob + (lq & 1) * 16 + (lq >> 1) * 8) = v;
            } else {
#pragma unroll
                for (int j = 0; j < TN; j += 2) big_store_swiglu(p, m, n0 + wn + j * 16 + lq * 4, acc[i][j], acc[i][j + 1]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < TN; j += 2) {
                const int nb = n0 + wn + j * 16;
                const s16x8_t v = pair_to_row8(big_value_pre<EPI, F16>(acc[i][j], has_sc, scq[j], has_bi, biq[j], rq[i][j]), big_value_pre<EPI, F16>(acc[i][j + 1], has_sc, scq[j + 1], has_bi, biq[j + 1], rq[i][j + 1]));
                if (m < p.M) *reinterpret_cast<s16x8_t*>((bf16_t*)p.Y + (long long)m * p.ldy + nb + (lq & 1) * 16 + (lq >> 1) * 8) = v;
            }
        }
    }
}

template <int BN>
static void launch_big(const GemmP& p, const GemmPlan& pl, hipStream_t st) {
    const int KT = p.K >> 5;
    const dim3 grid(pl.gx, pl.gy, pl.splits);
    if (pl.bm == 160) {
        if constexpr (BN == 64) {
            if (p.epi == EPI_RESID) hipLaunchKernelGGL((gemm_big_kernel<64, EPI_RESID, false, 160>), grid, dim3(256), 0, st, p, KT);
            else hipLaunchKernelGGL((gemm_big_kernel<64, EPI_NONE, false, 160>), grid, dim3(256), 0, st, p, KT);
        }
        return;
    }
    if (pl.f16) {          // the fp16 vision tower: plain / GELU(tanh) / residual epilogues
        switch (p.epi) {
            case EPI_GELU_TANH: hipLaunchKernelGGL((gemm_big_kernel<BN, EPI_GELU_TANH, true>), grid, dim3(256), 0, st, p, KT); break;
            case EPI_RESID: hipLaunchKernelGGL((gemm_big_kernel<BN, EPI_RESID, true>), grid, dim3(256), 0, st, p, KT); break;
            default: hipLaunchKernelGGL((gemm_big_kernel<BN, EPI_NONE, true>), grid, dim3(256), 0, st, p, KT); break;
        }
        return;
    }
    switch (p.epi) {
        case EPI_GELU_TANH: hipLaunchKernelGGL((gemm_big_kernel<BN, EPI_GELU_TANH>), grid, dim3(256), 0, st, p, KT); break;
        case EPI_GELU_ERF: hipLaunchKernelGGL((gemm_big_kernel<BN, EPI_GELU_ERF>), grid, dim3(256), 0, st, p, KT); break;
        case EPI_RESID: hipLaunchKernelGGL((gemm_big_kernel<BN, EPI_RESID>), grid, dim3(256), 0, st, p, KT); break;
        case EPI_SWIGLU: hipLaunchKernelGGL((gemm_big_kernel<BN, EPI_SWIGLU>), grid, dim3(256), 0, st, p, KT); break;
        default: hipLaunchKernelGGL((gemm_big_kernel<BN, EPI_NONE>), grid, dim3(256), 0, st, p, KT); break;
    }
    if (pl.reduce) launch_reduce(splitk_reduce_kernel<bf16_t>, p, pl.splits, st);
}


// the ring kernels' masked output lanes need somewhere harmless to store (the store COUNT per wave must not depend on the tile): one 8 KB buffer per device
static void* ring_dump_slot() {
    static void* dump_slot[64] = {};
    int dev = 0; hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) return nullptr;
    if (!dump_slot[dev] && hipMalloc(&dump_slot[dev], 8192) != hipSuccess) return nullptr;
    return dump_slot[dev];
}

template <int WN, bool F16 = false>
static hipError_t launch_ringx_t(const GemmP& p, const GemmPlan& pl, hipStream_t st) {
    constexpr int BN = 64 * WN;
    const dim3 grid(pl.gx, 1, pl.splits);
    const int KT = p.K >> 5;
    const size_t smem = 3 * (256 * 32 + BN * 32) * sizeof(bf16_t);          // three ring slots: 96 KB (WN = 4) / 72 KB (WN = 2)
    static bool attr_set[64] = {};          // per device (hipFuncSetAttribute applies to the current device's code object)
    int adev = 0; hipGetDevice(&adev);
    if (adev >= 0 && adev < 64 && !attr_set[adev]) {
#define RX_ATTR(E) hipFuncSetAttribute((const void*)gemm_ringx_kernel<E, WN, F16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        RX_ATTR(EPI_NONE) RX_ATTR(EPI_GELU_TANH) RX_ATTR(EPI_RESID)
        if constexpr (!F16) { RX_ATTR(EPI_GELU_ERF) RX_ATTR(EPI_SWIGLU) }
#undef RX_ATTR
        attr_set[adev] = true;
    }
    const dim3 block(WN * 128);
    GemmP q = p;
    q.dump = ring_dump_slot();
    if (!q.dump) return hipErrorOutOfMemory;
#define RX_GO(E) hipLaunchKernelGGL((gemm_ringx_kernel<E, WN, F16>), grid, block, smem, st, q, KT)
    switch (p.epi) {          // (the IEEE-half form has the plain / GELU(tanh) / residual epilogues: the plan holds no other for it)
        case EPI_GELU_TANH: RX_GO(EPI_GELU_TANH); break;
        case EPI_GELU_ERF: if constexpr (!F16) RX_GO(EPI_GELU_ERF); break;
        case EPI_RESID: RX_GO(EPI_RESID); break;
        case EPI_SWIGLU: if constexpr (!F16) RX_GO(EPI_SWIGLU); break;
        default: RX_GO(EPI_NONE); break;
    }
#undef RX_GO
    if (pl.reduce) launch_reduce(splitk_reduce_kernel<bf16_t>, p, pl.splits, st);
    return hipSuccess;
}
// the instantiations of gemm_ringx_kernel in the library (plan_ring, gemm_plan.h, says what they are for)
static hipError_t launch_ringx(const GemmP& p, const GemmPlan& pl, hipStream_t st) {
    if (pl.f16) return launch_ringx_t<4, true>(p, pl, st);
    return pl.wn == 4 ? launch_ringx_t<4>(p, pl, st) : launch_ringx_t<2>(p, pl, st);
}

static inline void set_plan(const GemmArgs& a, const GemmPlan& pl) {
    if (a.plan_out) { a.plan_out[0] = pl.kernel; a.plan_out[1] = pl.tiles; a.plan_out[2] = pl.splits; a.plan_out[3] = pl.blocks; }
}

template <typename T>
static hipError_t launch_t(const GemmArgs& a, const GemmPlan& pl, hipStream_t st) {
    GemmP p;
    p.X = a.X; p.W = pl.w_from == GEMM_W_PACKED8 ? a.Wp8 : (pl.w_from == GEMM_W_PACKED ? a.Wp : a.W); p.bias = a.bias; p.R = a.R; p.Y = a.Y; p.ws = a.splitk_ws; p.wscale = a.wscale;
    p.ldx = a.ldx; p.ldw = a.ldw; p.ldr = a.ldr; p.ldy = a.ldy;
    p.M = a.M; p.N = a.N; p.K = a.K; p.epi = a.epi; p.out_f32 = a.out_f32; p.slabs = a.slabs_out ? 1 : 0; p.dump = nullptr; p.flags = 0; p.kper = pl.kper; p.x_pm = a.x_pm; p.y_pm = a.y_pm;
    p.vec = (sizeof(T) == 2 && (a.ldx % 8) == 0 && (a.ldw % 8) == 0 && ((uintptr_t)a.X % 16) == 0 && ((uintptr_t)a.W % 16) == 0) ? 1 : 0;
    if (a.ring_slabs_out) *a.ring_slabs_out = pl.ring_slabs;
    if (pl.kernel == GEMM_PLAN_EMPTY) return hipSuccess;
    if (!pl.valid()) return hipErrorInvalidValue;
    if (a.slabs_out && (pl.kernel == GEMM_K_GEMV16 || pl.kernel == GEMM_K_SKINNY || pl.kernel == GEMM_K_STREAM)) *a.slabs_out = pl.slabs;
    set_plan(a, pl);
    switch (pl.kernel) {
        case GEMM_K_GEMV16: launch_gemv16(p, pl, a.chain, st); break;
        case GEMM_K_STREAM: launch_stream(p, pl, st); break;
        case GEMM_K_RING256: case GEMM_K_RING128X2: if (hipError_t e = launch_ringx(p, pl, st); e != hipSuccess) return e; break;
        case GEMM_K_BIG128: launch_big<128>(p, pl, st); break;
        case GEMM_K_BIG64: launch_big<64>(p, pl, st); break;
        case GEMM_K_SKINNY: if (pl.mt == 1) launch_skinny_mt<1>(p, pl, st); else if (pl.mt == 2) launch_skinny_mt<2>(p, pl, st); else launch_skinny_mt<4>(p, pl, st); break;
        case GEMM_K_TILE128: hipLaunchKernelGGL((gemm_tile_kernel<T, 128, 128>), dim3(pl.gx, pl.gy, 1), dim3(256), 0, st, p); break;
        default:          // GEMM_K_TILE64
            hipLaunchKernelGGL((gemm_tile_kernel<T, 64, 64>), dim3(pl.gx, pl.gy, pl.splits), dim3(256), 0, st, p);
            if (pl.reduce) launch_reduce(splitk_reduce_kernel<T>, p, pl.splits, st);
    }
    return hipGetLastError();
}

// the process's GemmTuning: read from the environment once
const GemmTuning& gemm_tuning() {
    static const GemmTuning tune = [] { GemmTuning t; if (const char* s = getenv("MMDUET_GEMV_KSPLIT_SHORT")) t.gemv_ksplit_short = atoi(s); return t; }();
    return tune;
}
GemmPlan gemm_plan_for(int dtype, const GemmArgs& a) { return gemm_plan(dtype, a, gemm_tuning()); }
bool gemm_can_slab(int dtype, const GemmArgs& a) {
    int dummy = 0; GemmArgs b = a; b.slabs_out = &dummy; b.epi = EPI_NONE;
    const int k = gemm_plan_for(dtype, b).kernel;
    return k == GEMM_K_GEMV16 || k == GEMM_K_SKINNY || k == GEMM_K_STREAM;          // (64 < M <= 256: gemm_stream_kernel leaves slabs too)
}
bool gemm_ring_auto(int dtype, const GemmArgs& a, bool plain_only) {
    const int ring = gemm_plan_for(dtype, a).ring_auto;
    return !a.wscale && (plain_only ? ring == RING_AUTO_PLAIN : ring != RING_AUTO_NONE);
}
hipError_t launch_gemm(int dtype, const GemmArgs& a, hipStream_t st, const GemmPlan* planned) {
    const GemmPlan pl = planned ? *planned : gemm_plan_for(dtype, a);
    return dtype != MMD_F32 ? launch_t<bf16_t>(a, pl, st) : launch_t<float>(a, pl, st);          // MMD_F16: 2-byte storage either way; the kernels' F16 forms read the bits as IEEE half
}
