// sample.hip -- temperature / top-k / top-p sampling of fp32 logit rows on the device (gfx950).  DESIGN.md "Sampling" states the contract; in short, per row:
//   z_i = pen(l_i) / T;  top-k keeps i iff #{z_j > z_i} < k;  top-p keeps i iff the mass of {z_j > z_i} is below p of the top-k survivors' mass;  both are thresholds, so
//   the kept set is {z_i >= tau};  the token is the first kept index, in index order, whose inclusive prefix mass exceeds u * Z_kept, u = r / 2^64, r a Philox4x32-10 word.
// Mass is FIXED POINT: m_i = trunc(exp(z_i - max) * 2^40) in 64-bit integers.  Integer adds commute, so every sum below -- LDS atomics, global atomics, per-slice partials --
// is the same number whatever the grid, the order of arrival or the other rows of the launch, and the inverse CDF is an exact integer search.
//
// Kernels (grid = (slices, rows), 256 threads; a slice is a contiguous column range, the same in every kernel of the chain):
//   sample_scores_kernel   l -> z into the row's fp32 scratch, the repetition penalty as a scatter over the list restricted to the block's slice (computed from the ORIGINAL
//                          logit: duplicates are idempotent), per-slice maximum and NaN flag (one writer each), the row's histograms zeroed
//   sample_select_kernel   one radix level of the threshold search on the order-preserving 32-bit key of z (11 + 11 + 10 bits): the block resolves the level before it
//                          from that level's global (count, mass) histogram, then adds its slice's elements under the resolved prefix to this level's histogram (LDS first).
//                          phases: 0 level 1 | 1, 2 levels 2, 3 of top-k | 3, 4 levels 2, 3 of top-p (level 1 is shared: the same histogram, another target) |
//                          5 resolve the last level, fix tau / kept count / kept mass, write the slice's kept mass.  Rows with both filters off only run phase 5.
//   sample_draw_kernel     one block per row: Philox word (or the explicit one), target = mulhi64(r, Z_kept), the slice from the per-slice masses, the token from a scan
//                          inside the slice; writes token / info, appends to the sampler's slots, advances the row's offset.
// Log-probabilities of the token a row ended with (DESIGN.md "Log-probabilities"; the kernels are at the end of the file): the draw kernel emits z[tok] - zmax - log(Z_kept 2^-40)
// through LogprobOut; three more kernels give the same over the RAW logits plus the top_n largest of them.  A launch records either into one array at consecutive slots or,
// per row, wherever the row's LogprobRow says (the rounds of several streams: every row is another sampler's).
#include "common.h"

constexpr int SMP_L12 = 2048, SMP_L3 = 1024;                                 // bins of radix levels 1, 2 and of level 3
constexpr int SMP_HIST_BINS = 3 * SMP_L12 + 2 * SMP_L3;                      // level 1 | top-k levels 2, 3 | top-p levels 2, 3
constexpr int H_L1 = 0, H_K2 = SMP_L12, H_K3 = 2 * SMP_L12, H_P2 = 2 * SMP_L12 + SMP_L3, H_P3 = 3 * SMP_L12 + SMP_L3;

struct SelState { uint32_t prefix, pad; unsigned long long c_above, m_above, target; };
struct RowState {
    SelState k[2], p[2];          // after radix level 1 / level 2 (one writer, read only behind the next kernel boundary)
    unsigned long long k_mass, total_mass, kept_mass;
    uint32_t k_tau, k_cnt, tau, kept_cnt;
};
// per-row workspace, carved from one allocation: [rows] RowState | [rows][slices] max key, nan, kept mass | [rows][bins] count, mass | [rows][V] z
struct SampleWs {
    RowState* state; uint32_t* part_max; uint32_t* part_nan; unsigned long long* part_mass; uint32_t* hist_c; unsigned long long* hist_m; float* z; long long ldz;
};

size_t sample_topkp_scratch_bytes(int V, int n, bool own_scores) {
    size_t b = (size_t)n * sizeof(RowState) + (size_t)n * SMP_MAX_SLICES * (4 + 4 + 8) + (size_t)n * SMP_HIST_BINS * (4 + 8);
    if (own_scores) b += (size_t)n * (size_t)V * sizeof(float);
    return b + 256;
}
static SampleWs carve(void* scratch, int V, int n, float* scores_out) {
    SampleWs w; char* p = (char*)scratch;
    w.state = (RowState*)p; p += (size_t)n * sizeof(RowState);
    w.part_mass = (unsigned long long*)p; p += (size_t)n * SMP_MAX_SLICES * 8;
    w.hist_m = (unsigned long long*)p; p += (size_t)n * SMP_HIST_BINS * 8;
    w.part_max = (uint32_t*)p; p += (size_t)n * SMP_MAX_SLICES * 4;
    w.part_nan = (uint32_t*)p; p += (size_t)n * SMP_MAX_SLICES * 4;
    w.hist_c = (uint32_t*)p; p += (size_t)n * SMP_HIST_BINS * 4;
    w.z = scores_out ? scores_out : (float*)p; w.ldz = V;
    return w;
}

// order-preserving key: a > b (as floats, no NaN, -0 canonicalised to +0) <=> key(a) > key(b)
__device__ __forceinline__ uint32_t f2key(float f) { const uint32_t b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// fixed-point mass: the maximum is exactly 2^40 (also when it is +inf), -inf is 0
__device__ __forceinline__ unsigned long long mass_fx(float z, float zmax) {
    if (z == zmax) return 1ull << 40;
    return (unsigned long long)(expf(z - zmax) * 1099511627776.f);
}
__device__ __forceinline__ bool row_k_on(const SampleRow& r, int V) { return r.top_k > 0 && r.top_k < V; }
__device__ __forceinline__ bool row_p_on(const SampleRow& r) { return r.top_p < 1.f; }

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the slice of block `blk`: columns [beg, end)
__device__ __forceinline__ void slice_of(int V, int blk, int nblk, int* beg, int* end) {
    const int per = (V + nblk - 1) / nblk;
    *beg = min(V, blk * per); *end = min(V, *beg + per);
}
// row maximum and NaN flag from the per-slice partials (every block folds the <= 64 partials itself).  Flag bit 0: a NaN in the slice.  Bit 1, written for constrained rows
// only: no score of the slice is above -inf -- set in EVERY slice, nothing is left to draw from, and the row is treated like a NaN row (no token, MMD_EDOM).
__device__ __forceinline__ float row_max(const SampleWs& w, int r, int nblk, bool* nan) {
    uint32_t mk = 0, nn = 0, empty = 2u;
    for (int b = 0; b < nblk; ++b) { const uint32_t f = w.part_nan[r * SMP_MAX_SLICES + b]; mk = max(mk, w.part_max[r * SMP_MAX_SLICES + b]); nn |= f & 1u; empty &= f; }
    *nan = (nn | empty) != 0;
    return key2f(mk);
}

// CONS (DESIGN.md "Constraints"): the row's (id, bias) table, sorted by id, is staged in LDS; inside the block's slice the kernel writes, each pass behind a barrier,
//   (l + b) / T for the biased ids  ->  pen(l + b) / T for the ids on the penalty list (b looked up in LDS, 0 when absent: every duplicate writes the same value)  ->
//   -inf for the suppressed ids and, while fewer than min_new tokens have been returned, for the EOS ids.
// Only the block that owns a column writes it.  Without CONS the kernel is the code it was.
template <bool CONS>
__global__ __launch_bounds__(256) void sample_scores_kernel(const float* __restrict__ logits, int V, const SampleRow* __restrict__ rows, SampleWs w, const ConstraintRow* __restrict__ cons) {
    __shared__ uint32_t s_max[4], s_nan[4];
    __shared__ int s_id[CONS ? CONS_MAX_TABLE : 1]; __shared__ float s_b[CONS ? CONS_MAX_TABLE : 1];
    const int r = blockIdx.y; const SampleRow row = rows[r];
    const float* lg = logits + (long long)r * V; float* z = w.z + (long long)r * w.ldz;
    int beg, end; slice_of(V, blockIdx.x, gridDim.x, &beg, &end);
    const float T = row.temperature;
    for (int i = beg + threadIdx.x; i < end; i += 256) { float v = lg[i] / T; if (v == 0.f) v = 0.f; z[i] = v; }
    if (row_k_on(row, V) || row_p_on(row)) {          // this row's histograms: zeroed here, filled by the select kernels behind the kernel boundary
        uint32_t* hc = w.hist_c + (size_t)r * SMP_HIST_BINS; unsigned long long* hm = w.hist_m + (size_t)r * SMP_HIST_BINS;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < SMP_HIST_BINS; i += gridDim.x * 256) { hc[i] = 0; hm[i] = 0; }
    }
    const float pen = row.penalty;
    int nt = 0, n_eos = 0; bool on = false, eos_masked = false;
    if constexpr (CONS) {
        nt = min(cons[r].n, CONS_MAX_TABLE); n_eos = min(cons[r].n_eos, CONS_MAX_EOS); on = nt > 0 || n_eos > 0;
        if (on) {
            const int step = cons[r].step_ptr ? *cons[r].step_ptr : cons[r].step;
            eos_masked = step < cons[r].min_new;
            if ((int)threadIdx.x < nt) { s_id[threadIdx.x] = cons[r].ids[threadIdx.x]; s_b[threadIdx.x] = cons[r].bias[threadIdx.x]; }
            __syncthreads();
            if ((int)threadIdx.x < nt) {
                const int id = s_id[threadIdx.x]; const float b = s_b[threadIdx.x];
                if (id >= beg && id < end && b != -INFINITY) { float v = (lg[id] + b) / T; if (v == 0.f) v = 0.f; z[id] = v; }
            }
        }
    }
    if (pen > 0.f && pen != 1.f) {
        __syncthreads();
        int np = row.n_prev_ptr ? *row.n_prev_ptr : row.n_prev;
        if (np > row.prev_cap) np = row.prev_cap;
        for (int j = threadIdx.x; j < np; j += 256) {
            const long long id = row.prev[j];
            if (id >= beg && id < end) {
                float l = lg[id];
                if constexpr (CONS) {          // the bias of this id, if the table holds it (binary search over the sorted ids)
                    int lo = 0, hi = nt;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_id[mid] < (int)id) lo = mid + 1; else hi = mid; }
                    if (lo < nt && s_id[lo] == (int)id) l = l + s_b[lo];
                }
                float v = (l > 0.f ? l / pen : l * pen) / T; if (v == 0.f) v = 0.f; z[id] = v;          // same value from every duplicate
            }
        }
        __syncthreads();
    }
    if constexpr (CONS) {
        if (on) {
            __syncthreads();
            if ((int)threadIdx.x < nt) { const int id = s_id[threadIdx.x]; if (id >= beg && id < end && s_b[threadIdx.x] == -INFINITY) z[id] = -INFINITY; }
            if (eos_masked && (int)threadIdx.x < n_eos) { const long long id = cons[r].eos[threadIdx.x]; if (id >= beg && id < end) z[id] = -INFINITY; }
            __syncthreads();
        }
    }
    uint32_t mk = 0, nn = 0;
    for (int i = beg + threadIdx.x; i < end; i += 256) { const float v = z[i]; if (v != v) nn = 1; else mk = max(mk, f2key(v)); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mk = max(mk, (uint32_t)__shfl_xor((int)mk, o, 64)); nn |= (uint32_t)__shfl_xor((int)nn, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_max[threadIdx.x >> 6] = mk; s_nan[threadIdx.x >> 6] = nn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) { mk = max(mk, s_max[k]); nn |= s_nan[k]; }
        if constexpr (CONS) { if (on && mk <= 0x007fffffu) nn |= 2u; }          // a constrained row's slice without a score above -inf (0x007fffff = f2key(-inf)): row_max folds the bit
        w.part_max[r * SMP_MAX_SLICES + blockIdx.x] = mk; w.part_nan[r * SMP_MAX_SLICES + blockIdx.x] = nn;
    }
}

// Descending walk over a level's histogram: the first bin whose inclusive cumulative (count if !by_mass, else mass) reaches `target` (1 <= target <= total).
// p_of_total > 0: the target is max(1, ceil(p * Z)), Z = z_override or this histogram's total mass.  All 256 threads call it; all get the result.
struct Found { uint32_t bin; unsigned long long c_above, m_above, c_bin, m_bin, c_tot, m_tot, target; };
__device__ unsigned long long mass_target(float p, unsigned long long Z) {
    unsigned long long t = (unsigned long long)ceil((double)p * (double)Z);
    if (t > Z) t = Z;
    return t < 1 ? 1 : t;
}
__device__ Found hist_find(const uint32_t* __restrict__ hc, const unsigned long long* __restrict__ hm, int nb, bool by_mass, unsigned long long target, float p_of_total,
                           unsigned long long z_override) {
    __shared__ unsigned long long sc[256], sm[256];
    __shared__ Found found;
    const int t = threadIdx.x, q = nb / 256;
    unsigned long long lc = 0, lm = 0;
    for (int i = 0; i < q; ++i) { const int bin = nb - 1 - (t * q + i); lc += hc[bin]; lm += hm[bin]; }
    __syncthreads();          // (a caller may still be reading `found` of an earlier call)
    sc[t] = lc; sm[t] = lm;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        unsigned long long ac = 0, am = 0;
        if (t >= off) { ac = sc[t - off]; am = sm[t - off]; }
        __syncthreads();
        sc[t] += ac; sm[t] += am;
        __syncthreads();
    }
    const unsigned long long c_tot = sc[255], m_tot = sm[255];
    if (p_of_total > 0.f) target = mass_target(p_of_total, z_override ? z_override : m_tot);
    if (t == 0) { found.bin = 0; found.c_above = c_tot; found.m_above = m_tot; found.c_bin = 0; found.m_bin = 0; found.c_tot = c_tot; found.m_tot = m_tot; found.target = target; }
    __syncthreads();
    const unsigned long long ic = sc[t], im = sm[t], ec = ic - lc, em = im - lm;
    const unsigned long long wi = by_mass ? im : ic, we = by_mass ? em : ec;
    if (we < target && target <= wi) {
        unsigned long long rc = ec, rm = em;
        for (int i = 0; i < q; ++i) {
            const int bin = nb - 1 - (t * q + i);
            const unsigned long long bc = hc[bin], bm = hm[bin];
            if ((by_mass ? rm + bm : rc + bc) >= target) { found.bin = bin; found.c_above = rc; found.m_above = rm; found.c_bin = bc; found.m_bin = bm; break; }
            rc += bc; rm += bm;
        }
    }
    __syncthreads();
    return found;
}

__global__ __launch_bounds__(256) void sample_select_kernel(int V, const SampleRow* __restrict__ rows, SampleWs w, int phase) {
    __shared__ uint32_t l_c[SMP_L12]; __shared__ unsigned long long l_m[SMP_L12];
    const int r = blockIdx.y; const SampleRow row = rows[r];
    const bool k_on = row_k_on(row, V), p_on = row_p_on(row);
    if (phase < 5 && !(k_on || p_on)) return;
    if ((phase == 1 || phase == 2) && !k_on) return;
    if ((phase == 3 || phase == 4) && !p_on) return;
    bool nan; const float zmax = row_max(w, r, gridDim.x, &nan);
    if (nan) return;
    RowState* st = w.state + r;
    uint32_t* hc = w.hist_c + (size_t)r * SMP_HIST_BINS; unsigned long long* hm = w.hist_m + (size_t)r * SMP_HIST_BINS;
    const float* z = w.z + (long long)r * w.ldz;
    int beg, end; slice_of(V, blockIdx.x, gridDim.x, &beg, &end);
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;

    // ---- resolve what the kernels before this one left in the histograms ----
    uint32_t prefix = 0; int out_h = H_L1, shift = 21, match_shift = 32, nb = SMP_L12;          // this phase's histogram, digit position, prefix width
    uint32_t tau = 0;
    if (phase == 1) {
        const Found f = hist_find(hc + H_L1, hm + H_L1, SMP_L12, false, (unsigned long long)row.top_k, 0.f, 0);
        prefix = f.bin << 21;
        if (lead) { st->k[0].prefix = prefix; st->k[0].c_above = f.c_above; st->k[0].m_above = f.m_above; st->k[0].target = f.target - f.c_above; st->total_mass = f.m_tot; }
        out_h = H_K2; shift = 10; match_shift = 21;
    } else if (phase == 2 || phase == 4) {
        const SelState s = phase == 2 ? st->k[0] : st->p[0];
        const int in_h = phase == 2 ? H_K2 : H_P2;
        const Found f = hist_find(hc + in_h, hm + in_h, SMP_L12, phase == 4, s.target, 0.f, 0);
        prefix = s.prefix | (f.bin << 10);
        if (lead) {
            SelState* o = phase == 2 ? &st->k[1] : &st->p[1];
            o->prefix = prefix; o->c_above = s.c_above + f.c_above; o->m_above = s.m_above + f.m_above; o->target = s.target - (phase == 4 ? f.m_above : f.c_above);
        }
        out_h = phase == 2 ? H_K3 : H_P3; shift = 0; match_shift = 10; nb = SMP_L3;
    } else if (phase == 3) {
        unsigned long long zk = 0;
        if (k_on) {          // top-k is final: its threshold, survivors and their mass
            const SelState s = st->k[1];
            const Found f = hist_find(hc + H_K3, hm + H_K3, SMP_L3, false, s.target, 0.f, 0);
            zk = s.m_above + f.m_above + f.m_bin;
            if (lead) { st->k_tau = s.prefix | f.bin; st->k_cnt = (uint32_t)(s.c_above + f.c_above + f.c_bin); st->k_mass = zk; }
        }
        const Found f = hist_find(hc + H_L1, hm + H_L1, SMP_L12, true, 0, row.top_p, zk);
        prefix = f.bin << 21;
        if (lead) { st->p[0].prefix = prefix; st->p[0].c_above = f.c_above; st->p[0].m_above = f.m_above; st->p[0].target = f.target - f.m_above; st->total_mass = f.m_tot; }
        out_h = H_P2; shift = 10; match_shift = 21;
    } else if (phase == 5) {
        uint32_t cnt = (uint32_t)V; unsigned long long km = 0;
        if (p_on) {
            const SelState s = st->p[1];
            const Found f = hist_find(hc + H_P3, hm + H_P3, SMP_L3, true, s.target, 0.f, 0);
            tau = s.prefix | f.bin; cnt = (uint32_t)(s.c_above + f.c_above + f.c_bin); km = s.m_above + f.m_above + f.m_bin;
            if (k_on && st->k_tau > tau) { tau = st->k_tau; cnt = st->k_cnt; km = st->k_mass; }
        } else if (k_on) {
            const SelState s = st->k[1];
            const Found f = hist_find(hc + H_K3, hm + H_K3, SMP_L3, false, s.target, 0.f, 0);
            tau = s.prefix | f.bin; cnt = (uint32_t)(s.c_above + f.c_above + f.c_bin); km = s.m_above + f.m_above + f.m_bin;
        }
        if (lead) { st->tau = tau; st->kept_cnt = cnt; st->kept_mass = km; if (!k_on && !p_on) st->total_mass = 0; }
        // the slice's kept mass, for the draw
        unsigned long long m = 0;
        for (int i = beg + threadIdx.x; i < end; i += 256) { const float v = z[i]; if (f2key(v) >= tau) m += mass_fx(v, zmax); }
        __syncthreads();
        l_m[threadIdx.x] = m;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) { if (threadIdx.x < off) l_m[threadIdx.x] += l_m[threadIdx.x + off]; __syncthreads(); }
        if (threadIdx.x == 0) w.part_mass[r * SMP_MAX_SLICES + blockIdx.x] = l_m[0];
        return;
    }

    // ---- this level's histogram over the slice's elements under the prefix ----
    for (int i = threadIdx.x; i < nb; i += 256) { l_c[i] = 0; l_m[i] = 0; }
    __syncthreads();
    for (int i = beg + threadIdx.x; i < end; i += 256) {
        const float v = z[i]; const uint32_t key = f2key(v);
        if (match_shift < 32 && (key >> match_shift) != (prefix >> match_shift)) continue;
        const uint32_t d = (key >> shift) & (uint32_t)(nb - 1);
        atomicAdd(&l_c[d], 1u);
        const unsigned long long m = mass_fx(v, zmax);
        if (m) atomicAdd(&l_m[d], m);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256) {
        const uint32_t cc = l_c[i];
        if (cc) { atomicAdd(&hc[out_h + i], cc); const unsigned long long m = l_m[i]; if (m) atomicAdd(&hm[out_h + i], m); }
    }
}

// Where row r of a launch records (null: nowhere) and how many alternatives.  Both depend on the launch's arguments and the row alone: every thread of a block gets the same.
__device__ __forceinline__ LogprobRec* lp_dest(const LogprobOut& o, int r) {
    if (o.rows) { const LogprobRow d = o.rows[r]; return (d.rec && d.slot >= 0 && d.slot < d.cap) ? d.rec + d.slot : nullptr; }
    if (!o.rec) return nullptr;
    const int ri = (o.dyn ? o.dyn->step : o.idx0) + r;
    return ri < o.cap ? o.rec + ri : nullptr;
}
__device__ __forceinline__ int lp_top_of(const LogprobOut& o, int r) { return min(max(o.rows ? o.rows[r].top_n : o.top_n, 0), LP_MAX_TOP); }

__global__ __launch_bounds__(256) void sample_draw_kernel(int V, int nblk, SampleRow* __restrict__ rows, SampleWs w, const unsigned long long* __restrict__ r_words,
                                                          int64_t* __restrict__ toks_out, float* __restrict__ info_out, LogprobOut lp) {
    __shared__ unsigned long long sm[256];
    __shared__ int s_slice; __shared__ unsigned long long s_base, s_target, s_Z; __shared__ int s_tok;
    const int r = blockIdx.x, t = threadIdx.x; const SampleRow row = rows[r];
    bool nan; const float zmax = row_max(w, r, nblk, &nan);
    const RowState* st = w.state + r;
    const uint32_t tau = st->tau;
    const float* z = w.z + (long long)r * w.ldz;
    if (t == 0) {
        unsigned long long Z = 0;
        for (int b = 0; b < nblk; ++b) Z += w.part_mass[r * SMP_MAX_SLICES + b];
        unsigned long long word;
        if (r_words) word = r_words[r];
        else { uint32_t x[4]; philox4x32_10((uint32_t)row.offset, (uint32_t)(row.offset >> 32), row.lane, 0u, row.seed_lo, row.seed_hi, x); word = ((unsigned long long)x[0] << 32) | x[1]; }
        const unsigned long long target = __umul64hi(word, Z);          // floor(u Z): in [0, Z)
        unsigned long long base = 0; int s = nblk - 1;
        for (int b = 0; b < nblk; ++b) { const unsigned long long m = w.part_mass[r * SMP_MAX_SLICES + b]; if (base + m > target) { s = b; break; } base += m; }
        s_slice = s; s_base = base; s_target = target; s_Z = Z; s_tok = -1;
    }
    __syncthreads();
    if (!nan) {
        int beg, end; slice_of(V, s_slice, nblk, &beg, &end);
        const int run = (end - beg + 255) / 256, i0 = min(end, beg + t * run), i1 = min(end, i0 + run);          // thread t owns the contiguous run [i0, i1)
        unsigned long long m = 0;
        for (int i = i0; i < i1; ++i) { const float v = z[i]; if (f2key(v) >= tau) m += mass_fx(v, zmax); }
        sm[t] = m;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            unsigned long long a = 0;
            if (t >= off) a = sm[t - off];
            __syncthreads();
            sm[t] += a;
            __syncthreads();
        }
        const unsigned long long incl = s_base + sm[t], excl = incl - m, target = s_target;
        if (excl <= target && target < incl) {          // exactly one thread: prefix masses are monotone and the slice holds the target
            unsigned long long run_m = excl;
            for (int i = i0; i < i1; ++i) {
                const float v = z[i];
                if (f2key(v) >= tau) { run_m += mass_fx(v, zmax); if (run_m > target) { s_tok = i; break; } }
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        const long long tok = nan ? -1 : s_tok;
        if (row.tok) *row.tok = tok;
        if (row.append) *row.append = tok;
        if (toks_out) toks_out[r] = tok;
        if (info_out) {
            const bool filt = row_k_on(row, V) || row_p_on(row);
            const unsigned long long tot = filt ? st->total_mass : s_Z;
            info_out[r * 4 + 0] = filt ? key2f(tau) : -INFINITY;
            info_out[r * 4 + 1] = (float)st->kept_cnt;
            info_out[r * 4 + 2] = tot ? (float)((double)s_Z / (double)tot) : 0.f;
            info_out[r * 4 + 3] = nan ? 1.f : 0.f;
        }
        // log-probability of the token under the distribution it was drawn from: the kept set's masses are exactly the ones the draw searched
        LogprobRec* rec = lp_dest(lp, r);
        if (rec) rec->slp = tok < 0 ? NAN : (float)((double)z[tok] - (double)zmax - log((double)s_Z * 0x1p-40));
        if (row.advance) rows[r].offset = row.offset + 1;
    }
}

// the chain's workspace of a launch over n rows, seen from its row r0 on (the records of a block's tail)
static SampleWs carve_from(void* scratch, int V, int n, float* scores_out, int r0) {
    SampleWs w = carve(scratch, V, n, scores_out);
    w.state += r0; w.part_mass += (size_t)r0 * SMP_MAX_SLICES; w.part_max += (size_t)r0 * SMP_MAX_SLICES; w.part_nan += (size_t)r0 * SMP_MAX_SLICES;
    w.hist_m += (size_t)r0 * SMP_HIST_BINS; w.hist_c += (size_t)r0 * SMP_HIST_BINS; w.z += (long long)r0 * w.ldz;
    return w;
}

int sample_topkp_slices(int V) { const int s = cdiv(V, 256); return s < 1 ? 1 : (s > SMP_MAX_SLICES ? SMP_MAX_SLICES : s); }

hipError_t launch_sample_batch_topkp(const float* logits, int V, int n, SampleRow* rows_dev, bool any_k, bool any_p, const unsigned long long* r_words_dev, int64_t* toks_out_dev,
                                     float* info_out_dev, float* scores_out_dev, void* scratch, hipStream_t st, const LogprobOut* lp, const ConstraintRow* cons_dev) {
    if (n <= 0) return hipSuccess;
    if (n > MMD_ROUND_MAX_SAMPLERS || V <= 0 || V > (1 << 18)) return hipErrorInvalidValue;
    const SampleWs w = carve(scratch, V, n, scores_out_dev);
    const int nblk = sample_topkp_slices(V);
    const dim3 grid(nblk, n), blk(256);
    if (cons_dev) hipLaunchKernelGGL(sample_scores_kernel<true>, grid, blk, 0, st, logits, V, (const SampleRow*)rows_dev, w, cons_dev);
    else hipLaunchKernelGGL(sample_scores_kernel<false>, grid, blk, 0, st, logits, V, (const SampleRow*)rows_dev, w, cons_dev);
    if (any_k || any_p) hipLaunchKernelGGL(sample_select_kernel, grid, blk, 0, st, V, (const SampleRow*)rows_dev, w, 0);
    if (any_k) { hipLaunchKernelGGL(sample_select_kernel, grid, blk, 0, st, V, (const SampleRow*)rows_dev, w, 1); hipLaunchKernelGGL(sample_select_kernel, grid, blk, 0, st, V, (const SampleRow*)rows_dev, w, 2); }
    if (any_p) { hipLaunchKernelGGL(sample_select_kernel, grid, blk, 0, st, V, (const SampleRow*)rows_dev, w, 3); hipLaunchKernelGGL(sample_select_kernel, grid, blk, 0, st, V, (const SampleRow*)rows_dev, w, 4); }
    hipLaunchKernelGGL(sample_select_kernel, grid, blk, 0, st, V, (const SampleRow*)rows_dev, w, 5);
    hipLaunchKernelGGL(sample_draw_kernel, dim3(n), blk, 0, st, V, nblk, rows_dev, w, r_words_dev, toks_out_dev, info_out_dev, lp ? *lp : LogprobOut{});
    return hipGetLastError();
}

// ---- log-probabilities ---------------------------------------------------------------------------------------------------------------------------------------------------
// Per row, for the token `t` the row ended with:  lp = l[t] - logsumexp(l) over the RAW logits,  slp = z[t] - logsumexp_{kept} z  (the draw kernel writes it; after an arg-max
// the chain's scores + phase 5 run with T = 1 and nothing filtered, and logprob_final_kernel reads their partials),  and the top_n largest raw logits by (value descending, index
// ascending) with their lp.  The sums are the chain's: the maximum subtracted, mass_fx in 64-bit integers, one writer per (row, slice) partial over the chain's slices -- a row's
// numbers are the same bits whatever the grid and the other rows of the launch.  The last step (two differences and one log per number) runs in double on one thread.
//   logprob_max_top_kernel   grid (slices, rows): the slice's maximum key and NaN flag, then top_n rounds of a block arg-max that each take the best element after the last taken
//   logprob_mass_kernel      grid (slices, rows): the slice's mass against the row maximum
//   logprob_final_kernel     one block per row: Z, the top_n of the slices' candidates (the same rounds over <= 64 * 8 entries in LDS), the record
struct LogprobWs { uint32_t* part_max; uint32_t* part_nan; unsigned long long* part_mass; float* cand_v; int* cand_i; };
constexpr int LP_NONE = 0x7fffffff;          // candidate slot without an element (the slice / row is shorter than top_n)

size_t logprob_scratch_bytes(int n) { return (size_t)n * SMP_MAX_SLICES * (4 + 4 + 8 + LP_MAX_TOP * 8) + 256; }
static LogprobWs carve_lp(void* scratch, int n) {
    LogprobWs w; char* p = (char*)scratch;
    w.part_mass = (unsigned long long*)p; p += (size_t)n * SMP_MAX_SLICES * 8;
    w.part_max = (uint32_t*)p; p += (size_t)n * SMP_MAX_SLICES * 4;
    w.part_nan = (uint32_t*)p; p += (size_t)n * SMP_MAX_SLICES * 4;
    w.cand_v = (float*)p; p += (size_t)n * SMP_MAX_SLICES * LP_MAX_TOP * 4;
    w.cand_i = (int*)p;
    return w;
}

// (value descending, index ascending); NaN is never better than anything
__device__ __forceinline__ bool lp_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }
// the best of one (value, index) per thread; all 256 threads get it
__device__ __forceinline__ void block_best(float& v, int& i, float* s_v, int* s_i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64); const int oi = __shfl_xor(i, o, 64);
        if (lp_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    __syncthreads();          // (the round before may still be reading s_v / s_i)
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = v; s_i[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = s_v[0]; i = s_i[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) if (lp_better(s_v[k], s_i[k], v, i)) { v = s_v[k]; i = s_i[k]; }
}

// `rows` (or null): per-row destinations; a block whose row has none returns at once, the others take their row's own top_n
__global__ __launch_bounds__(256) void logprob_max_top_kernel(const float* __restrict__ logits, int V, LogprobWs w, int top_n, const LogprobRow* __restrict__ rows) {
    __shared__ uint32_t s_max[4], s_nan[4];
    __shared__ float s_v[4]; __shared__ int s_i[4];
    const int r = blockIdx.y;
    if (rows) {          // (block-uniform: the descriptor of blockIdx.y)
        const LogprobRow d = rows[r];
        if (!d.rec || d.slot < 0 || d.slot >= d.cap) return;
        top_n = min(max(d.top_n, 0), LP_MAX_TOP);
    }
    const float* lg = logits + (long long)r * V;
    int beg, end; slice_of(V, blockIdx.x, gridDim.x, &beg, &end);
    uint32_t mk = 0, nn = 0;
    for (int i = beg + threadIdx.x; i < end; i += 256) { const float v = lg[i]; if (v != v) nn = 1; else mk = max(mk, f2key(v)); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mk = max(mk, (uint32_t)__shfl_xor((int)mk, o, 64)); nn |= (uint32_t)__shfl_xor((int)nn, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_max[threadIdx.x >> 6] = mk; s_nan[threadIdx.x >> 6] = nn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) { mk = max(mk, s_max[k]); nn |= s_nan[k]; }
        w.part_max[r * SMP_MAX_SLICES + blockIdx.x] = mk; w.part_nan[r * SMP_MAX_SLICES + blockIdx.x] = nn;
    }
    float last_v = INFINITY; int last_i = -1;          // the element taken last: the next one is the best of those it beats
    for (int j = 0; j < top_n; ++j) {
        float bv = -INFINITY; int bi = LP_NONE;
        for (int i = beg + threadIdx.x; i < end; i += 256) { const float v = lg[i]; if (lp_better(last_v, last_i, v, i) && lp_better(v, i, bv, bi)) { bv = v; bi = i; } }
        block_best(bv, bi, s_v, s_i);
        if (threadIdx.x == 0) { const int c = (r * SMP_MAX_SLICES + blockIdx.x) * LP_MAX_TOP + j; w.cand_v[c] = bv; w.cand_i[c] = bi; }
        last_v = bv; last_i = bi;
    }
}

// row maximum and NaN flag of the raw logits from the per-slice partials
__device__ __forceinline__ float lp_row_max(const LogprobWs& w, int r, int nblk, bool* nan) {
    uint32_t mk = 0, nn = 0;
    for (int b = 0; b < nblk; ++b) { mk = max(mk, w.part_max[r * SMP_MAX_SLICES + b]); nn |= w.part_nan[r * SMP_MAX_SLICES + b]; }
    *nan = nn != 0;
    return key2f(mk);
}

__global__ __launch_bounds__(256) void logprob_mass_kernel(const float* __restrict__ logits, int V, LogprobWs w, const LogprobRow* __restrict__ rows) {
    __shared__ unsigned long long s_m[256];
    const int r = blockIdx.y;
    if (rows) { const LogprobRow d = rows[r]; if (!d.rec || d.slot < 0 || d.slot >= d.cap) return; }          // (before the row's partials are read: nobody wrote them)
    bool nan; const float lmax = lp_row_max(w, r, gridDim.x, &nan);
    if (nan) return;
    const float* lg = logits + (long long)r * V;
    int beg, end; slice_of(V, blockIdx.x, gridDim.x, &beg, &end);
    unsigned long long m = 0;
    for (int i = beg + threadIdx.x; i < end; i += 256) m += mass_fx(lg[i], lmax);
    s_m[threadIdx.x] = m;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) { if (threadIdx.x < off) s_m[threadIdx.x] += s_m[threadIdx.x + off]; __syncthreads(); }
    if (threadIdx.x == 0) w.part_mass[r * SMP_MAX_SLICES + blockIdx.x] = s_m[0];
}

// `greedy`: the row's token came from the arg-max; sw holds the chain's scores pen(l) (T = 1) with their per-slice maxima and (unfiltered) masses
__global__ __launch_bounds__(256) void logprob_final_kernel(const float* __restrict__ logits, int V, int nblk, LogprobWs w, LogprobOut o, int greedy, SampleWs sw) {
    __shared__ float s_cv[SMP_MAX_SLICES * LP_MAX_TOP]; __shared__ int s_ci[SMP_MAX_SLICES * LP_MAX_TOP];
    __shared__ float s_v[4]; __shared__ int s_i[4];
    __shared__ double s_logZ;
    const int r = blockIdx.x, t = threadIdx.x;
    LogprobRec* rec = lp_dest(o, r);
    if (!rec) return;
    const int top_n = lp_top_of(o, r);
    const float* lg = logits + (long long)r * V;
    bool nan; const float lmax = lp_row_max(w, r, nblk, &nan);
    if (t == 0) {
        unsigned long long Z = 0;
        if (!nan) for (int b = 0; b < nblk; ++b) Z += w.part_mass[r * SMP_MAX_SLICES + b];
        s_logZ = log((double)Z * 0x1p-40);
    }
    const int nc = nblk * top_n;
    for (int c = t; c < nc; c += 256) { const int g = (r * SMP_MAX_SLICES + c / top_n) * LP_MAX_TOP + c % top_n; s_cv[c] = w.cand_v[g]; s_ci[c] = w.cand_i[g]; }
    __syncthreads();
    const double logZ = s_logZ;
    float last_v = INFINITY; int last_i = -1;
    for (int j = 0; j < top_n; ++j) {
        float bv = -INFINITY; int bi = LP_NONE;
        for (int c = t; c < nc; c += 256) { const float v = s_cv[c]; const int i = s_ci[c]; if (i != LP_NONE && lp_better(last_v, last_i, v, i) && lp_better(v, i, bv, bi)) { bv = v; bi = i; } }
        block_best(bv, bi, s_v, s_i);
        if (t == 0) {
            rec->top_id[j] = bi == LP_NONE ? -1 : bi;
            rec->top_lp[j] = bi == LP_NONE ? -INFINITY : (nan ? NAN : (float)((double)bv - (double)lmax - logZ));
        }
        last_v = bv; last_i = bi;
    }
    if (t == 0) {
        const long long tok = o.toks[r];
        const bool ok = !nan && tok >= 0 && tok < V;          // (the arg-max of a row of NaNs names no index)
        rec->lp = ok ? (float)((double)lg[tok] - (double)lmax - logZ) : NAN;
        if (greedy) {
            bool znan; const float zmax = row_max(sw, r, nblk, &znan);
            float slp = NAN;
            if (ok && !znan) {
                unsigned long long Z = 0;
                for (int b = 0; b < nblk; ++b) Z += sw.part_mass[r * SMP_MAX_SLICES + b];
                slp = (float)((double)sw.z[(long long)r * sw.ldz + tok] - (double)zmax - log((double)Z * 0x1p-40));
            }
            rec->slp = slp;
        }
    }
}

hipError_t launch_sample_scores_unfiltered(const float* logits, int V, int n, const SampleRow* rows_dev, float* scores_out_dev, void* scratch, hipStream_t st, const ConstraintRow* cons_dev) {
    if (n <= 0) return hipSuccess;
    if (n > MMD_ROUND_MAX_SAMPLERS || V <= 0 || V > (1 << 18)) return hipErrorInvalidValue;
    const SampleWs w = carve(scratch, V, n, scores_out_dev);
    const dim3 grid(sample_topkp_slices(V), n), blk(256);
    if (cons_dev) hipLaunchKernelGGL(sample_scores_kernel<true>, grid, blk, 0, st, logits, V, rows_dev, w, cons_dev);
    else hipLaunchKernelGGL(sample_scores_kernel<false>, grid, blk, 0, st, logits, V, rows_dev, w, cons_dev);
    hipLaunchKernelGGL(sample_select_kernel, grid, blk, 0, st, V, rows_dev, w, 5);
    return hipGetLastError();
}

// The constrained arg-max (DESIGN.md "Constraints"): one block per row over the scores and per-slice maxima the two kernels above left.  The first slice whose maximum is the
// row's holds the first maximal index; the block scans that slice alone.  -1 when the row has a NaN or nothing above -inf.
__global__ __launch_bounds__(256) void argmax_scores_kernel(int V, int nblk, const SampleRow* __restrict__ rows, SampleWs w, int64_t* __restrict__ toks_out) {
    __shared__ int s_i[4];
    const int r = blockIdx.x; const SampleRow row = rows[r];
    bool nan; const float zmax = row_max(w, r, nblk, &nan);
    const uint32_t kmax = f2key(zmax);
    int s = 0;
    while (s < nblk - 1 && w.part_max[r * SMP_MAX_SLICES + s] != kmax) ++s;
    int beg, end; slice_of(V, s, nblk, &beg, &end);
    const float* z = w.z + (long long)r * w.ldz;
    int bi = 0x7fffffff;
    for (int i = beg + threadIdx.x; i < end; i += 256) if (f2key(z[i]) == kmax) { bi = i; break; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bi = min(bi, __shfl_xor(bi, o, 64));
    if ((threadIdx.x & 63) == 0) s_i[threadIdx.x >> 6] = bi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) bi = min(bi, s_i[k]);
        const long long tok = (nan || bi == 0x7fffffff) ? -1 : bi;
        if (row.tok) *row.tok = tok;
        if (row.append) *row.append = tok;
        if (toks_out) toks_out[r] = tok;
    }
}
hipError_t launch_argmax_scores(int V, int n, const SampleRow* rows_dev, float* scores_out_dev, void* scratch, int64_t* toks_out_dev, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (n > MMD_ROUND_MAX_SAMPLERS || V <= 0 || V > (1 << 18)) return hipErrorInvalidValue;
    const SampleWs w = carve(scratch, V, n, scores_out_dev);
    hipLaunchKernelGGL(argmax_scores_kernel, dim3(n), dim3(256), 0, st, V, sample_topkp_slices(V), rows_dev, w, toks_out_dev);
    return hipGetLastError();
}

hipError_t launch_logprob_rows(const float* logits, int V, int n, const LogprobOut& o, bool greedy, float* scores_out_dev, void* sample_scratch, void* lp_scratch, hipStream_t st,
                               int sw_rows, int sw_row0) {
    if (n <= 0) return hipSuccess;
    if (n > MMD_ROUND_MAX_SAMPLERS || V <= 0 || V > (1 << 18) || !o.toks) return hipErrorInvalidValue;
    if (!o.rows && (o.top_n < 0 || o.top_n > LP_MAX_TOP || !o.rec)) return hipErrorInvalidValue;
    if (sw_rows <= 0) { sw_rows = n; sw_row0 = 0; }
    if (sw_row0 < 0 || sw_row0 + n > sw_rows || sw_rows > MMD_ROUND_MAX_SAMPLERS) return hipErrorInvalidValue;
    const LogprobWs w = carve_lp(lp_scratch, n);
    const SampleWs sw = greedy ? carve_from(sample_scratch, V, sw_rows, scores_out_dev, sw_row0) : SampleWs{};
    const int nblk = sample_topkp_slices(V);
    const dim3 grid(nblk, n), blk(256);
    hipLaunchKernelGGL(logprob_max_top_kernel, grid, blk, 0, st, logits, V, w, o.top_n, o.rows);
    hipLaunchKernelGGL(logprob_mass_kernel, grid, blk, 0, st, logits, V, w, o.rows);
    hipLaunchKernelGGL(logprob_final_kernel, dim3(n), blk, 0, st, logits, V, nblk, w, o, greedy ? 1 : 0, sw);
    return hipGetLastError();
}
