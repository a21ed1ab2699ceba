// Top-k filtered sampling of the vocabulary head (Phenaki.sample(filter_thres=, top_k=)).
//
//  pk_logits_topk_sample : per row of an f32 logits slab (pk_gemm of the head's operands): cut = the k-th largest logit, counting
//                          multiplicity; a column is kept iff logit >= cut (as floats: -0.0 == +0.0, exact ties at the cut are ALL kept);
//                          pred = argmax over the kept columns of the noisy logit -- the noise expressions, the (logical row, column) noise
//                          index and the first-maximum rule of vocab_sample_kernel (sampler.hip) -- and, on request, 1 - softmax[pred]
//                          over ALL columns; the write-out is pk_vocab_reduce's.
//
// One workgroup of 1024 lanes owns one row and holds it in registers: lane t keeps the f32x4 pieces at columns 4 (t + 1024 j), j < 16
// (V <= 65 536), loaded once with coalesced 16-byte loads.  The k-th largest is found exactly by an MSB-first radix select over an
// order-preserving 32-bit key of the logit: at most 4 passes of 8 bits, each an integer LDS histogram of 256 bins (integer atomics: the
// counts do not depend on the order of arrival) followed by a suffix scan in one wave that names the bin holding the k-th and the count
// above it.  Logits of one row share their sign and exponent bits, so in the first pass nearly every lane would add to the same bin: a
// lane counts a run of equal bins in a register and issues one atomic per run.  The noisy arg-max, the maximum and the sum of
// exponentials are reduced in a fixed order (lanes of a wave by butterfly, then the 16 waves in wave order through LDS); the sum is taken
// against the row's exact maximum, so no partial sum is ever rescaled.  Two calls on the same inputs agree bit for bit.
//
//  pk_logits_nucleus_sample : the same kernel with the adaptive filters in front of the draw (Phenaki.sample(top_p=, min_p=)).
//                          With T = max(temperature, 1e-10f), inv_t = 1.0f / T, lmax the row maximum, arg[v] = (l[v] - lmax) * inv_t in f32,
//                          w[v] = __expf(arg[v]) and the fixed-point mass q[v] = (unsigned long long)(w[v] * 2^40):
//                            top-k  S = {v : l[v] >= cut_k}, cut_k the k-th largest (k == V: all columns);
//                            top-p  cut_p = the largest row value c with sum_{v in S, l[v] >= c} q[v] >= top_p * Z_S, Z_S = sum_{v in S} q[v]
//                                   (product and comparison in double; ties at the cut all kept; top_p == 1: none);
//                            min-p  v passes iff arg[v] >= log_min_p = (float)log((double)min_p) (min_p == 0: none);
//                          kept = S & {l >= cut_p} & {min-p passes} = {v : l[v] >= cut}, cut the smallest kept logit; the draw and the score
//                          are those above.  Order of work: the row maximum (keys compare as integers: exact in any order), the count select
//                          for cut_k, then the mass select: four 8-bit passes over the keys >= cut_k, each an LDS histogram of 256 64-bit
//                          integer masses (a lane sums a run of equal bins in a register and issues one 64-bit integer LDS atomic per run),
//                          scanned from the top by wave 0, which names the bin in which the running mass first reaches the target.  A key's
//                          weight is recomputed from the key in every pass (the 64 keys take half the register budget).  Integer mass: the
//                          cut does not depend on the order of arrival; no float atomics anywhere.
#include "common.hpp"

#include <limits.h>

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

using pk::f32x4;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int FS_THREADS = 1024, FS_NJ = 16, FS_WAVES = FS_THREADS / 64;
constexpr int FS_MAX_V = 4 * FS_THREADS * FS_NJ;

struct FilterArgs {
    const float* logits; long long ldl; int V, k;
    float temp;
    const float* U; const int* rows; int row_base;
    uint32_t seed_lo, seed_hi; const unsigned long long* seed_dev;
    int need_lse, no_noise;
    const unsigned char* mask; long long* ids; long long* pred; float* scores;
    float* cut_out; int* kept_out;
    float top_p, log_min_p;                              // the nucleus kernel only: top_p in (0, 1], 1 = off; log(min_p), -inf = off
};

// order-preserving key of a float: a < b <=> key(a) < key(b) for every pair that is not NaN; -0.0 takes the key of +0.0
__device__ __forceinline__ uint32_t order_key(float x) {
    uint32_t b = __builtin_bit_cast(uint32_t, x);
    if (b == 0x80000000u) b = 0u;
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t key) {
    return __builtin_bit_cast(float, (key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}

template <bool PARITY, bool NUCLEUS>
__global__ __launch_bounds__(FS_THREADS) void filter_sample_kernel(const FilterArgs a) {
    __shared__ int hist[256];
    __shared__ unsigned long long mass[NUCLEUS ? 256 : 1], sel_above;   // the mass histogram of a pass; the mass above the bin it names
    __shared__ uint32_t r_key[NUCLEUS ? 2 * FS_WAVES : 1];
    __shared__ int sel[2];                               // the bin that holds the k-th largest, the count of keys above that bin
    __shared__ float r_best[FS_WAVES], r_blog[FS_WAVES], r_max[FS_WAVES], r_sum[FS_WAVES];
    __shared__ int r_idx[FS_WAVES], r_kept[FS_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = blockIdx.x, V = a.V, nj = (V + 4 * FS_THREADS - 1) / (4 * FS_THREADS);
    const float* __restrict__ row = a.logits + (size_t)m * (size_t)a.ldl;

    // the row, held as keys (the logit comes back from its key exactly, -0.0 as +0.0, which no expression below tells apart: holding both the
    // floats and the keys would take the whole register budget); columns >= V are never read and never counted
    u32x4 x[FS_NJ];
#pragma unroll
    for (int j = 0; j < FS_NJ; ++j) {
        x[j] = u32x4{0u, 0u, 0u, 0u};
        if (j < nj) {
            const int col = 4 * (t + FS_THREADS * j);
            if (col < V) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(row + col);
                x[j] = u32x4{order_key(v[0]), order_key(v[1]), order_key(v[2]), order_key(v[3])};
            }
        }
    }

    // ---- nucleus: the row maximum first.  Keys compare as the floats do, so the largest key is the maximum's, in any order
    float nmax = 0.f;
    if (NUCLEUS) {
        uint32_t km = 0u;                                 // below the key of every float that is not NaN
#pragma unroll
        for (int j = 0; j < FS_NJ; ++j) km = max(max(km, max(x[j][0], x[j][1])), max(x[j][2], x[j][3]));
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) km = max(km, (uint32_t)__shfl_xor((int)km, off, 64));
        if (lane == 0) r_key[wave] = km;
        __syncthreads();
        km = r_key[0];
#pragma unroll
        for (int w = 1; w < FS_WAVES; ++w) km = max(km, r_key[w]);
        nmax = key_value(km);
    }

    // ---- the k-th largest key, MSB first
    uint32_t prefix = order_key(-INFINITY);               // k == V: no select, everything that is not NaN is kept
    if (a.k < V) {
        prefix = 0;
        int kk = a.k;
#pragma unroll 1
        for (int p = 0; p < 4; ++p) {
            const int shift = 24 - 8 * p;
            if (t < 256) hist[t] = 0;
            __syncthreads();
            int run_bin = -1, run_len = 0;
#pragma unroll
            for (int j = 0; j < FS_NJ; ++j) {
                if (j < nj && 4 * (t + FS_THREADS * j) < V) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t key = x[j][r];
                        if (p == 0 || (key >> (shift + 8)) == prefix) {
                            const int b = (int)((key >> shift) & 255u);
                            if (b == run_bin) ++run_len;
                            else {
                                if (run_len) atomicAdd(&hist[run_bin], run_len);
                                run_bin = b; run_len = 1;
                            }
                        }
                    }
                }
            }
            if (run_len) atomicAdd(&hist[run_bin], run_len);
            __syncthreads();
            if (wave == 0) {
                // lane l owns bins 255 - 4 l .. 252 - 4 l; `above` = keys in higher bins, by an inclusive scan over the lanes
                int c[4], s = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) { c[i] = hist[255 - 4 * lane - i]; s += c[i]; }
                int incl = s;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int v = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += v;
                }
                int above = incl - s;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (above < kk && kk <= above + c[i]) { sel[0] = 255 - 4 * lane - i; sel[1] = above; }
                    above += c[i];
                }
            }
            __syncthreads();
            prefix = (prefix << 8) | (uint32_t)sel[0];
            kk -= sel[1];
        }
    }
    if (NUCLEUS) {
        const float inv_t = 1.0f / a.temp;
        if (a.top_p < 1.0f) {
            // ---- the mass select over S = {key >= cut_k}: the largest key c with mass{key >= c} >= top_p * Z_S, MSB first.  `base` is the
            // exact integer mass of S above the keys that share the prefix; the target is formed once, from pass 0's total
            const uint32_t cutk = prefix;
            unsigned long long base = 0ull;
            double target = 0.;                           // wave 0 only
            prefix = 0;
#pragma unroll 1
            for (int p = 0; p < 4; ++p) {
                const int shift = 24 - 8 * p;
                if (t < 256) mass[t] = 0ull;
                __syncthreads();
                int run_bin = -1;
                unsigned long long run_mass = 0ull;
#pragma unroll
                for (int j = 0; j < FS_NJ; ++j) {
                    if (j < nj && 4 * (t + FS_THREADS * j) < V) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const uint32_t key = x[j][r];
                            if (key >= cutk && (p == 0 || (key >> (shift + 8)) == prefix)) {
                                const int b = (int)((key >> shift) & 255u);
                                // the weight does not depend on the pass: opaque, or it is hoisted out of the pass loop, 64 values per lane, and spills
                                uint32_t kw = key;
                                asm volatile("" : "+v"(kw));
                                const unsigned long long q = (unsigned long long)(__expf((key_value(kw) - nmax) * inv_t) * 1099511627776.0f);
                                if (b == run_bin) run_mass += q;
                                else {
                                    if (run_bin >= 0) atomicAdd(&mass[run_bin], run_mass);
                                    run_bin = b; run_mass = q;
                                }
                            }
                        }
                    }
                }
                if (run_bin >= 0) atomicAdd(&mass[run_bin], run_mass);
                __syncthreads();
                if (wave == 0) {
                    // lane l owns bins 255 - 4 l .. 252 - 4 l; `above` = the mass in higher bins, by an inclusive scan over the lanes
                    unsigned long long c[4], s = 0ull;
#pragma unroll
                    for (int i = 0; i < 4; ++i) { c[i] = mass[255 - 4 * lane - i]; s += c[i]; }
                    unsigned long long incl = s;
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        const unsigned long long v = __shfl_up(incl, off, 64);
                        if (lane >= off) incl += v;
                    }
                    if (p == 0) target = (double)a.top_p * (double)__shfl(incl, 63, 64);      // top_p * Z_S
                    unsigned long long above = base + (incl - s);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        // the one bin in which the running mass first reaches the target (a bin of mass 0 never does)
                        if ((double)above < target && target <= (double)(above + c[i])) { sel[0] = 255 - 4 * lane - i; sel_above = above; }
                        above += c[i];
                    }
                }
                __syncthreads();
                prefix = (prefix << 8) | (uint32_t)sel[0];
                base = sel_above;
            }
        }
        if (a.log_min_p > -INFINITY) {
            // ---- min-p: arg is non-decreasing in the logit, so what passes is upward-closed; the smallest key that is kept so far and passes
            // becomes the cut (the maximum has arg = 0 > log(min_p): it always passes)
            uint32_t kmin = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < FS_NJ; ++j) {
                if (j < nj && 4 * (t + FS_THREADS * j) < V) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t key = x[j][r];
                        if (key >= prefix && (key_value(key) - nmax) * inv_t >= a.log_min_p) kmin = min(kmin, key);
                    }
                }
            }
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, off, 64));
            if (lane == 0) r_key[FS_WAVES + wave] = kmin;
            __syncthreads();
            kmin = r_key[FS_WAVES];
#pragma unroll
            for (int w = 1; w < FS_WAVES; ++w) kmin = min(kmin, r_key[FS_WAVES + w]);
            if (kmin != 0xFFFFFFFFu) prefix = kmin;      // only a row holding NaN can keep nothing
        }
    }
    const uint32_t cut = prefix;                          // key >= cut <=> the column is kept: logit >= the k-th largest, as floats

    // ---- noisy arg-max over the kept columns, maximum over all columns
    const long lrow = a.rows ? a.rows[m] : (long)a.row_base + m;
    uint32_t seed_lo = a.seed_lo, seed_hi = a.seed_hi;
    if (!PARITY && a.seed_dev) {
        const unsigned long long sd = (((unsigned long long)a.seed_hi << 32) | a.seed_lo) + *a.seed_dev;
        seed_lo = (uint32_t)sd; seed_hi = (uint32_t)(sd >> 32);
    }
    const float inv_t = 1.0f / a.temp, inv_t_log2e = inv_t * 1.44269504088896340736f;
    float best = -INFINITY, blog = 0.f, lmax = -INFINITY;
    int bidx = INT_MAX, nkept = 0;
#pragma unroll
    for (int j = 0; j < FS_NJ; ++j) {
        const int col = 4 * (t + FS_THREADS * j);
        if (j < nj && col < V) {
            const u32x4 kv = x[j];
            const f32x4 xv = f32x4{key_value(kv[0]), key_value(kv[1]), key_value(kv[2]), key_value(kv[3])};
            const bool k0 = kv[0] >= cut, k1 = kv[1] >= cut, k2 = kv[2] >= cut, k3 = kv[3] >= cut;
            const bool kp[4] = {k0, k1, k2, k3};
            nkept += (int)k0 + (int)k1 + (int)k2 + (int)k3;
            lmax = fmaxf(fmaxf(lmax, fmaxf(xv[0], xv[1])), fmaxf(xv[2], xv[3]));
            if (k0 || k1 || k2 || k3) {
                f32x4 uv = f32x4{0.5f, 0.5f, 0.5f, 0.5f};
                float uf[4] = {0.5f, 0.5f, 0.5f, 0.5f};
                if (!a.no_noise) {
                    if (PARITY) uv = *reinterpret_cast<const f32x4*>(a.U + (size_t)lrow * V + col);
                    else {
                        const uint64_t gq = ((uint64_t)lrow * (uint64_t)V + (uint64_t)col) >> 2;      // V % 4 == 0: group of 4 columns
                        pk::uniform24x4(seed_lo, seed_hi, (uint32_t)gq, (uint32_t)(gq >> 32), uf);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float logit = xv[r];
                    float noisy;
                    if (PARITY) {
                        const float gum = -logf(-logf(uv[r] + 1e-10f) + 1e-10f);
                        noisy = logit / a.temp + gum;
                    } else {
                        noisy = fmaf(logit, inv_t_log2e, -__log2f(-__log2f(uf[r])));                 // u = 0: -inf
                    }
                    if (a.no_noise) noisy = logit;
                    // ascending columns: the first maximum wins; a kept column always beats "none yet", whatever its value
                    if (kp[r] && (noisy > best || bidx == INT_MAX)) { best = noisy; bidx = col + r; blog = logit; }
                }
            }
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float ob = __shfl_xor(best, off, 64), ol = __shfl_xor(blog, off, 64);
        const int oi = __shfl_xor(bidx, off, 64);
        if (oi != INT_MAX && (bidx == INT_MAX || ob > best || (ob == best && oi < bidx))) { best = ob; bidx = oi; blog = ol; }
        lmax = fmaxf(lmax, __shfl_xor(lmax, off, 64));
        nkept += __shfl_xor(nkept, off, 64);
    }
    if (lane == 0) { r_best[wave] = best; r_idx[wave] = bidx; r_blog[wave] = blog; r_max[wave] = lmax; r_kept[wave] = nkept; }
    __syncthreads();
    best = r_best[0]; bidx = r_idx[0]; blog = r_blog[0]; lmax = r_max[0]; nkept = r_kept[0];
#pragma unroll
    for (int w = 1; w < FS_WAVES; ++w) {
        const float ob = r_best[w];
        const int oi = r_idx[w];
        if (oi != INT_MAX && (bidx == INT_MAX || ob > best || (ob == best && oi < bidx))) { best = ob; bidx = oi; blog = r_blog[w]; }
        lmax = fmaxf(lmax, r_max[w]);
        nkept += r_kept[w];
    }
    if (bidx == INT_MAX) bidx = 0;                       // nothing kept: only a row of NaN can get here (k >= 1 keeps the maximum)

    // ---- sum exp over all columns against the row's maximum
    float lsum = 0.f;
    if (a.need_lse) {
#pragma unroll
        for (int j = 0; j < FS_NJ; ++j) {
            if (j < nj && 4 * (t + FS_THREADS * j) < V) {
#pragma unroll
                for (int r = 0; r < 4; ++r) lsum += __expf(key_value(x[j][r]) - lmax);
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) lsum += __shfl_xor(lsum, off, 64);
        if (lane == 0) r_sum[wave] = lsum;
        __syncthreads();
        lsum = r_sum[0];
#pragma unroll
        for (int w = 1; w < FS_WAVES; ++w) lsum += r_sum[w];
    }

    if (t != 0) return;
    if (a.cut_out) a.cut_out[m] = key_value(cut);
    if (a.kept_out) a.kept_out[m] = nkept;
    const long r = lrow;
    a.pred[r] = bidx;
    const bool mk = a.mask ? a.mask[r] != 0 : true;
    if (a.ids && mk) a.ids[r] = bidx;
    if (a.scores && a.need_lse) a.scores[r] = mk ? 1.0f - __expf(blog - lmax) / lsum : -1e4f;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the checks and the argument block that the two entry points share
int filter_args(FilterArgs& a, const float* logits, long long ldl, int M, int V, int k, float temperature, const float* U, const int* rows, int row_base,
                unsigned long long seed, const unsigned long long* seed_dev, int need_lse, const unsigned char* mask, long long* ids, long long* pred,
                float* scores, float* cut_out, int* kept_out) {
    if (!logits || !pred || M <= 0) return PK_EINVAL;
    if (V < 4 || V > FS_MAX_V || (V & 3) || k < 1 || k > V || ldl < V || (ldl & 3)) return PK_EINVAL;
    if ((scores && !(need_lse & 1)) || (rows && row_base != 0) || row_base < 0) return PK_EINVAL;
    if (!al16(logits) || (U && !al16(U))) return PK_EALIGN;
    a.logits = logits; a.ldl = ldl; a.V = V; a.k = k;
    a.temp = temperature > 1e-10f ? temperature : 1e-10f;
    a.U = U; a.rows = rows; a.row_base = row_base;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.seed_dev = seed_dev;
    a.need_lse = need_lse & 1; a.no_noise = (need_lse >> 1) & 1;
    a.mask = mask; a.ids = ids; a.pred = pred; a.scores = scores; a.cut_out = cut_out; a.kept_out = kept_out;
    a.top_p = 1.0f; a.log_min_p = -INFINITY;
    return PK_OK;
}

}  // namespace

extern "C" int pk_logits_topk_sample(const float* logits, long long ldl, int M, int V, int k, float temperature,
                                     const float* U, const int* rows, int row_base, unsigned long long seed,
                                     const unsigned long long* seed_dev, int need_lse, const unsigned char* mask, long long* ids,
                                     long long* pred, float* scores, float* cut_out, int* kept_out, void* stream) {
    FilterArgs a;
    const int rc = filter_args(a, logits, ldl, M, V, k, temperature, U, rows, row_base, seed, seed_dev, need_lse, mask, ids, pred, scores, cut_out,
                               kept_out);
    if (rc != PK_OK) return rc;
    if (U) hipLaunchKernelGGL((filter_sample_kernel<true, false>), dim3(M), dim3(FS_THREADS), 0, STREAM(stream), a);
    else hipLaunchKernelGGL((filter_sample_kernel<false, false>), dim3(M), dim3(FS_THREADS), 0, STREAM(stream), a);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_logits_nucleus_sample(const float* logits, long long ldl, int M, int V, int k, float top_p, float min_p, float temperature,
                                        const float* U, const int* rows, int row_base, unsigned long long seed,
                                        const unsigned long long* seed_dev, int need_lse, const unsigned char* mask, long long* ids,
                                        long long* pred, float* scores, float* cut_out, int* kept_out, void* stream) {
    if (!(top_p > 0.f && top_p <= 1.f) || !(min_p >= 0.f && min_p < 1.f)) return PK_EINVAL;             // NaN fails both
    FilterArgs a;
    const int rc = filter_args(a, logits, ldl, M, V, k, temperature, U, rows, row_base, seed, seed_dev, need_lse, mask, ids, pred, scores, cut_out,
                               kept_out);
    if (rc != PK_OK) return rc;
    a.top_p = top_p;
    a.log_min_p = min_p > 0.f ? (float)log((double)min_p) : -INFINITY;
    if (U) hipLaunchKernelGGL((filter_sample_kernel<true, true>), dim3(M), dim3(FS_THREADS), 0, STREAM(stream), a);
    else hipLaunchKernelGGL((filter_sample_kernel<false, true>), dim3(M), dim3(FS_THREADS), 0, STREAM(stream), a);
    PK_CHECK_LAUNCH();
    return PK_OK;
}
