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

template <bool PARITY>
__global__ __launch_bounds__(FS_THREADS) void filter_sample_kernel(const FilterArgs a) {
    __shared__ int hist[256];
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
    const uint32_t cut = prefix;                          // key >= cut <=> logit >= the k-th largest, as floats

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

}  // namespace

extern "C" int pk_logits_topk_sample(const float* logits, long long ldl, int M, int V, int k, float temperature,
                                     const float* U, const int* rows, int row_base, unsigned long long seed,
                                     const unsigned long long* seed_dev, int need_lse, const unsigned char* mask, long long* ids,
                                     long long* pred, float* scores, float* cut_out, int* kept_out, void* stream) {
    if (!logits || !pred || M <= 0) return PK_EINVAL;
    if (V < 4 || V > FS_MAX_V || (V & 3) || k < 1 || k > V || ldl < V || (ldl & 3)) return PK_EINVAL;
    if ((scores && !(need_lse & 1)) || (rows && row_base != 0) || row_base < 0) return PK_EINVAL;
    if (!al16(logits) || (U && !al16(U))) return PK_EALIGN;
    FilterArgs a;
    a.logits = logits; a.ldl = ldl; a.V = V; a.k = k;
    a.temp = temperature > 1e-10f ? temperature : 1e-10f;
    a.U = U; a.rows = rows; a.row_base = row_base;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.seed_dev = seed_dev;
    a.need_lse = need_lse & 1; a.no_noise = (need_lse >> 1) & 1;
    a.mask = mask; a.ids = ids; a.pred = pred; a.scores = scores; a.cut_out = cut_out; a.kept_out = kept_out;
    if (U) hipLaunchKernelGGL(filter_sample_kernel<true>, dim3(M), dim3(FS_THREADS), 0, STREAM(stream), a);
    else hipLaunchKernelGGL(filter_sample_kernel<false>, dim3(M), dim3(FS_THREADS), 0, STREAM(stream), a);
    PK_CHECK_LAUNCH();
    return PK_OK;
}
