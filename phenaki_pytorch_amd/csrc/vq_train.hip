// Training step of the cosine-sim VectorQuantize tokenizer (reference construction cvivit.py:321, forward cvivit.py:568-570; the quantizer itself is
// the un-vendored vector-quantize-pytorch module -- its training-mode semantics are RESTATED in DESIGN.md "VectorQuantize training", parity unpinned):
//
//     q = E[ids]                                            gathered before the update, handed on with the straight-through gradient dx = dq
//     commit = w * mean over kept rows of (q - x)^2         x un-normalised, q detached          (pk_vq_gather_commit / pk_vq_commit_bwd)
//     bins[c] = #{kept r : ids[r] = c},  sum[c] = sum of xn[r] over those rows,  xn = l2norm(x)
//     cluster_size = decay cluster_size + (1 - decay) bins;  embed_avg = decay embed_avg + (1 - decay) sum
//     embed[c] = l2norm(embed_avg[c] / smoothed[c]),  smoothed[c] = (cluster_size[c] + eps) / (S + V eps) S,  S = sum_c cluster_size[c]
//
// At the real size the codebook is 65 536 x 512 f32 (134 MB) and a step touches at most M = 4 608 codes, so neither a dense (V, D) `sum` nor an
// (M, V) one-hot exists: the kept rows are counting-sorted by id (integer atomics only -- counts do not depend on arrival order) and every code's
// wave sums ITS rows in ascending row index, whatever order the fill landed them in.  The f32 sums have one fixed order: results are bit-reproducible.
//
//     pk_vq_hist             one thread per row: atomicAdd(counts[id], 1) for kept rows                                   (counts zeroed by the caller)
//     pk_vq_scan             one workgroup: counts -> exclusive offsets (and the fill cursors), EMA of cluster_size, S by a fixed-order tree
//     pk_vq_fill             one thread per kept row: rows[atomicAdd(cursor[id], 1)] = r
//     pk_vq_codebook_update  one wave per code, four codes per workgroup, grid-stride: a pure stream over embed_avg (read + write) and embed (write)
//
// Upkeep of the codebook (DESIGN.md "VectorQuantize upkeep"; the published module's threshold_ema_dead_code and kmeans_init, restated there):
//
//     pick(b, j, n) = ((b mod n) + j P) mod n,  P = 2^31 - 1 (prime: a bijection of [0, n) in j for n < P), 64-bit integers; the j-th choice is the
//     pick-th KEPT row (pk_vq_compact_keep lists them in ascending order; no mask: the identity).  b is a host integer.
//
//     dead-code expiry   pk_vq_scan_expire is pk_vq_scan that also ranks the codes whose post-EMA size is < threshold (jrank[c] = j(c), -1 otherwise);
//                        pk_vq_codebook_update_expire is pk_vq_codebook_update whose wave, for a ranked code, writes embed[c] = xn[r(c)],
//                        embed_avg[c] = reset xn[r(c)], cluster_size[c] = reset instead of the EMA result: no extra launch, no second stream.
//     k-means init       pk_vq_pick_rows seeds means[c] = data[pick(b, c, n)]; an iteration is the lookup, hist / scan (on a scratch cluster_size) /
//                        fill, and pk_vq_kmeans_means: the same ascending-row segment sum, means[c] = l2norm(sum[c]) where bins[c] > 0.
//
// ids are device data: every kernel that indexes with one tests 0 <= id < V first and treats the row as dropped otherwise, so a bad id can never turn
// into an address.  pk_vq_hist(check_ids = 1) additionally copies the ids to the host (one stream synchronisation) and refuses them with PK_EINVAL
// before anything is launched; the training step passes 0 (its ids come out of the library's own argmax kernel).
#include "common.hpp"

#include <limits.h>
#include <vector>

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

using pk::f32x4;

constexpr int VQ_KMAX = 4;               // float4 chunks per lane of a codebook row: D <= 64 * 4 * VQ_KMAX = 1024
constexpr int VQ_SCAN_THREADS = 1024;

__device__ __forceinline__ bool id_ok(long long id, int V) { return (unsigned long long)id < (unsigned long long)V; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void vq_hist_kernel(const long long* __restrict__ ids, const unsigned char* __restrict__ keep, int M, int V,
                                                      int* __restrict__ counts) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= M || (keep && !keep[r])) return;
    const long long id = ids[r];
    if (id_ok(id, V)) atomicAdd(&counts[id], 1);
}

// One workgroup of 16 waves; wave w owns `tiles` consecutive tiles of 64 codes, one code per lane, so every access is a coalesced 256-byte row and the
// loads of a batch of four tiles are in flight together.  Pass 1: EMA of cluster_size, the wave's count total and its share of S.  Pass 2: exclusive
// scan, a shuffle scan per tile on top of a running base.  S is summed lane-serially, then by the butterfly, then over the waves in order: one fixed order.
// EXPIRE: the flags (post-EMA size < threshold, strict) are scanned beside the counts: jrank[c] = the number of flagged codes below c, -1 for the others.
template <bool EXPIRE>
__global__ __launch_bounds__(VQ_SCAN_THREADS) void vq_scan_kernel(const int* __restrict__ counts, int V, float decay, float* __restrict__ cluster_size,
                                                                  int* __restrict__ offsets, int* __restrict__ cursor, float* __restrict__ S,
                                                                  float threshold, int* __restrict__ jrank) {
    constexpr int WAVES = VQ_SCAN_THREADS / 64;
    __shared__ int wtot[WAVES];
    __shared__ int wexp[WAVES];
    __shared__ float wsum[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles = ((V + WAVES - 1) / WAVES + 63) / 64;
    const int base = wave * tiles * 64 + lane;
    const float grow = 1.0f - decay;
    int n = 0, nx = 0;
    float s = 0.f;
    for (int i0 = 0; i0 < tiles; i0 += 4) {
        int k[4];
        float cs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = base + (i0 + u) * 64;
            const bool in = i0 + u < tiles && c < V;
            k[u] = in ? counts[c] : 0;
            cs[u] = in ? cluster_size[c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = base + (i0 + u) * 64;
            if (i0 + u < tiles && c < V) {
                const float v = decay * cs[u] + grow * (float)k[u];
                cluster_size[c] = v;
                n += k[u];
                s += v;
                if (EXPIRE) nx += v < threshold ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    s = wave_sum(s);
    if (EXPIRE) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nx += __shfl_xor(nx, o, 64);
    }
    if (lane == 0) { wtot[wave] = n; wsum[wave] = s; }
    if (EXPIRE && lane == 0) wexp[wave] = nx;
    __syncthreads();
    int run = 0, runx = 0;
    for (int w = 0; w < wave; ++w) run += wtot[w];
    if (EXPIRE)
        for (int w = 0; w < wave; ++w) runx += wexp[w];
    for (int i0 = 0; i0 < tiles; i0 += 4) {
        int k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = base + (i0 + u) * 64;
            k[u] = (i0 + u < tiles && c < V) ? counts[c] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = base + (i0 + u) * 64;
            int inc = k[u];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(inc, o, 64);
                if (lane >= o) inc += y;
            }
            if (i0 + u < tiles && c < V) {
                offsets[c] = run + inc - k[u];
                cursor[c] = run + inc - k[u];
            }
            run += __shfl(inc, 63, 64);
            if (EXPIRE) {
                // (this thread's own pass-1 store: the same thread owns code c in both passes)
                const int dead = (i0 + u < tiles && c < V && cluster_size[c] < threshold) ? 1 : 0;
                int incx = dead;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int y = __shfl_up(incx, o, 64);
                    if (lane >= o) incx += y;
                }
                if (i0 + u < tiles && c < V) jrank[c] = dead ? runx + incx - 1 : -1;
                runx += __shfl(incx, 63, 64);
            }
        }
    }
    if (threadIdx.x == 0) {
        float tot = 0.f;
        for (int w = 0; w < WAVES; ++w) tot += wsum[w];
        S[0] = tot;
    }
}

__global__ __launch_bounds__(256) void vq_fill_kernel(const long long* __restrict__ ids, const unsigned char* __restrict__ keep, int M, int V,
                                                      int* __restrict__ cursor, int* __restrict__ rows) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= M || (keep && !keep[r])) return;
    const long long id = ids[r];
    if (!id_ok(id, V)) return;
    const int pos = atomicAdd(&cursor[id], 1);
    if ((unsigned)pos < (unsigned)M) rows[pos] = r;
}

// The segment walk one wave does for its code: the code's segment of `rows` in ascending row index by repeated minimum extraction.  A segment of
// <= 64 rows (all but a collapsed codebook's) sits one row per lane in a register and each step is six shuffles; a longer one is re-read per step
// (n^2 / 64 loads).  acc = sum of xn[r] over the segment, lane-strided 16-byte chunks.
__device__ __forceinline__ void vq_segment_sum(const float* __restrict__ xn, const int* __restrict__ counts, const int* __restrict__ offsets,
                                               const int* __restrict__ rows, int c, int M, int D, int lane, f32x4 (&acc)[VQ_KMAX]) {
    const int nq = D >> 2;
    int n = counts[c];
    const int off = offsets[c];
    if (n < 0 || off < 0 || off > M - n) n = 0;                      // (never taken after pk_vq_hist / scan / fill on the same ids)
#pragma unroll
    for (int k = 0; k < VQ_KMAX; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int mine = (n <= 64 && lane < n) ? rows[off + lane] : INT_MAX;
    int last = -1;
    for (int j = 0; j < n; ++j) {
        int cand = INT_MAX;
        if (n <= 64) {
            cand = mine > last ? mine : INT_MAX;
        } else {
            for (int i = lane; i < n; i += 64) {
                const int v = rows[off + i];
                if (v > last && v < cand) cand = v;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
        if ((unsigned)cand >= (unsigned)M) break;
        const f32x4* row = reinterpret_cast<const f32x4*>(xn + (size_t)cand * D);
#pragma unroll
        for (int k = 0; k < VQ_KMAX; ++k) {
            const int q = lane + 64 * k;
            if (q < nq) acc[k] += row[q];
        }
        last = cand;
    }
}

constexpr long long VQ_PICK_P = 2147483647LL;                       // 2^31 - 1

// The j-th chosen row, or -1: pick(b, j, n) = ((b mod n) + j P) mod n over the n kept rows (kept NULL: the identity, n = M; else n = n_keep[0] and
// the row is kept[pick]).  n, the position and the row read from `kept` are device data and are range-tested before they are used.
__device__ __forceinline__ int vq_pick_row(long long b, int j, const int* __restrict__ kept, const int* __restrict__ n_keep, int M) {
    const int n = kept ? n_keep[0] : M;
    if (n <= 0 || n > M || j < 0 || b < 0) return -1;
    const long long p = ((b % n) + (long long)j * VQ_PICK_P) % n;
    const int r = kept ? kept[p] : (int)p;
    return (unsigned)r < (unsigned)M ? r : -1;
}

// One wave per code.  EXPIRE: a code ranked by pk_vq_scan_expire (jrank[c] >= 0) takes the chosen row instead of the EMA result.
template <bool EXPIRE>
__global__ __launch_bounds__(256) void vq_codebook_update_kernel(const float* __restrict__ xn, const int* __restrict__ counts, const int* __restrict__ offsets,
                                                                 const int* __restrict__ rows, float* __restrict__ cluster_size,
                                                                 const float* __restrict__ S, const int* __restrict__ jrank, const int* __restrict__ kept,
                                                                 const int* __restrict__ n_keep, int M, int V, int D, float decay, float eps, float reset,
                                                                 long long b, float* __restrict__ embed_avg, float* __restrict__ embed) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nq = D >> 2;
    const float Sv = S[0];
    const float denom = Sv + (float)V * eps;
    const float grow = 1.0f - decay;
    for (int c = blockIdx.x * 4 + wave; c < V; c += gridDim.x * 4) {
        f32x4* avg = reinterpret_cast<f32x4*>(embed_avg + (size_t)c * D);
        f32x4* out = reinterpret_cast<f32x4*>(embed + (size_t)c * D);
        if (EXPIRE) {
            const int j = jrank[c];
            const int r = j >= 0 ? vq_pick_row(b, j, kept, n_keep, M) : -1;
            if (r >= 0) {                                                // (wave-uniform: c, j and r are)
                const f32x4* row = reinterpret_cast<const f32x4*>(xn + (size_t)r * D);
                for (int q = lane; q < nq; q += 64) {
                    const f32x4 v = row[q];
                    out[q] = v;
                    avg[q] = v * reset;
                }
                if (lane == 0) cluster_size[c] = reset;
                continue;
            }
        }
        f32x4 acc[VQ_KMAX];
        vq_segment_sum(xn, counts, offsets, rows, c, M, D, lane, acc);
        const float smoothed = (cluster_size[c] + eps) / denom * Sv;
        f32x4 e[VQ_KMAX];
        float sq = 0.f;
#pragma unroll
        for (int k = 0; k < VQ_KMAX; ++k) {
            const int q = lane + 64 * k;
            if (q < nq) {
                const f32x4 a = decay * avg[q] + grow * acc[k];
                avg[q] = a;
                e[k] = a / smoothed;
                sq += e[k].x * e[k].x + e[k].y * e[k].y + e[k].z * e[k].z + e[k].w * e[k].w;
            }
        }
        const float inv = 1.0f / fmaxf(sqrtf(wave_sum(sq)), 1e-12f);
#pragma unroll
        for (int k = 0; k < VQ_KMAX; ++k) {
            const int q = lane + 64 * k;
            if (q < nq) out[q] = e[k] * inv;
        }
    }
}

// k-means: one wave per code, the same segment sum; means[c] = l2norm(sum[c]) where the code has rows, left alone where it has none.  With
// embed_avg / cluster_size (the last iteration) the initialised state is written beside it: embed_avg[c] = means[c] * bins[c], cluster_size[c] = bins[c].
__global__ __launch_bounds__(256) void vq_kmeans_means_kernel(const float* __restrict__ xn, const int* __restrict__ counts, const int* __restrict__ offsets,
                                                              const int* __restrict__ rows, int M, int V, int D, float* __restrict__ means,
                                                              float* __restrict__ embed_avg, float* __restrict__ cluster_size) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nq = D >> 2;
    for (int c = blockIdx.x * 4 + wave; c < V; c += gridDim.x * 4) {
        f32x4 acc[VQ_KMAX];
        vq_segment_sum(xn, counts, offsets, rows, c, M, D, lane, acc);
        int n = counts[c];
        if (n < 0 || n > M) n = 0;
        f32x4* mean = reinterpret_cast<f32x4*>(means + (size_t)c * D);
        if (n > 0) {
            float sq = 0.f;
#pragma unroll
            for (int k = 0; k < VQ_KMAX; ++k)
                if (lane + 64 * k < nq) sq += acc[k].x * acc[k].x + acc[k].y * acc[k].y + acc[k].z * acc[k].z + acc[k].w * acc[k].w;
            const float inv = 1.0f / fmaxf(sqrtf(wave_sum(sq)), 1e-12f);
#pragma unroll
            for (int k = 0; k < VQ_KMAX; ++k) {
                const int q = lane + 64 * k;
                if (q < nq) {
                    acc[k] = acc[k] * inv;
                    mean[q] = acc[k];
                }
            }
        } else if (embed_avg) {
#pragma unroll
            for (int k = 0; k < VQ_KMAX; ++k) {
                const int q = lane + 64 * k;
                if (q < nq) acc[k] = mean[q];
            }
        }
        if (embed_avg) {
            f32x4* avg = reinterpret_cast<f32x4*>(embed_avg + (size_t)c * D);
#pragma unroll
            for (int k = 0; k < VQ_KMAX; ++k) {
                const int q = lane + 64 * k;
                if (q < nq) avg[q] = acc[k] * (float)n;
            }
            if (lane == 0) cluster_size[c] = (float)n;
        }
    }
}

// out[c] = xn[the c-th chosen row] (the k-means seeds); a choice that fails its range test leaves zeros
__global__ __launch_bounds__(256) void vq_pick_rows_kernel(const float* __restrict__ xn, const int* __restrict__ kept, const int* __restrict__ n_keep, int M,
                                                           int V, int D, long long b, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= V) return;
    const int r = vq_pick_row(b, c, kept, n_keep, M);
    const f32x4* row = reinterpret_cast<const f32x4*>(xn + (size_t)(r >= 0 ? r : 0) * D);
    f32x4* o = reinterpret_cast<f32x4*>(out + (size_t)c * D);
    for (int q = lane; q < (D >> 2); q += 64) o[q] = r >= 0 ? row[q] : f32x4{0.f, 0.f, 0.f, 0.f};
}

// One workgroup: kept[0 .. n) = the indices of the rows `keep` keeps, ascending; n_keep[0] = n.  Thread t owns a run of consecutive rows.
__global__ __launch_bounds__(VQ_SCAN_THREADS) void vq_compact_keep_kernel(const unsigned char* __restrict__ keep, int M, int* __restrict__ kept,
                                                                          int* __restrict__ n_keep) {
    constexpr int WAVES = VQ_SCAN_THREADS / 64;
    __shared__ int wtot[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = (M + VQ_SCAN_THREADS - 1) / VQ_SCAN_THREADS;
    const int lo = min(M, (int)threadIdx.x * per), hi = min(M, lo + per);
    int n = 0;
    for (int r = lo; r < hi; ++r) n += keep[r] ? 1 : 0;
    int inc = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int pos = inc - n;
    for (int w = 0; w < wave; ++w) pos += wtot[w];
    for (int r = lo; r < hi; ++r)
        if (keep[r] && (unsigned)pos < (unsigned)M) kept[pos++] = r;
    if (threadIdx.x == VQ_SCAN_THREADS - 1) n_keep[0] = pos;
}

// one wave per row: y[r] = E[ids[r]], rowsq[r] = sum_d (E[ids[r]][d] - x[r][d])^2 for kept rows, 0 for dropped ones
__global__ __launch_bounds__(256) void vq_gather_commit_kernel(const float* __restrict__ x, const float* __restrict__ E, const long long* __restrict__ ids,
                                                               const unsigned char* __restrict__ keep, int M, int V, int D, float* __restrict__ y,
                                                               float* __restrict__ rowsq) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const int nq = D >> 2;
    const long long id = ids[r];
    const bool ok = id_ok(id, V);
    const f32x4* code = reinterpret_cast<const f32x4*>(E + (size_t)(ok ? id : 0) * D);
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)r * D);
    f32x4* yr = reinterpret_cast<f32x4*>(y + (size_t)r * D);
    float sq = 0.f;
    for (int q = lane; q < nq; q += 64) {
        const f32x4 e = ok ? code[q] : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 d = e - xr[q];
        yr[q] = e;
        sq += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
    }
    sq = wave_sum(sq);
    if (lane == 0) rowsq[r] = (ok && (!keep || keep[r])) ? sq : 0.f;
}

// dx = dy + coef * coef_dev[0] * keep[r] * (x - q), q = the forward's own output rows (the codebook has been updated in place since): 4 elements per thread
__global__ __launch_bounds__(256) void vq_commit_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ q,
                                                            const unsigned char* __restrict__ keep, int M, int D, float coef,
                                                            const float* __restrict__ coef_dev, float* __restrict__ dx) {
    const int nq = D >> 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)M * nq) return;
    f32x4 g = reinterpret_cast<const f32x4*>(dy)[i];
    if (!keep || keep[i / nq]) {
        const float c = coef_dev ? coef * coef_dev[0] : coef;
        g += c * (reinterpret_cast<const f32x4*>(x)[i] - reinterpret_cast<const f32x4*>(q)[i]);
    }
    reinterpret_cast<f32x4*>(dx)[i] = g;
}

inline bool mis16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
inline bool mis4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }
inline bool mis8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; }
inline bool bad_rows(int M, int V) { return M <= 0 || V <= 0; }
inline bool bad_width(int D) { return D <= 0 || (D & 3) || D > 256 * VQ_KMAX; }

}  // namespace

extern "C" int pk_vq_hist(const long long* ids, const unsigned char* keep, int M, int V, int* counts, int check_ids, void* stream) {
    if (!ids || !counts || bad_rows(M, V)) return PK_EINVAL;
    if (mis8(ids) || mis4(counts)) return PK_EALIGN;
    if (check_ids) {
        std::vector<long long> host((size_t)M);
        if (hipMemcpyAsync(host.data(), ids, sizeof(long long) * (size_t)M, hipMemcpyDeviceToHost, STREAM(stream)) != hipSuccess ||
            hipStreamSynchronize(STREAM(stream)) != hipSuccess)
            return PK_ELAUNCH;
        for (int r = 0; r < M; ++r)
            if (host[r] < 0 || host[r] >= V) return PK_EINVAL;
    }
    hipLaunchKernelGGL(vq_hist_kernel, dim3((M + 255) / 256), dim3(256), 0, STREAM(stream), ids, keep, M, V, counts);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_vq_scan(const int* counts, int V, float decay, float* cluster_size, int* offsets, int* cursor, float* S, void* stream) {
    if (!counts || !cluster_size || !offsets || !cursor || !S || V <= 0 || !(decay >= 0.f && decay <= 1.f)) return PK_EINVAL;
    if (mis4(counts) || mis4(cluster_size) || mis4(offsets) || mis4(cursor) || mis4(S)) return PK_EALIGN;
    hipLaunchKernelGGL(vq_scan_kernel<false>, dim3(1), dim3(VQ_SCAN_THREADS), 0, STREAM(stream), counts, V, decay, cluster_size, offsets, cursor, S, 0.f,
                       (int*)nullptr);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_vq_scan_expire(const int* counts, int V, float decay, float threshold, float* cluster_size, int* offsets, int* cursor, float* S,
                                 int* jrank, void* stream) {
    if (!counts || !cluster_size || !offsets || !cursor || !S || !jrank || V <= 0 || !(decay >= 0.f && decay <= 1.f) || !(threshold >= 0.f))
        return PK_EINVAL;
    if (mis4(counts) || mis4(cluster_size) || mis4(offsets) || mis4(cursor) || mis4(S) || mis4(jrank)) return PK_EALIGN;
    hipLaunchKernelGGL(vq_scan_kernel<true>, dim3(1), dim3(VQ_SCAN_THREADS), 0, STREAM(stream), counts, V, decay, cluster_size, offsets, cursor, S, threshold,
                       jrank);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_vq_compact_keep(const unsigned char* keep, int M, int* kept, int* n_keep, void* stream) {
    if (!keep || !kept || !n_keep || M <= 0) return PK_EINVAL;
    if (mis4(kept) || mis4(n_keep)) return PK_EALIGN;
    hipLaunchKernelGGL(vq_compact_keep_kernel, dim3(1), dim3(VQ_SCAN_THREADS), 0, STREAM(stream), keep, M, kept, n_keep);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_vq_fill(const long long* ids, const unsigned char* keep, int M, int V, int* cursor, int* rows, void* stream) {
    if (!ids || !cursor || !rows || bad_rows(M, V)) return PK_EINVAL;
    if (mis8(ids) || mis4(cursor) || mis4(rows)) return PK_EALIGN;
    hipLaunchKernelGGL(vq_fill_kernel, dim3((M + 255) / 256), dim3(256), 0, STREAM(stream), ids, keep, M, V, cursor, rows);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_vq_codebook_update(const float* xn, const int* counts, const int* offsets, const int* rows, const float* cluster_size, const float* S,
                                     int M, int V, int D, float decay, float eps, float* embed_avg, float* embed, void* stream) {
    if (!xn || !counts || !offsets || !rows || !cluster_size || !S || !embed_avg || !embed || bad_rows(M, V) || bad_width(D) ||
        !(decay >= 0.f && decay <= 1.f) || !(eps > 0.f))
        return PK_EINVAL;
    if (mis16(xn) || mis16(embed_avg) || mis16(embed) || mis4(counts) || mis4(offsets) || mis4(rows) || mis4(cluster_size) || mis4(S)) return PK_EALIGN;
    const int blocks = (V + 3) / 4 < 2048 ? (V + 3) / 4 : 2048;                        // 8 workgroups of 4 waves on each of the 256 CUs, grid-stride over the codes
    hipLaunchKernelGGL(vq_codebook_update_kernel<false>, dim3(blocks), dim3(256), 0, STREAM(stream), xn, counts, offsets, rows,
                       const_cast<float*>(cluster_size), S, (const int*)nullptr, (const int*)nullptr, (const int*)nullptr, M, V, D, decay, eps, 0.f, 0LL,
                       embed_avg, embed);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_vq_codebook_update_expire(const float* xn, const int* counts, const int* offsets, const int* rows, float* cluster_size, const float* S,
                                            const int* jrank, const int* kept, const int* n_keep, int M, int V, int D, float decay, float eps,
                                            float reset, long long b, float* embed_avg, float* embed, void* stream) {
    if (!xn || !counts || !offsets || !rows || !cluster_size || !S || !jrank || !embed_avg || !embed || (kept != nullptr) != (n_keep != nullptr) ||
        bad_rows(M, V) || bad_width(D) || !(decay >= 0.f && decay <= 1.f) || !(eps > 0.f) || !(reset >= 0.f) || b < 0)
        return PK_EINVAL;
    if (mis16(xn) || mis16(embed_avg) || mis16(embed) || mis4(counts) || mis4(offsets) || mis4(rows) || mis4(cluster_size) || mis4(S) || mis4(jrank) ||
        (kept && (mis4(kept) || mis4(n_keep))))
        return PK_EALIGN;
    const int blocks = (V + 3) / 4 < 2048 ? (V + 3) / 4 : 2048;
    hipLaunchKernelGGL(vq_codebook_update_kernel<true>, dim3(blocks), dim3(256), 0, STREAM(stream), xn, counts, offsets, rows, cluster_size, S, jrank, kept,
                       n_keep, M, V, D, decay, eps, reset, b, embed_avg, embed);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_vq_pick_rows(const float* xn, const int* kept, const int* n_keep, int M, int V, int D, long long b, float* out, void* stream) {
    if (!xn || !out || (kept != nullptr) != (n_keep != nullptr) || bad_rows(M, V) || bad_width(D) || b < 0) return PK_EINVAL;
    if (mis16(xn) || mis16(out) || (kept && (mis4(kept) || mis4(n_keep)))) return PK_EALIGN;
    hipLaunchKernelGGL(vq_pick_rows_kernel, dim3((V + 3) / 4), dim3(256), 0, STREAM(stream), xn, kept, n_keep, M, V, D, b, out);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_vq_kmeans_means(const float* xn, const int* counts, const int* offsets, const int* rows, int M, int V, int D, float* means,
                                  float* embed_avg, float* cluster_size, void* stream) {
    if (!xn || !counts || !offsets || !rows || !means || (embed_avg != nullptr) != (cluster_size != nullptr) || bad_rows(M, V) || bad_width(D))
        return PK_EINVAL;
    if (mis16(xn) || mis16(means) || mis4(counts) || mis4(offsets) || mis4(rows) || (embed_avg && (mis16(embed_avg) || mis4(cluster_size))))
        return PK_EALIGN;
    const int blocks = (V + 3) / 4 < 2048 ? (V + 3) / 4 : 2048;
    hipLaunchKernelGGL(vq_kmeans_means_kernel, dim3(blocks), dim3(256), 0, STREAM(stream), xn, counts, offsets, rows, M, V, D, means, embed_avg, cluster_size);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_vq_gather_commit(const float* x, const float* E, const long long* ids, const unsigned char* keep, int M, int V, int D, float* y,
                                   float* rowsq, void* stream) {
    if (!x || !E || !ids || !y || !rowsq || bad_rows(M, V) || bad_width(D)) return PK_EINVAL;
    if (mis16(x) || mis16(E) || mis16(y) || mis8(ids) || mis4(rowsq)) return PK_EALIGN;
    hipLaunchKernelGGL(vq_gather_commit_kernel, dim3((M + 3) / 4), dim3(256), 0, STREAM(stream), x, E, ids, keep, M, V, D, y, rowsq);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_vq_commit_bwd(const float* dy, const float* x, const float* q, const unsigned char* keep, int M, int D, float coef,
                                const float* coef_dev, float* dx, void* stream) {
    if (!dy || !x || !q || !dx || M <= 0 || bad_width(D)) return PK_EINVAL;
    if (mis16(dy) || mis16(x) || mis16(q) || mis16(dx) || (coef_dev && mis4(coef_dev))) return PK_EALIGN;
    const long long total = (long long)M * (D >> 2);
    hipLaunchKernelGGL(vq_commit_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, STREAM(stream), dy, x, q, keep, M, D, coef, coef_dev, dx);
    PK_CHECK_LAUNCH();
    return PK_OK;
}
