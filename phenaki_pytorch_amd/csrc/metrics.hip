// Validation metrics of the tokenizer: per-frame squared error (MSE / PSNR), per-frame SSIM and the usage statistics of a code histogram.  The
// reference's CViViTTrainer only dumps image grids every save_results_every steps (cvivit_trainer.py:284-323); these kernels give that validation
// pass numbers at the price of about one extra read of the two videos.  Always f32 in, whatever the compute dtype of the model under validation.
//
// Videos are contiguous f32 (B, C, F, H, W); a plane is one (b, c, f) image of H x W pixels, a frame the C planes of one (b, f).  Every launch of
// the first stage owns one slot of a double `partials` array (plane-major, `parts` slots per plane); the finishing stage gives one wave to a frame
// and adds the frame's C x parts slots in index order.  No floating-point atomics: two calls on the same input give the same bits.  The optional
// clamp acts on the FIRST operand only (the reconstruction: min(max(a, 0), clamp_hi)); no clamped copy is written.
//
//     pk_frame_sqerr   one workgroup per (plane, chunk of 4096 pixels): 4 consecutive pixels per lane and pass, 16-byte loads where both chunk
//                      bases are 16-byte aligned, 4-byte loads of the same pixels otherwise (the same sums either way).  Memory-bound.
//     pk_frame_ssim    SSIM of Wang et al. with the 11 x 11 Gaussian window (sigma 1.5), 'valid' positions, biased moments.  A workgroup walks up to 4
//                      consecutive (plane, 32 x 32 tile of window positions) pairs: the 42 x 42 pixels of both videos go to LDS, an 11-tap horizontal
//                      pass of the five maps a, b, a^2, b^2, ab goes to LDS, the vertical pass runs in registers, 2 x 2 positions per lane, and the next
//                      pair's pixels are fetched meanwhile.  The moments are formed on a - s and b - s, s = the mean of the tile's pixels of a: sigma
//                      and the covariance do not depend on s, and on a nearly flat frame E[a^2] - E[a]^2 on the raw pixels loses what the shifted form
//                      keeps (6e-4 against 4e-7 in f32); s comes back only in the luminance term.  The point formula is kept free of fma contraction
//                      so that two identical frames give exactly 1.  ~130 multiply-adds per position: bound by VALU issue, 0.23 ms at
//                      (8, 3, 17, 256, 256) where the two reads alone are 0.035 ms.
//     pk_code_usage    one workgroup over the (V,) int32 histogram pk_vq_hist wrote: total, used codes, H = ln T - (sum c ln c) / T, exp(H), max c / T
//                      in double, lane-strided sums and a fixed tree.
#include "common.hpp"

#include <limits.h>

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

using pk::f32x2;
using pk::f32x4;

constexpr int SQ_CHUNK = 4096;                                     // pixels per workgroup of the squared-error pass: 4 passes of 256 lanes x 4
constexpr int SS_WIN = 11, SS_TILE = 32, SS_HALO = SS_TILE + SS_WIN - 1;
constexpr int SS_LDA = SS_HALO + 1, SS_LDH = SS_TILE + 1;          // odd row strides: two rows of a 32-lane group fall on different banks
constexpr int USAGE_THREADS = 1024;
constexpr long MAX_BLOCKS = (1L << 24) - 1;                        // 256-lane workgroups of one launch

// exp(-(k - 5)^2 / (2 * 1.5^2)) normalised to sum 1 in double, rounded to f32
#define SS_WEIGHTS {1.028380084e-03f, 7.598758135e-03f, 3.600077213e-02f, 1.093606895e-01f, 2.130055377e-01f, 2.660117249e-01f, \
                    2.130055377e-01f, 1.093606895e-01f, 3.600077213e-02f, 7.598758135e-03f, 1.028380084e-03f}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool CLAMP>
__device__ __forceinline__ float clamp_first(float v, float hi) { return CLAMP ? fminf(fmaxf(v, 0.f), hi) : v; }

__device__ __forceinline__ bool aligned16(const void* p, const void* q) {
    return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & 15) == 0;
}

// the four wave sums of a 256-lane workgroup in a fixed order -> partials[blockIdx.x]
__device__ __forceinline__ void block_partial(double acc, double* red, double* __restrict__ partials) {
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- squared error: workgroup = (plane, chunk).  Lane t owns pixels (u * 256 + t) * 4 .. + 3 of the chunk, u = 0..3, whichever load form is taken
template <bool CLAMP>
__global__ __launch_bounds__(256) void sqerr_chunk_kernel(const float* __restrict__ a, const float* __restrict__ b, long HW, int nchunks, float clamp_hi,
                                                          double* __restrict__ partials) {
    __shared__ double red[4];
    const long plane = blockIdx.x / (unsigned)nchunks;
    const long off = (long)(blockIdx.x - plane * nchunks) * SQ_CHUNK;
    const int n = (int)(HW - off < SQ_CHUNK ? HW - off : SQ_CHUNK);
    const float* __restrict__ pa = a + plane * HW + off;
    const float* __restrict__ pb = b + plane * HW + off;
    const bool vec = aligned16(pa, pb);
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < SQ_CHUNK / 1024; ++u) {
        const int i = (u * 256 + (int)threadIdx.x) * 4;
        float va[4] = {0.f, 0.f, 0.f, 0.f}, vb[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && i + 3 < n) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(pa + i), y = *reinterpret_cast<const f32x4*>(pb + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) { va[e] = clamp_first<CLAMP>(x[e], clamp_hi); vb[e] = y[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < n) { va[e] = clamp_first<CLAMP>(pa[i + e], clamp_hi); vb[e] = pb[i + e]; }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = va[e] - vb[e];
            acc = fmaf(d, d, acc);
        }
    }
    block_partial((double)acc, red, partials);
}

// ---- SSIM at one window position from the five filtered maps of the shifted pixels: luminance x contrast-structure as ONE quotient.  No
// contraction: with a == b every pair of operands below is bit-identical, numerator and denominator are the same product and the quotient is exactly 1
__device__ __forceinline__ float ssim_point(float m1, float m2, float e11, float e22, float e12, float s, float C1, float C2) {
#pragma clang fp contract(off)
    const float v1 = e11 - m1 * m1, v2 = e22 - m2 * m2, cov = e12 - m1 * m2;
    const float mu1 = m1 + s, mu2 = m2 + s;
    const float num = (2.f * (mu1 * mu2) + C1) * (2.f * cov + C2);
    const float den = ((mu1 * mu1 + mu2 * mu2) + C1) * ((v1 + v2) + C2);
    return num / den;
}

// a barrier that orders LDS traffic only: __syncthreads() would also wait for the next tile's pixel loads, which are meant to stay in flight
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

constexpr int SS_GROUPS = (SS_HALO + 3) / 4;                       // 4-pixel groups of a halo row (the last keeps 2 pixels)
constexpr int SS_FETCH = (SS_HALO * SS_GROUPS + 255) / 256;        // groups per lane: 2
struct SsimHalo { float a[SS_FETCH][4], b[SS_FETCH][4]; };

// the lane's groups of the tile's 42 x 42 pixels of both videos -> registers (first operand clamped; 0 outside the image).  A 16-byte load where
// the group lies inside the row and both addresses allow it, 4-byte loads of the same pixels otherwise
template <bool CLAMP>
__device__ __forceinline__ void ssim_fetch(const float* __restrict__ a, const float* __restrict__ b, int H, int W, unsigned tilesX, unsigned ntiles,
                                           unsigned blk, float clamp_hi, SsimHalo& h) {
    const unsigned plane = blk / ntiles, tile = blk - plane * ntiles, trow = tile / tilesX;
    const int ty0 = (int)trow * SS_TILE, tx0 = (int)(tile - trow * tilesX) * SS_TILE;
    const float* __restrict__ pa = a + plane * ((long)H * W);
    const float* __restrict__ pb = b + plane * ((long)H * W);
#pragma unroll
    for (int it = 0; it < SS_FETCH; ++it) {
        const int i = it * 256 + (int)threadIdx.x;
        const int r = i / SS_GROUPS, c0 = (i - r * SS_GROUPS) * 4;
        const int y = ty0 + r, x = tx0 + c0;
#pragma unroll
        for (int e = 0; e < 4; ++e) h.a[it][e] = h.b[it][e] = 0.f;
        if (i < SS_HALO * SS_GROUPS && y < H) {
            const float* __restrict__ ra = pa + (long)y * W + x;
            const float* __restrict__ rb = pb + (long)y * W + x;
            if (x + 3 < W && aligned16(ra, rb)) {
                const f32x4 p = *reinterpret_cast<const f32x4*>(ra), q = *reinterpret_cast<const f32x4*>(rb);
#pragma unroll
                for (int e = 0; e < 4; ++e) { h.a[it][e] = clamp_first<CLAMP>(p[e], clamp_hi); h.b[it][e] = q[e]; }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (x + e < W) { h.a[it][e] = clamp_first<CLAMP>(ra[e], clamp_hi); h.b[it][e] = rb[e]; }
            }
        }
    }
}

// A workgroup walks `tpw` consecutive (plane, tile) pairs of the launch; pair blk owns partials[blk].  Tile: window positions [ty0, ty0 + 32) x
// [tx0, tx0 + 32), pixels [ty0, ty0 + 42) x [tx0, tx0 + 42), of which nrows x ncols lie in the image (ty0 <= H - 11, tx0 <= W - 11: at least 11 x 11).
// The pixels of the next pair are fetched into registers while the two passes of the current one run.  The raw pixels lie in LDS and the shift is
// taken where they are read: a pixel outside the image reads as -s, which reaches only positions outside the valid range, and those are not summed.
template <bool CLAMP>
__global__ __launch_bounds__(256) void ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W, unsigned tilesX,
                                                        unsigned ntiles, unsigned total, unsigned tpw, float clamp_hi, float C1, float C2,
                                                        double* __restrict__ partials) {
    __shared__ float sa[SS_HALO * SS_LDA];
    __shared__ float sb[SS_HALO * SS_LDA];
    __shared__ float sh[5][SS_HALO * SS_LDH];
    __shared__ double red[4];
    __shared__ float reds[4];
    static_assert(SS_FETCH * 256 >= SS_HALO * SS_GROUPS, "every group of the halo has a lane");
    const float g[SS_WIN] = SS_WEIGHTS;
    const int tid = threadIdx.x;
    unsigned blk = blockIdx.x * tpw;                                 // total <= MAX_BLOCKS: 32-bit index arithmetic throughout
    const unsigned end = blk + tpw < total ? blk + tpw : total;
    SsimHalo h;
    ssim_fetch<CLAMP>(a, b, H, W, tilesX, ntiles, blk, clamp_hi, h);
    for (; blk < end; ++blk) {
        const unsigned tile = blk % ntiles, trow = tile / tilesX;
        const int ty0 = (int)trow * SS_TILE, tx0 = (int)(tile - trow * tilesX) * SS_TILE;

        // registers -> LDS, each lane keeping the sum of the pixels of `a` it stores (0 outside the image)
        float part = 0.f;
#pragma unroll
        for (int it = 0; it < SS_FETCH; ++it) {
            const int i = it * 256 + tid;
            const int r = i / SS_GROUPS, c0 = (i - r * SS_GROUPS) * 4;
            if (i < SS_HALO * SS_GROUPS) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c0 + e < SS_HALO) {
                        sa[r * SS_LDA + c0 + e] = h.a[it][e];
                        sb[r * SS_LDA + c0 + e] = h.b[it][e];
                        part += h.a[it][e];
                    }
            }
        }
        // s = the mean of the tile's pixels of `a`, in a fixed order: lane, butterfly, the four waves
        part = pk::wave_sum(part);
        if ((tid & 63) == 0) reds[tid >> 6] = part;
        lds_barrier();
        const int nrows = H - ty0 < SS_HALO ? H - ty0 : SS_HALO, ncols = W - tx0 < SS_HALO ? W - tx0 : SS_HALO;
        const float s = ((reds[0] + reds[1]) + (reds[2] + reds[3])) / (float)(nrows * ncols);

        if (blk + 1 < end) ssim_fetch<CLAMP>(a, b, H, W, tilesX, ntiles, blk + 1, clamp_hi, h);       // in flight until the next round's stores

        // horizontal pass: 42 rows x 16 pairs of columns; 12 pixels of each video feed two positions of the five maps
        for (int i = tid; i < SS_HALO * (SS_TILE / 2); i += 256) {
            const int r = i >> 4, c = (i & 15) * 2;
            float o[5][2] = {};
#pragma unroll
            for (int k = 0; k < SS_WIN + 1; ++k) {
                const float x = sa[r * SS_LDA + c + k] - s, y = sb[r * SS_LDA + c + k] - s;
                const float q[5] = {x, y, x * x, y * y, x * y};
#pragma unroll
                for (int m = 0; m < 5; ++m) {
                    if (k < SS_WIN) o[m][0] = fmaf(g[k], q[m], o[m][0]);
                    if (k > 0) o[m][1] = fmaf(g[k - 1], q[m], o[m][1]);
                }
            }
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                sh[m][r * SS_LDH + c] = o[m][0];
                sh[m][r * SS_LDH + c + 1] = o[m][1];
            }
        }
        lds_barrier();

        // vertical pass: lane = (pair of columns, pair of rows); 12 rows of a map feed its 2 x 2 positions, the two columns in one packed multiply-add
        const int cx = (tid & 15) * 2, r0 = (tid >> 4) * 2;
        f32x2 f[5][2] = {};
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            f32x2 v[SS_WIN + 1];
#pragma unroll
            for (int j = 0; j < SS_WIN + 1; ++j) v[j] = f32x2{sh[m][(r0 + j) * SS_LDH + cx], sh[m][(r0 + j) * SS_LDH + cx + 1]};
#pragma unroll
            for (int o = 0; o < 2; ++o)
#pragma unroll
                for (int k = 0; k < SS_WIN; ++k) f[m][o] = __builtin_elementwise_fma(f32x2{g[k], g[k]}, v[o + k], f[m][o]);
        }
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const bool valid = ty0 + r0 + o < H - (SS_WIN - 1) && tx0 + cx + e < W - (SS_WIN - 1);
                const float v = ssim_point(f[0][o][e], f[1][o][e], f[2][o][e], f[3][o][e], f[4][o][e], s, C1, C2);
                acc += valid ? v : 0.f;
            }
        // the four wave sums in a fixed order.  The barrier also closes the round: every lane is done with sa / sb / sh / reds before the next stores
        const double wsum = wave_sum_f64((double)acc);
        if ((tid & 63) == 0) red[tid >> 6] = wsum;
        lds_barrier();
        if (tid == 0) partials[blk] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// ---- one wave per frame (b, f): its C x parts slots in index order (lane-strided, then the butterfly), over `count`
__global__ __launch_bounds__(64) void frame_finish_kernel(const double* __restrict__ partials, int C, int F, int parts, double count, double r2,
                                                          float* __restrict__ mean, float* __restrict__ psnr) {
    const int frame = blockIdx.x, bi = frame / F, fi = frame - bi * F;
    const long n = (long)C * parts;
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 64) {
        const long c = i / parts, t = i - c * parts;
        acc += partials[(((long)bi * C + c) * F + fi) * parts + t];
    }
    acc = wave_sum_f64(acc);
    if (threadIdx.x == 0) {
        const double m = acc / count;
        mean[frame] = (float)m;
        if (psnr) psnr[frame] = (float)(10.0 * log10(r2 / fmax(m, 1e-10 * r2)));        // identical frames: 100 dB, and means stay finite
    }
}

// ---- usage of a code histogram.  Entries <= 0 count as unused
__global__ __launch_bounds__(USAGE_THREADS) void code_usage_kernel(const int* __restrict__ counts, int V, double* __restrict__ out) {
    __shared__ double s_clogc[USAGE_THREADS];
    __shared__ long long s_total[USAGE_THREADS];
    __shared__ int s_used[USAGE_THREADS];
    __shared__ int s_max[USAGE_THREADS];
    const int tid = threadIdx.x;
    double clogc = 0.0;
    long long total = 0;
    int used = 0, mx = 0;
    for (int i = tid; i < V; i += USAGE_THREADS) {
        const int c = counts[i];
        if (c > 0) {
            total += c;
            ++used;
            mx = c > mx ? c : mx;
            clogc += (double)c * log((double)c);
        }
    }
    s_clogc[tid] = clogc; s_total[tid] = total; s_used[tid] = used; s_max[tid] = mx;
    __syncthreads();
    for (int o = USAGE_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            s_clogc[tid] += s_clogc[tid + o];
            s_total[tid] += s_total[tid + o];
            s_used[tid] += s_used[tid + o];
            s_max[tid] = s_max[tid + o] > s_max[tid] ? s_max[tid + o] : s_max[tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double T = (double)s_total[0];
        double H = 0.0;
        if (s_total[0] > 0) H = fmax(log(T) - s_clogc[0] / T, 0.0);
        out[0] = T;
        out[1] = (double)s_used[0];
        out[2] = H;
        out[3] = exp(H);
        out[4] = s_total[0] > 0 ? (double)s_max[0] / T : 0.0;
    }
}

inline bool mis4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }
inline bool mis8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; }
inline bool bad_video(const float* a, const float* b, int B, int C, int F, int H, int W) { return !a || !b || B <= 0 || C <= 0 || F <= 0 || H <= 0 || W <= 0; }

}  // namespace

// slots of the partials array per plane (host only; < 0: PK_EINVAL)
extern "C" int pk_frame_sqerr_parts(int H, int W) {
    if (H <= 0 || W <= 0) return PK_EINVAL;
    const long parts = ((long)H * W + SQ_CHUNK - 1) / SQ_CHUNK;
    return parts > INT_MAX ? PK_EINVAL : (int)parts;
}

extern "C" int pk_frame_ssim_parts(int H, int W) {
    if (H < SS_WIN || W < SS_WIN) return PK_EINVAL;
    const long parts = (long)((H - SS_WIN + SS_TILE) / SS_TILE) * ((W - SS_WIN + SS_TILE) / SS_TILE);
    return parts > INT_MAX ? PK_EINVAL : (int)parts;
}

extern "C" int pk_frame_sqerr(const float* a, const float* b, int B, int C, int F, int H, int W, float clamp_hi, float data_range, double* partials,
                              long long nparts, float* mse, float* psnr, void* stream) {
    if (bad_video(a, b, B, C, F, H, W) || !partials || !mse || (psnr && !(data_range > 0.f))) return PK_EINVAL;
    const int parts = pk_frame_sqerr_parts(H, W);
    const long planes = (long)B * C * F;
    if (parts < 0 || planes * parts > MAX_BLOCKS || (long)B * F > INT_MAX || nparts != planes * parts) return PK_EINVAL;
    if (mis4(a) || mis4(b) || mis8(partials) || mis4(mse) || (psnr && mis4(psnr))) return PK_EALIGN;
    const long HW = (long)H * W;
    if (clamp_hi > 0.f)
        hipLaunchKernelGGL(sqerr_chunk_kernel<true>, dim3((unsigned)(planes * parts)), dim3(256), 0, STREAM(stream), a, b, HW, parts, clamp_hi, partials);
    else
        hipLaunchKernelGGL(sqerr_chunk_kernel<false>, dim3((unsigned)(planes * parts)), dim3(256), 0, STREAM(stream), a, b, HW, parts, 0.f, partials);
    hipLaunchKernelGGL(frame_finish_kernel, dim3((unsigned)(B * F)), dim3(64), 0, STREAM(stream), (const double*)partials, C, F, parts,
                       (double)C * (double)HW, (double)data_range * (double)data_range, mse, psnr);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_frame_ssim(const float* a, const float* b, int B, int C, int F, int H, int W, float clamp_hi, float data_range, double* partials,
                             long long nparts, float* ssim, void* stream) {
    if (bad_video(a, b, B, C, F, H, W) || H < SS_WIN || W < SS_WIN || !partials || !ssim || !(data_range > 0.f)) return PK_EINVAL;
    const int parts = pk_frame_ssim_parts(H, W);
    const long planes = (long)B * C * F;
    if (parts < 0 || planes * parts > MAX_BLOCKS || (long)B * F > INT_MAX || nparts != planes * parts) return PK_EINVAL;
    if (mis4(a) || mis4(b) || mis8(partials) || mis4(ssim)) return PK_EALIGN;
    const int tilesX = (W - SS_WIN + SS_TILE) / SS_TILE;
    const unsigned total = (unsigned)(planes * parts);
    const unsigned tpw = total >= 16384 ? 4 : total >= 4096 ? 2 : 1;  // pairs per workgroup: the next pair's loads overlap the current pair's passes
    const unsigned grid = (total + tpw - 1) / tpw;
    const float C1 = (0.01f * data_range) * (0.01f * data_range), C2 = (0.03f * data_range) * (0.03f * data_range);
    if (clamp_hi > 0.f)
        hipLaunchKernelGGL(ssim_tile_kernel<true>, dim3(grid), dim3(256), 0, STREAM(stream), a, b, H, W, (unsigned)tilesX, (unsigned)parts, total, tpw, clamp_hi, C1, C2,
                           partials);
    else
        hipLaunchKernelGGL(ssim_tile_kernel<false>, dim3(grid), dim3(256), 0, STREAM(stream), a, b, H, W, (unsigned)tilesX, (unsigned)parts, total, tpw, 0.f, C1, C2,
                           partials);
    hipLaunchKernelGGL(frame_finish_kernel, dim3((unsigned)(B * F)), dim3(64), 0, STREAM(stream), (const double*)partials, C, F, parts,
                       (double)C * (double)(H - SS_WIN + 1) * (double)(W - SS_WIN + 1), 1.0, ssim, (float*)nullptr);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_code_usage(const int* counts, int V, double* out, void* stream) {
    if (!counts || !out || V <= 0) return PK_EINVAL;
    if (mis4(counts) || mis8(out)) return PK_EALIGN;
    hipLaunchKernelGGL(code_usage_kernel, dim3(1), dim3(USAGE_THREADS), 0, STREAM(stream), counts, V, out);
    PK_CHECK_LAUNCH();
    return PK_OK;
}
