// The tail of a training step, between loss.backward() and the next forward (reference cvivit_trainer.py:245-246, 268-269, 282 and
// phenaki_trainer.py:380-381): the global L2 norm of all gradients, the clip coefficient of torch.nn.utils.clip_grad_norm_, the in-place
// scale, and the exponential moving average of a model's weights.  All of it is bandwidth-bound streaming over the whole parameter set, so
// the launches are packed exactly as pk_adamw_multi packs them (train.hip): tensors below 256 Ki elements share launches through a per-block
// {tensor, chunk} table carried by value, the large ones go several per launch behind a prefix array of block counts.  4-byte accesses (gradient
// views are not guaranteed 16-byte aligned, and the 16-byte form of the AdamW stream was not faster).  No atomics: every block of the norm pass
// owns one slot of the partials array and the slots are summed in index order, so no result depends on scheduling or launch order.
#include "common.hpp"

namespace pk {

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

constexpr int TAIL_T = 40, TAIL_B = 512, TAIL_CHUNK = 2048;            // small tensors: the geometry of adamw_multi_kernel
constexpr int TAIL_BIG_T = 32, TAIL_BIG_CHUNK = 1024;                  // large tensors, read-modify-write streams: that of adamw_big_kernel
constexpr int SUMSQ_BIG_CHUNK = 8192;                                  // the read-only norm pass: 32 loads in flight per thread, 8x fewer partials
constexpr long TAIL_BIG_MIN = 262144;

template <int NP>
struct TailMulti {
    float* p[NP][TAIL_T];
    int n[TAIL_T];
    unsigned short bc[TAIL_B];
    unsigned char bt[TAIL_B];
};
template <int NP>
struct TailBig {
    float* p[NP][TAIL_BIG_T];
    long n[TAIL_BIG_T];
    int blk0[TAIL_BIG_T];
};
template <int NP>
struct TailSpan { float* p[NP]; long n, base; };

// the chunk of this block: tensor pointers, element count, first element
template <int NP, int CHUNK>
__device__ __forceinline__ TailSpan<NP> tail_span(const TailMulti<NP>& a, int) {
    TailSpan<NP> s;
    const int t = a.bt[blockIdx.x];
#pragma unroll
    for (int k = 0; k < NP; ++k) s.p[k] = a.p[k][t];
    s.n = a.n[t];
    s.base = (long)a.bc[blockIdx.x] * CHUNK;
    return s;
}
template <int NP, int CHUNK>
__device__ __forceinline__ TailSpan<NP> tail_span(const TailBig<NP>& a, int count) {
    TailSpan<NP> s;
    const int b = blockIdx.x;
    int t = 0;
#pragma unroll
    for (int c = 1; c < TAIL_BIG_T; ++c)
        if (c < count && b >= a.blk0[c]) t = c;
#pragma unroll
    for (int k = 0; k < NP; ++k) s.p[k] = a.p[k][t];
    s.n = a.n[t];
    s.base = (long)(b - a.blk0[t]) * CHUNK;
    return s;
}

// ---- sum of squares: one f32 per block.  Per thread a fixed-order f32 sum of its CHUNK / 256 elements, a wave-shuffle reduction, then the
// four wave sums added in a fixed order
template <class Tab, int CHUNK>
__global__ __launch_bounds__(256) void sumsq_kernel(const Tab a, int count, float* __restrict__ partials) {
    __shared__ float red[4];
    const TailSpan<1> s = tail_span<1, CHUNK>(a, count);
    const float* __restrict__ g = s.p[0];
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < CHUNK / 256; ++u) {
        const long i = s.base + u * 256 + threadIdx.x;
        const float gi = i < s.n ? g[i] : 0.f;
        acc += gi * gi;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// total_norm and the clamped coefficient of torch.nn.utils.clip_grad_norm_ (norm_type 2, error_if_nonfinite False): the partials in index order,
// in double; a NaN norm gives a NaN coefficient (torch.clamp keeps NaN), an infinite one gives 0
__global__ __launch_bounds__(256) void clip_coef_kernel(const float* __restrict__ partials, long nparts, float max_norm, float* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (long i = threadIdx.x; i < nparts; i += 256) s += (double)partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float total = (float)sqrt(red[0]);
        const float c = max_norm / (total + 1e-6f);
        out[0] = total;
        out[1] = c > 1.0f ? 1.0f : c;
    }
}

// ---- g *= *coef, in place (one rounded multiply: what torch.mul gives)
template <class Tab, int CHUNK>
__global__ __launch_bounds__(256) void scale_kernel(const Tab a, int count, const float* __restrict__ coef) {
    const TailSpan<1> s = tail_span<1, CHUNK>(a, count);
    float* __restrict__ g = s.p[0];
    const float c = coef[0];
#pragma unroll
    for (int u = 0; u < CHUNK / 256; ++u) {
        const long i = s.base + u * 256 + threadIdx.x;
        if (i >= s.n) break;
        g[i] = mul_rn(g[i], c);
    }
}

// ---- ema += w (src - ema); w >= 1 stores src verbatim (the copies of the warm-up steps are exact)
template <class Tab, int CHUNK>
__global__ __launch_bounds__(256) void ema_kernel(const Tab a, int count, float w) {
    const TailSpan<2> s = tail_span<2, CHUNK>(a, count);
    float* __restrict__ e = s.p[0];
    const float* __restrict__ x = s.p[1];
    const bool copy = w >= 1.0f;
#pragma unroll
    for (int u = 0; u < CHUNK / 256; ++u) {
        const long i = s.base + u * 256 + threadIdx.x;
        if (i >= s.n) break;
        const float xi = x[i];
        if (copy) e[i] = xi;
        else {
            const float ei = e[i];
            e[i] = ei + w * (xi - ei);
        }
    }
}

}  // namespace pk

using namespace pk;

// walks a HOST table of count x (NP + 1) 64-bit words {pointers..., numel}: every entry is checked before anything is launched, then the
// small tensors go to small(table, blocks) and the large ones to big(table, tensors, blocks) in table order
template <int NP, int BIGCHUNK, class FS, class FB>
static int tail_walk(const long long* table, int count, FS&& small, FB&& big) {
    if (!table || count <= 0) return PK_EINVAL;
    for (int i = 0; i < count; ++i) {
        const long long* e = table + (NP + 1) * (long)i;
        for (int k = 0; k < NP; ++k)
            if (!e[k]) return PK_EINVAL;
        if (e[NP] <= 0 || e[NP] > (1LL << 40)) return PK_EINVAL;
    }
    TailMulti<NP> a;
    TailBig<NP> g;
    int nt = 0, nb = 0, bt = 0;
    long bblocks = 0;
    auto flush = [&]() {
        if (nb > 0) small(a, nb);
        nt = 0; nb = 0;
    };
    auto flush_big = [&]() {
        if (bt > 0) big(g, bt, (unsigned)bblocks);
        bt = 0; bblocks = 0;
    };
    for (int i = 0; i < count; ++i) {
        const long long* e = table + (NP + 1) * (long)i;
        const long n = e[NP];
        if (n >= TAIL_BIG_MIN) {
            const long nbk = (n + BIGCHUNK - 1) / BIGCHUNK;
            if (bt == TAIL_BIG_T || bblocks + nbk > 0x7fffffffL) flush_big();
            for (int k = 0; k < NP; ++k) g.p[k][bt] = reinterpret_cast<float*>(e[k]);
            g.n[bt] = n; g.blk0[bt] = (int)bblocks;
            bblocks += nbk;
            ++bt;
            continue;
        }
        const int chunks = (int)((n + TAIL_CHUNK - 1) / TAIL_CHUNK);
        int c = 0;
        while (c < chunks) {
            if (nt == TAIL_T || nb == TAIL_B) flush();
            for (int k = 0; k < NP; ++k) a.p[k][nt] = reinterpret_cast<float*>(e[k]);
            a.n[nt] = (int)n;
            while (c < chunks && nb < TAIL_B) { a.bt[nb] = (unsigned char)nt; a.bc[nb] = (unsigned short)c; ++nb; ++c; }
            ++nt;
        }
    }
    flush();
    flush_big();
    return PK_OK;
}

// the number of f32 partial sums pk_grad_sumsq writes for this table of {g, numel} pairs (host only; < 0: PK_EINVAL)
extern "C" int pk_grad_sumsq_parts(const long long* table, int count) {
    long parts = 0;
    const int rc = tail_walk<1, SUMSQ_BIG_CHUNK>(table, count, [&](const TailMulti<1>&, int nb) { parts += nb; },
                                                 [&](const TailBig<1>&, int, unsigned blocks) { parts += blocks; });
    return rc != PK_OK ? rc : (parts > 0x7fffffffL ? PK_EINVAL : (int)parts);
}

extern "C" int pk_grad_sumsq(const long long* table, int count, float* partials, long long nparts, void* stream) {
    const int parts = pk_grad_sumsq_parts(table, count);
    if (parts < 0) return parts;
    if (!partials || nparts != parts) return PK_EINVAL;
    hipStream_t s = STREAM(stream);
    float* out = partials;
    const int rc = tail_walk<1, SUMSQ_BIG_CHUNK>(
        table, count,
        [&](const TailMulti<1>& a, int nb) {
            hipLaunchKernelGGL((sumsq_kernel<TailMulti<1>, TAIL_CHUNK>), dim3(nb), dim3(256), 0, s, a, 0, out);
            out += nb;
        },
        [&](const TailBig<1>& a, int bt, unsigned blocks) {
            hipLaunchKernelGGL((sumsq_kernel<TailBig<1>, SUMSQ_BIG_CHUNK>), dim3(blocks), dim3(256), 0, s, a, bt, out);
            out += blocks;
        });
    if (rc != PK_OK) return rc;
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_grad_clip_coef(const float* partials, long long nparts, float max_norm, float* out, void* stream) {
    if (!partials || nparts <= 0 || !out) return PK_EINVAL;
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, STREAM(stream), partials, (long)nparts, max_norm, out);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_scale_multi(const long long* table, int count, const float* coef_dev, void* stream) {
    if (!coef_dev) return PK_EINVAL;
    hipStream_t s = STREAM(stream);
    const int rc = tail_walk<1, TAIL_BIG_CHUNK>(
        table, count,
        [&](const TailMulti<1>& a, int nb) { hipLaunchKernelGGL((scale_kernel<TailMulti<1>, TAIL_CHUNK>), dim3(nb), dim3(256), 0, s, a, 0, coef_dev); },
        [&](const TailBig<1>& a, int bt, unsigned blocks) {
            hipLaunchKernelGGL((scale_kernel<TailBig<1>, TAIL_BIG_CHUNK>), dim3(blocks), dim3(256), 0, s, a, bt, coef_dev);
        });
    if (rc != PK_OK) return rc;
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_ema_multi(const long long* table, int count, float weight, void* stream) {
    if (!(weight >= 0.0f)) return PK_EINVAL;
    hipStream_t s = STREAM(stream);
    const int rc = tail_walk<2, TAIL_BIG_CHUNK>(
        table, count,
        [&](const TailMulti<2>& a, int nb) { hipLaunchKernelGGL((ema_kernel<TailMulti<2>, TAIL_CHUNK>), dim3(nb), dim3(256), 0, s, a, 0, weight); },
        [&](const TailBig<2>& a, int bt, unsigned blocks) {
            hipLaunchKernelGGL((ema_kernel<TailBig<2>, TAIL_BIG_CHUNK>), dim3(blocks), dim3(256), 0, s, a, bt, weight);
        });
    if (rc != PK_OK) return rc;
    PK_CHECK_LAUNCH();
    return PK_OK;
}
