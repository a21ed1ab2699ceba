// The perceptual network of the tokenizer's GAN objective (reference cvivit.py:349-352: torchvision's VGG16 with the last two classifier layers cut;
// :636-651: F.mse_loss(vgg(frame), vgg(recon frame)) and its gradient with respect to the reconstructed frame).  13 convolutions 3x3 / stride 1 / pad 1
// with ReLU, five 2x2 max-pools, an adaptive average pool to 7x7 and two Linear layers (the Linears are pk_gemm calls).
//
// Images are CHANNELS-LAST pixel rows x[(b, y, x)][c] (the discriminator's convention, conv.hip) with C % 8 == 0.
//
// pk_conv3x3 is a DIRECT convolution: the implicit GEMM  y[m][co] = sum_k A[m][k] W[co][k],  m = (b, y, x),  k = (ky * 3 + kx) * C + c  (pk_im2col's column
// order), whose A-tile producer gathers the nine shifted pixel rows straight from the image -- the patch matrix (9x the activations: 440 MB of f32 per
// 256 x 256 frame over the 13 layers) never exists in HBM.  The main loop is the register-staged loop of gemm_core.hpp (global -> registers -> LDS, the next
// k-tile's loads in flight over the current tile's MFMAs, 128-byte LDS rows with the slot ^ (row & 7) swizzle); only the producer differs:
//   * a thread owns ONE 16-byte k-slot of TM tile rows, so (tap, channel) of a k-tile is computed once per thread and k-tile; C % 8 == 0 keeps a slot inside
//     one tap;
//   * every row carries its own (y, x): border taps, rows of the tile tail and k >= 9 C are predicated off PER ROW (a 128-row tile spans several images
//     when H W < 128), and a predicated-off load is never issued (its address is not formed);
//   * the optional `gate` operand zeroes x[r][c] wherever gate[r][c] <= 0: with x = dy and gate = the saved post-ReLU output this is the ReLU backward
//     fused into the backward-data convolution  dx = conv3x3(dy o (y > 0), Wb),  Wb[c][((2 - ky) * 3 + (2 - kx)) * Co + co] = W[co][(ky * 3 + kx) * C + c].
// Compute types as pk_gemm: 0 exact f32, 1 bf16 MFMA (x f32 or bf16 in HBM), 2 split-bf16 (f32 rows split in registers, W in the pre-split plane format).
#include <type_traits>
#include "gemm_core.hpp"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

using namespace pk;

struct ConvArgs {
    const void* x;       // [M][C]      TA
    const void* w;       // [N][ldw]    T (operand image, K zero-padded to the k-tile)
    const void* gate;    // [M][ldg]    f32 or bf16, or null
    const float* bias;   // [N] or null
    void* y;             // [M][ldy]    f32 or T
    int H, W, C, ldw, ldg, ldy;
    int M, N, K;         // M = B H W, N = Co, K = 9 C
    int relu, out_f32;
};

// the gate values of one A slot (NE = 8 or 4 consecutive channels) and the bit mask "gate > 0" of them
template <int NE, typename GT> struct GateSlot;
template <> struct GateSlot<8, float> { f32x4 a, b; };
template <> struct GateSlot<4, float> { f32x4 a; };
template <> struct GateSlot<8, bf16> { u32x4 v; };
template <> struct GateSlot<4, bf16> { u32x2 v; };

__device__ __forceinline__ void gate_load(GateSlot<8, float>& r, const float* p, bool ok) {
    if (ok) { r.a = *reinterpret_cast<const f32x4*>(p); r.b = *reinterpret_cast<const f32x4*>(p + 4); }
    else { r.a = f32x4{0, 0, 0, 0}; r.b = r.a; }
}
__device__ __forceinline__ void gate_load(GateSlot<4, float>& r, const float* p, bool ok) {
    r.a = ok ? *reinterpret_cast<const f32x4*>(p) : f32x4{0, 0, 0, 0};
}
__device__ __forceinline__ void gate_load(GateSlot<8, bf16>& r, const bf16* p, bool ok) {
    r.v = ok ? *reinterpret_cast<const u32x4*>(p) : u32x4{0, 0, 0, 0};
}
__device__ __forceinline__ void gate_load(GateSlot<4, bf16>& r, const bf16* p, bool ok) {
    r.v = ok ? *reinterpret_cast<const u32x2*>(p) : u32x2{0, 0};
}
__device__ __forceinline__ unsigned pos_bits4(const f32x4& v, int sh) {
    return ((v[0] > 0.f ? 1u : 0u) | (v[1] > 0.f ? 2u : 0u) | (v[2] > 0.f ? 4u : 0u) | (v[3] > 0.f ? 8u : 0u)) << sh;
}
__device__ __forceinline__ unsigned pos_bits2(uint32_t w, int sh) {      // two bf16: element 2i in the low half
    return ((bf2f((u16)(w & 0xFFFFu)) > 0.f ? 1u : 0u) | (bf2f((u16)(w >> 16)) > 0.f ? 2u : 0u)) << sh;
}
__device__ __forceinline__ unsigned gate_bits(const GateSlot<8, float>& r) { return pos_bits4(r.a, 0) | pos_bits4(r.b, 4); }
__device__ __forceinline__ unsigned gate_bits(const GateSlot<4, float>& r) { return pos_bits4(r.a, 0); }
__device__ __forceinline__ unsigned gate_bits(const GateSlot<8, bf16>& r) {
    return pos_bits2(r.v[0], 0) | pos_bits2(r.v[1], 2) | pos_bits2(r.v[2], 4) | pos_bits2(r.v[3], 6);
}
__device__ __forceinline__ unsigned gate_bits(const GateSlot<4, bf16>& r) { return pos_bits2(r.v[0], 0) | pos_bits2(r.v[1], 2); }

// zero the elements of a raw A slot whose bit is clear
__device__ __forceinline__ void gate_apply(RawSlot<bf16, float>& r, unsigned bits) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r.a[e] = (bits >> e) & 1u ? r.a[e] : 0.f;
        r.b[e] = (bits >> (4 + e)) & 1u ? r.b[e] : 0.f;
    }
}
__device__ __forceinline__ void gate_apply(RawSlot<bf16, bf16>& r, unsigned bits) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        r.v[i] &= ((bits >> (2 * i)) & 1u ? 0x0000FFFFu : 0u) | ((bits >> (2 * i + 1)) & 1u ? 0xFFFF0000u : 0u);
}
template <typename T>      // 4-byte elements (exact f32, split-bf16)
__device__ __forceinline__ void gate_apply(RawSlot<T, T>& r, unsigned bits) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[i] = (bits >> i) & 1u ? r.v[i] : 0u;
}

struct NoGate {};

// T: operand type of the product (float | bf16 | bf16x3); TA: element type of x in HBM (float for T = bf16 with f32 rows, else T);
// GT: element type of the gate (NoGate: none)
template <typename T, typename TA, int TM, int TN, typename GT>
__global__ __launch_bounds__(256) void conv3x3_kernel(const ConvArgs p) {
    constexpr int BM = 32 * TM, BN = 32 * TN;
    constexpr int EPS = 16 / (int)sizeof(T);     // elements per 16-byte LDS slot = channels per A slot
    constexpr int BK = 8 * EPS;                  // k per tile: 64 bf16, 32 otherwise
    constexpr int CH = BK / 32;
    constexpr bool GATED = !__is_same(GT, NoGate);
    typedef typename std::conditional<GATED, GT, float>::type G;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 4, lr = lane & 15;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    auto sA = [&](int buf) { return smem + buf * (BM + BN) * 128; };      // two stages of [A tile | W tile]
    auto sW = [&](int buf) { return smem + buf * (BM + BN) * 128 + BM * 128; };

    const TA* X = reinterpret_cast<const TA*>(p.x);
    const T* Wp = reinterpret_cast<const T*>(p.w);
    const G* Gp = reinterpret_cast<const G*>(p.gate);

    // slot s = tid + i * 256 -> tile row = s >> 3, k-slot = s & 7: a thread's TM rows share one k-slot
    const int sl = tid & 7;
    int py[TM], px[TM];
    long pix[TM];
    bool a_ok[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int gm = m0 + (tid >> 3) + i * 32;
        a_ok[i] = gm < p.M;
        const int m = a_ok[i] ? gm : 0;
        px[i] = m % p.W;
        py[i] = (m / p.W) % p.H;
        pix[i] = m;
    }
    const T* w_src[TN];
    bool w_ok[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int gn = n0 + (tid >> 3) + j * 32;
        w_ok[j] = gn < p.N;
        w_src[j] = Wp + (size_t)(w_ok[j] ? gn : 0) * p.ldw + sl * EPS;      // ldw >= K rounded up to BK (host): every k-tile of a live row is readable
    }

    RawSlot<T, TA> ra[TM];
    GateSlot<EPS, G> rg[TM];
    RawSlot<T, T> rw[TN];
    auto gload = [&](int k0) {
        const int k = k0 + sl * EPS;
        const int tap = k / p.C, c = k - tap * p.C;           // tap >= 9 <=> k >= K: the zero padding of the k-tile
        const int ky = tap / 3, kx = tap - ky * 3;
        const int dy = ky - 1, dx = kx - 1;
        const long shift = (long)dy * p.W + dx;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const bool ok = a_ok[i] && tap < 9 && (unsigned)(py[i] + dy) < (unsigned)p.H && (unsigned)(px[i] + dx) < (unsigned)p.W;
            const long q = ok ? pix[i] + shift : 0;           // the shifted pixel is in the same image: its row index is m + dy W + dx
            raw_load(ra[i], X + q * p.C + (ok ? c : 0), ok);
            if (GATED) gate_load(rg[i], Gp + q * p.ldg + (ok ? c : 0), ok);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) raw_load(rw[j], w_src[j] + k0, w_ok[j]);
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row = (tid >> 3) + i * 32;
            if (GATED) gate_apply(ra[i], gate_bits(rg[i]));
            *reinterpret_cast<u32x4*>(sA(buf) + row * 128 + ((sl ^ (row & 7)) << 4)) = raw_pack(ra[i]);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int row = (tid >> 3) + j * 32;
            *reinterpret_cast<u32x4*>(sW(buf) + row * 128 + ((sl ^ (row & 7)) << 4)) = raw_pack(rw[j]);
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

    const int nt = (p.K + BK - 1) / BK;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        if (t + 1 < nt) gload((t + 1) * BK);
        const char* a = sA(buf);
        const char* w = sW(buf);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            Frag<T> fa[TM], fw[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) lds_frag_a<T>(fa[i], a, wm * 16 * TM + i * 16 + lr, c, g);
#pragma unroll
            for (int j = 0; j < TN; ++j) lds_frag_w<T>(fw[j], w, wn * 16 * TN + j * 16 + lr, c, g);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = mma(fw[j], fa[i], acc[i][j]);
        }
        if (t + 1 < nt) lstore(buf ^ 1);
        __syncthreads();
    }

    // epilogue: lane l holds 4 consecutive output channels of one pixel row (gemm_core.hpp); N % 4 == 0
    float* Yf = reinterpret_cast<float*>(p.y);
    bf16* Yb = reinterpret_cast<bf16*>(p.y);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * 16 * TN + j * 16 + g * 4;
        if (n >= p.N) continue;
        const f32x4 b4 = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m0 + wm * 16 * TM + i * 16 + lr;
            if (m >= p.M) continue;
            f32x4 v = acc[i][j] + b4;
            if (p.relu) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            }
            const size_t o = (size_t)m * p.ldy + n;
            if (p.out_f32) store4(Yf + o, v); else store4(Yb + o, v);
        }
    }
}

// ---- pooling on channels-last rows, 4 channels per thread ----------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4(const bf16* p) {
    const u32x2 v = *reinterpret_cast<const u32x2*>(p);
    return f32x4{bf2f((u16)(v[0] & 0xFFFFu)), bf2f((u16)(v[0] >> 16)), bf2f((u16)(v[1] & 0xFFFFu)), bf2f((u16)(v[1] >> 16))};
}

// y[(b, yo, xo)][c] = max over the 2 x 2 window at (2 yo, 2 xo); Ho = H / 2, Wo = W / 2 (floor: an odd last row / column is not read)
template <typename T>
__global__ void maxpool_kernel(const T* __restrict__ x, int H, int W, int C4, int Ho, int Wo, T* __restrict__ y, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    const long r = i / C4;
    const int xo = (int)(r % Wo), yo = (int)((r / Wo) % Ho);
    const long b = r / ((long)Wo * Ho);
    const T* s = x + (((b * H + 2 * yo) * W + 2 * xo) * (long)C4 + c4) * 4;
    const long dx = (long)C4 * 4, dy = (long)W * C4 * 4;
    f32x4 m = ld4(s);
    const f32x4 v1 = ld4(s + dx), v2 = ld4(s + dy), v3 = ld4(s + dy + dx);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        m[e] = v1[e] > m[e] ? v1[e] : m[e];
        m[e] = v2[e] > m[e] ? v2[e] : m[e];
        m[e] = v3[e] > m[e] ? v3[e] : m[e];
    }
    store4(y + i * 4, m);
}

// dx[(b, y, x)][c] = dy[(b, y / 2, x / 2)][c] if (y, x) is the FIRST maximum of its window in scan order (0,0), (0,1), (1,0), (1,1) -- torch's rule:
// windows of four equal values (zeros after a ReLU) route to (0, 0) --, else 0; recomputed from the saved input, gather form, no atomics
template <typename T>
__global__ void maxpool_bwd_kernel(const T* __restrict__ x, const float* __restrict__ dy, int H, int W, int C4, int Ho, int Wo, float* __restrict__ dx,
                                   long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    const long r = i / C4;
    const int xx = (int)(r % W), yy = (int)((r / W) % H);
    const long b = r / ((long)W * H);
    const int yo = yy >> 1, xo = xx >> 1;
    f32x4 out = f32x4{0, 0, 0, 0};
    if (yo < Ho && xo < Wo) {
        const T* s = x + (((b * H + 2 * yo) * W + 2 * xo) * (long)C4 + c4) * 4;
        const long sx = (long)C4 * 4, sy = (long)W * C4 * 4;
        const f32x4 v0 = ld4(s), v1 = ld4(s + sx), v2 = ld4(s + sy), v3 = ld4(s + sy + sx);
        const f32x4 gy = ld4(dy + (((b * Ho + yo) * Wo + xo) * (long)C4 + c4) * 4);
        const int mine = (yy & 1) * 2 + (xx & 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float m = v0[e];
            int idx = 0;
            if (v1[e] > m) { m = v1[e]; idx = 1; }
            if (v2[e] > m) { m = v2[e]; idx = 2; }
            if (v3[e] > m) { m = v3[e]; idx = 3; }
            out[e] = idx == mine ? gy[e] : 0.f;
        }
    }
    *reinterpret_cast<f32x4*>(dx + i * 4) = out;
}

constexpr int AP = 7;      // nn.AdaptiveAvgPool2d((7, 7)) of torchvision's VGG
__device__ __forceinline__ int ap_start(int i, int s) { return (i * s) / AP; }                 // floor(i s / 7)
__device__ __forceinline__ int ap_end(int i, int s) { return ((i + 1) * s + AP - 1) / AP; }    // ceil((i + 1) s / 7)

// out[(b, i, j)][c] = mean of x over rows [floor(i H / 7), ceil((i + 1) H / 7)) x columns [floor(j W / 7), ceil((j + 1) W / 7))
template <typename T>
__global__ void avgpool_kernel(const T* __restrict__ x, int H, int W, int C4, float* __restrict__ out, long total) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c4 = (int)(t % C4);
    const long r = t / C4;
    const int j = (int)(r % AP), i = (int)((r / AP) % AP);
    const long b = r / (AP * AP);
    const int y0 = ap_start(i, H), y1 = ap_end(i, H), x0 = ap_start(j, W), x1 = ap_end(j, W);
    f32x4 acc = f32x4{0, 0, 0, 0};
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) acc += ld4(x + (((b * H + yy) * W + xx) * (long)C4 + c4) * 4);
    const float area = (float)((y1 - y0) * (x1 - x0));
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] /= area;
    *reinterpret_cast<f32x4*>(out + t * 4) = acc;
}

// the adjoint in gather form: dx[(b, y, x)][c] = sum over the (at most 2 x 2) windows that contain (y, x) of dy[(b, i, j)][c] / area(i, j), in (i, j) order
__global__ void avgpool_bwd_kernel(const float* __restrict__ dy, int H, int W, int C4, float* __restrict__ dx, long total) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c4 = (int)(t % C4);
    const long r = t / C4;
    const int xx = (int)(r % W), yy = (int)((r / W) % H);
    const long b = r / ((long)W * H);
    f32x4 acc = f32x4{0, 0, 0, 0};
    for (int i = 0; i < AP; ++i) {
        const int y0 = ap_start(i, H), y1 = ap_end(i, H);
        if (yy < y0 || yy >= y1) continue;
        for (int j = 0; j < AP; ++j) {
            const int x0 = ap_start(j, W), x1 = ap_end(j, W);
            if (xx < x0 || xx >= x1) continue;
            const float area = (float)((y1 - y0) * (x1 - x0));
            const f32x4 v = ld4(dy + (((b * AP + i) * AP + j) * (long)C4 + c4) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += v[e] / area;
        }
    }
    *reinterpret_cast<f32x4*>(dx + t * 4) = acc;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline unsigned nblk(long total) { return (unsigned)((total + 255) / 256); }

template <typename T, typename TA, int TM, int TN, typename GT>
int launch_conv(const ConvArgs& a, hipStream_t s) {
    constexpr int BM = 32 * TM, BN = 32 * TN, lds = 2 * (BM + BN) * 128;
    const dim3 grid((a.M + BM - 1) / BM, (a.N + BN - 1) / BN);
    hipLaunchKernelGGL((conv3x3_kernel<T, TA, TM, TN, GT>), grid, dim3(256), lds, s, a);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

template <typename T, typename TA, typename GT>
int launch_conv_tile(const ConvArgs& a, int tile, hipStream_t s) {
    switch (tile) {
        case 1: return launch_conv<T, TA, 2, 2, GT>(a, s);      // 64 x 64
        case 2: return launch_conv<T, TA, 4, 2, GT>(a, s);      // 128 x 64
        default: return launch_conv<T, TA, 4, 4, GT>(a, s);     // 128 x 128
    }
}

template <typename T, typename TA>
int launch_conv_gate(const ConvArgs& a, int gate_kind, int tile, hipStream_t s) {
    if (gate_kind == 0) return launch_conv_tile<T, TA, NoGate>(a, tile, s);
    if (gate_kind == 1) return launch_conv_tile<T, TA, float>(a, tile, s);
    return launch_conv_tile<T, TA, bf16>(a, tile, s);
}

}  // namespace

// which tile pk_conv3x3 picks for tile = 0: 128 x 128 once there is one per CU (256), 128 x 64 for the same row count when Co <= 64 (no half-empty weight
// tile), else 64 x 64 -- the deep layers are short and wide (16 frames of 256 x 256 at conv5: M = 4096, Co = 512 -> 128 tiles of 128 x 128 on 256 CUs,
// 512 of 64 x 64)
static int conv_auto_tile(long M, int N) {
    const long mt128 = (M + 127) / 128;
    if (N <= 64) return mt128 >= 256 ? 2 : 1;
    return mt128 * ((N + 127) / 128) >= 256 ? 3 : 1;
}

extern "C" int pk_conv3x3(int dtype, int a_is_f32, const void* x, int B, int H, int W, int C, const void* Wm, int ldw, int Co, const float* bias, int act,
                          const void* gate, int ldg, int gate_is_f32, void* y, int ldy, int out_is_f32, int tile, void* stream) {
    if (!x || !Wm || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || Co <= 0) return PK_EINVAL;
    if (dtype < 0 || dtype > 2 || act < 0 || act > 1 || tile < 0 || tile > 3) return PK_EINVAL;
    if (dtype != 1 && (!a_is_f32 || !out_is_f32)) return PK_EINVAL;      // exact-f32 and split-bf16 keep every activation f32
    const long M = (long)B * H * W;
    if (M > 0x7FFFFFFFl - 256 || C > (0x7FFFFFFF - 64) / 9) return PK_EINVAL;
    const int K = 9 * C, bk = dtype == 1 ? 64 : 32;
    if (ldw < (K + bk - 1) / bk * bk || ldy < Co || (gate && ldg < C)) return PK_EINVAL;
    if ((C & 7) || (Co & 3) || (ldy & 3) || (ldw & (dtype == 1 ? 7 : 3)) || (gate && (ldg & 7))) return PK_EALIGN;
    if (!al16(x) || !al16(Wm) || !al16(y) || (bias && !al16(bias)) || (gate && !al16(gate))) return PK_EALIGN;
    if ((Co + 31) / 32 > 65535) return PK_EINVAL;
    const ConvArgs a{x, Wm, gate, bias, y, H, W, C, ldw, ldg, ldy, (int)M, Co, K, act, out_is_f32};
    const int gk = gate ? (gate_is_f32 ? 1 : 2) : 0;
    if (tile == 0) tile = conv_auto_tile(M, Co);
    hipStream_t s = STREAM(stream);
    if (dtype == 0) return launch_conv_gate<float, float>(a, gk, tile, s);
    if (dtype == 2) return launch_conv_gate<bf16x3, bf16x3>(a, gk, tile, s);
    return a_is_f32 ? launch_conv_gate<bf16, float>(a, gk, tile, s) : launch_conv_gate<bf16, bf16>(a, gk, tile, s);
}

extern "C" int pk_maxpool2x2(int is_f32, const void* x, int B, int H, int W, int C, void* y, void* stream) {
    if (!x || !y || B <= 0 || H < 2 || W < 2 || C <= 0) return PK_EINVAL;
    if ((C & 3) || !al8(x) || !al8(y) || (is_f32 && (!al16(x) || !al16(y)))) return PK_EALIGN;
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)B * Ho * Wo * (C / 4);
    if (total > 0x7FFFFFFFl * 256) return PK_EINVAL;
    if (is_f32) hipLaunchKernelGGL(maxpool_kernel<float>, dim3(nblk(total)), dim3(256), 0, STREAM(stream), reinterpret_cast<const float*>(x), H, W, C / 4,
                                   Ho, Wo, reinterpret_cast<float*>(y), total);
    else hipLaunchKernelGGL(maxpool_kernel<pk::bf16>, dim3(nblk(total)), dim3(256), 0, STREAM(stream), reinterpret_cast<const pk::bf16*>(x), H, W, C / 4,
                            Ho, Wo, reinterpret_cast<pk::bf16*>(y), total);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_maxpool2x2_bwd(int is_f32, const void* x, const float* dy, int B, int H, int W, int C, float* dx, void* stream) {
    if (!x || !dy || !dx || B <= 0 || H < 2 || W < 2 || C <= 0) return PK_EINVAL;
    if ((C & 3) || !al8(x) || (is_f32 && !al16(x)) || !al16(dy) || !al16(dx)) return PK_EALIGN;
    const long total = (long)B * H * W * (C / 4);
    if (total > 0x7FFFFFFFl * 256) return PK_EINVAL;
    if (is_f32) hipLaunchKernelGGL(maxpool_bwd_kernel<float>, dim3(nblk(total)), dim3(256), 0, STREAM(stream), reinterpret_cast<const float*>(x), dy, H, W,
                                   C / 4, H / 2, W / 2, dx, total);
    else hipLaunchKernelGGL(maxpool_bwd_kernel<pk::bf16>, dim3(nblk(total)), dim3(256), 0, STREAM(stream), reinterpret_cast<const pk::bf16*>(x), dy, H, W,
                            C / 4, H / 2, W / 2, dx, total);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_adaptive_avgpool(int is_f32, const void* x, int B, int H, int W, int C, float* out, void* stream) {
    if (!x || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || H > 0x7FFFFFFF / 8 || W > 0x7FFFFFFF / 8) return PK_EINVAL;
    if ((C & 3) || !al8(x) || (is_f32 && !al16(x)) || !al16(out)) return PK_EALIGN;
    const long total = (long)B * AP * AP * (C / 4);
    if (total > 0x7FFFFFFFl * 256) return PK_EINVAL;
    if (is_f32) hipLaunchKernelGGL(avgpool_kernel<float>, dim3(nblk(total)), dim3(256), 0, STREAM(stream), reinterpret_cast<const float*>(x), H, W, C / 4, out,
                                   total);
    else hipLaunchKernelGGL(avgpool_kernel<pk::bf16>, dim3(nblk(total)), dim3(256), 0, STREAM(stream), reinterpret_cast<const pk::bf16*>(x), H, W, C / 4,
                            out, total);
    PK_CHECK_LAUNCH();
    return PK_OK;
}

extern "C" int pk_adaptive_avgpool_bwd(const float* dy, int B, int H, int W, int C, float* dx, void* stream) {
    if (!dy || !dx || B <= 0 || H <= 0 || W <= 0 || C <= 0 || H > 0x7FFFFFFF / 8 || W > 0x7FFFFFFF / 8) return PK_EINVAL;
    if ((C & 3) || !al16(dy) || !al16(dx)) return PK_EALIGN;
    const long total = (long)B * H * W * (C / 4);
    if (total > 0x7FFFFFFFl * 256) return PK_EINVAL;
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(nblk(total)), dim3(256), 0, STREAM(stream), dy, H, W, C / 4, dx, total);
    PK_CHECK_LAUNCH();
    return PK_OK;
}
