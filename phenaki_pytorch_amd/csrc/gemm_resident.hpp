// ff1_resident_kernel: the first feed-forward GEMM (LayerNorm fold with handed-over statistics, GEGLU, bf16 out) at K = 512 in the
// A-RESIDENT form of vocab_resident_kernel (sampler.hip).  Included by gemm.hip after GemmEpilogue.
//
// The tiled 128 x 128 loop (variant 24) fills BOTH operands of every tile through the LDS-DMA ring: 256 KB per tile, 792 tiles at
// 4608 x 2736 on 512 slots (1.55 rounds), fill-bound.  Here a 128-row panel of A (128 KB at K = 512) is loaded into LDS
// once and stays; W goes global -> VGPR as the MFMA operand itself through a register ring one sub-block ahead, and the main loop has no
// workgroup barrier.
//
// Work split.  One 8-wave workgroup per CU.  panels = ceil(M / 128); `workers` workgroups share a panel (host: n_cu / panels, at least 1;
// 4608 rows on 256 CUs: 36 panels x 7 workers = 252 workgroups, one round).  The panel's S = ceil(N / 16) sub-blocks of 16 columns are cut
// into `workers` contiguous ranges [wk S / workers, (wk + 1) S / workers); a worker with Sw sub-blocks runs
//   * Sw / 8 WHOLE steps: wave w takes sub-block 8 t + w of the range, all 8 row fragments of the panel (8 MFMAs per k-chunk), then
//   * Sw % 8 SHARED steps: left-over sub-block l is cut into its 8 row fragments and wave w takes fragment w (1 MFMA per k-chunk), so a
//     left-over sub-block costs every wave one eighth of a sub-block and no wave carries a whole extra one.
// Both counts are the same for all 8 waves of a workgroup.  At 4608 x 2736 a worker has 24 or 25 sub-blocks: 3 whole steps and 0 or 1
// shared step, 3 or 3.125 sub-block equivalents per wave (mean 3.05).  (unit = panel * workers + worker) is dealt to the XCDs in
// contiguous eighths (workgroup b runs on XCD b % 8), so the workers of a panel share an L2 and W (2.8 MB) is fetched once per XCD.
//
// Start.  The ln_stats partials, the first W slice and the 128 LDS-DMA pieces of the panel (k-tile major, 2 pieces per wave and k-tile)
// are issued at entry.  The first step does not wait for the whole panel: before k-tile kt it waits until at most 2 (7 - kt) vector-memory
// operations are outstanding -- the wave's own pieces of the k-tiles after kt; whatever else is in flight was issued later and only makes
// the wait longer, never shorter -- and meets the other waves at a barrier.  Steps after the first have no barrier.  The epilogue of a step
// (fold, two GELUs per lane and fragment, store) runs inside the MFMA sub-steps of the wave's next step; only the last step's stands alone.
//
// Arithmetic.  The same v_mfma per (k-tile, k-chunk) in the same order as GemmDma::run_stats with krot = 0 (no per-wave k rotation: it would
// change the accumulation order), the row statistics summed as gemm_dma_kernel<LNF = 2> sums them (4 threads per row, 4 partials each, two
// shuffles), and the fold / GEGLU / rounding sequence of gemm_epilogue_form<EPI_FF1>: the bf16 output is bit-identical to variant 24.
// Rows at or beyond M are loaded through the descriptor's out-of-range zero and never stored.
#pragma once

namespace pk {

constexpr int FR_NT = 8;                                            // k-tiles of 64: K = 512
constexpr int FR_PANEL = FR_NT * 128 * 128;                         // the A panel: 8 k-tile blocks of [128 rows][128 B]
constexpr int FR_SMEM = FR_PANEL + 128 * 8;                         // + (sum, sum of squares) of the panel's rows

__device__ __forceinline__ void fr_wait_block(int kt) {            // (kt is a constant after unrolling)
    switch (kt) {
        case 0: wait_vmcnt<14>(); break; case 1: wait_vmcnt<12>(); break; case 2: wait_vmcnt<10>(); break; case 3: wait_vmcnt<8>(); break;
        case 4: wait_vmcnt<6>(); break; case 5: wait_vmcnt<4>(); break; case 6: wait_vmcnt<2>(); break; default: wait_vmcnt<0>(); break;
    }
}

// one step: NF row fragments (from frag0) x the 16 columns whose W slice sits in wreg; every consumed ring slot is refilled from nbase,
// the slice of the wave's next step (out of range when there is none: reads as 0, no traffic).  The A fragments of (k-tile, chunk) t + 1
// are read before the MFMAs of t (read -> wait -> MFMA per fragment leaves the LDS latency in front of every MFMA); the first step meets
// block kt of the panel just before its first read of it.
// NFP > 0: the epilogue of the wave's PREVIOUS step (NFP fragments, prev_epi(i) does fragment i) rides in this step's sub-steps, one fragment
// behind every second one: its VALU work (two GELUs per lane and fragment, ~450 cycles) issues while the MFMAs just sent are in the matrix pipe.
struct FrNoEpi { __device__ __forceinline__ void operator()(int) const {} };
template <int NF, bool FIRST, int NFP = 0, typename PrevEpi = FrNoEpi>
__device__ __forceinline__ void fr_step(const char* smem, __amdgpu_buffer_rsrc_t rsW, u32x4 (&wreg)[FR_NT][2], uint32_t nbase, int frag0, int lr, int g,
                                        f32x4 (&acc)[NF], const PrevEpi& prev_epi = PrevEpi{}) {
    static_assert(!(FIRST && NFP), "the first step has no step before it");
#pragma unroll
    for (int i = 0; i < NF; ++i) acc[i] = f32x4{0, 0, 0, 0};
    Frag<bf16> fa[2][NF];
    if (FIRST) {
        fr_wait_block(0);
        __builtin_amdgcn_s_barrier();                               // block 0 of the panel (and the row statistics) are there for every wave
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) lds_frag(fa[0][i], smem, (frag0 + i) * 16 + lr, 0, g);
#pragma unroll
    for (int t = 0; t < 2 * FR_NT; ++t) {
        const int kt = t >> 1, ch = t & 1;
        if (t + 1 < 2 * FR_NT) {
            const int kt1 = (t + 1) >> 1, ch1 = (t + 1) & 1;
            if (FIRST && ch1 == 0) {
                fr_wait_block(kt1);
                __builtin_amdgcn_s_barrier();                       // block kt1 has landed for every wave
            }
#pragma unroll
            for (int i = 0; i < NF; ++i) lds_frag(fa[(t + 1) & 1][i], smem + kt1 * 16384, (frag0 + i) * 16 + lr, ch1, g);
        }
        Frag<bf16> fw;
        fw.v = wreg[kt][ch];
#pragma unroll
        for (int i = 0; i < NF; ++i) acc[i] = mma(fw, fa[t & 1][i], acc[i]);
        wreg[kt][ch] = __builtin_amdgcn_raw_buffer_load_b128(rsW, nbase + ch * 64, kt * 128, 0);
        if (NFP == 8 && ch == 0) prev_epi(kt);
        if (NFP == 1 && t == 0) prev_epi(0);
        __builtin_amdgcn_sched_barrier(0);                          // keep this order (vocab_resident_kernel: a free schedule hoists every read and spills)
    }
}

// fold, GEGLU and store of one fragment: the sequence of gemm_epilogue_form<EPI_FF1>.  The fused multiply-adds are spelled out as the compiler
// contracts them in the tiled kernel (-ffp-contract=fast): left to it, the copies of this code came out differently contracted from one
// another (one kept rstd * inner and + t apart) and 1 output in a million differed from variant 24 by a bf16 ulp.  tests/test_ff1_resident_gpu.py
// holds the two kernels to the same bytes: a compiler that contracts the tiled epilogue differently shows up there.
__device__ __forceinline__ void fr_epi_frag(const f32x4& a, const GemmOperands& p, const GemmEpilogue& e, const float2* ls, int m0, int frag, int n,
                                            const f32x4& s4, const f32x4& t4, int lr) {
    bf16* __restrict__ Ct = reinterpret_cast<bf16*>(e.C);
    const f32x4 b4 = f32x4{0, 0, 0, 0};                             // the null bias: still added, as in the tiled forms
    const float inv_k = 1.0f / (float)p.K;
    const int ml = frag * 16 + lr, m = m0 + ml;
    const float2 pr = ls[ml];
    // E[x^2] - mean^2 has two contractions and the tiled kernel's two epilogue copies got one each: tiles inside the matrix round E[x^2],
    // edge tiles round mean^2.  The element's 128 x 128 tile decides here as well (wave-uniform: a panel is a tile row, a sub-block lies in one tile).
    const bool edge = m0 + 128 > p.M || (n & ~127) + 128 > p.N;
    const float mean = pr.x * inv_k;
    const float var = edge ? __builtin_fmaf(inv_k, pr.y, -(mean * mean)) : __builtin_fmaf(-mean, mean, pr.y * inv_k);
    const float rstd = __builtin_amdgcn_rsqf(fmaxf(var, 0.f) + e.ln_eps);
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = __builtin_fmaf(rstd, __builtin_fmaf(-mean, s4[r], a[r]), t4[r]);
    v += b4;
    const float o0 = gelu_for<bf16>(v[1]) * v[0], o1 = gelu_for<bf16>(v[3]) * v[2];
    if (m < p.M && n < p.N) store2(Ct + ((size_t)m * e.ldc + (n >> 1)), o0, o1);
}
template <int NF>
__device__ __forceinline__ void fr_epilogue(const f32x4 (&acc)[NF], const GemmOperands& p, const GemmEpilogue& e, const float2* ls, int m0, int frag0,
                                            int n, const f32x4& s4, const f32x4& t4, int lr) {
#pragma unroll
    for (int i = 0; i < NF; ++i) fr_epi_frag(acc[i], p, e, ls, m0, frag0 + i, n, s4, t4, lr);
}

__global__ __launch_bounds__(512) void ff1_resident_kernel(const GemmOperands p, const GemmEpilogue e, int workers) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef __attribute__((address_space(3))) void* lds_ptr;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, lr = lane & 15;
    const int N = p.N;
    // ---- this workgroup's (panel, worker) and the worker's range of sub-blocks
    const int panels = (p.M + 127) / 128, units = panels * workers;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int u0 = (int)((long)xcd * units / 8), u1 = (int)((long)(xcd + 1) * units / 8);
    if (idx >= u1 - u0) return;                                     // (the whole workgroup, before any barrier)
    const int unit = u0 + idx, panel = unit / workers, wk = unit - panel * workers;
    const int S = (N + 15) / 16;
    const int sb0 = (int)((long)wk * S / workers), Sw = (int)((long)(wk + 1) * S / workers) - sb0;
    if (Sw == 0) return;                                            // more workers than sub-blocks
    const int full = Sw >> 3, steps = full + (Sw & 7);
    const int m0 = panel * 128;

    const uint32_t bytesA = (uint32_t)p.M * (uint32_t)p.lda * 2u, bytesW = (uint32_t)N * (uint32_t)p.ldw * 2u;
    __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.A), 0, bytesA, 0x00020000);
    __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.W), 0, bytesW, 0x00020000);
    // sub-block of this wave's step t: whole steps first, then the shared ones
    auto sb_of = [&](int t) { return t < full ? sb0 + t * 8 + wave : sb0 + full * 8 + (t - full); };
    // byte offset of this lane's fragment row of step t's W slice (no such step / row beyond N: out of range, reads as 0)
    auto w_base = [&](int t) -> uint32_t {
        const int row = sb_of(t) * 16 + lr;
        return (t < steps && row < N) ? (uint32_t)row * (uint32_t)p.ldw * 2u + g * 16 : bytesW;
    };
    auto fold_vec = [&](const float* v, int t) {                    // ln_s / ln_t of the lane's 4 columns of step t (clamped: never stored beyond N)
        const int n = sb_of(t < steps ? t : 0) * 16 + g * 4;
        return *reinterpret_cast<const f32x4*>(v + (n < N - 4 ? n : N - 4));
    };

    // ---- issued at entry, in this order: the rows' statistics partials, the fold vectors and the W slice of step 0, the panel
    const int srow = tid >> 2, sq4 = tid & 3;                      // 4 threads per panel row, 4 of the 16 partials (K = 512) each
    const float2* st = reinterpret_cast<const float2*>(e.ln_stats) + (size_t)min(m0 + srow, p.M - 1) * e.stats_np + sq4 * 4;
    float2 pre[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) pre[u] = st[u];
    f32x4 s4 = fold_vec(e.ln_s, 0), t4 = fold_vec(e.ln_t, 0);
    u32x4 wreg[FR_NT][2];
    {
        const uint32_t base = w_base(0);
#pragma unroll
        for (int kt = 0; kt < FR_NT; ++kt)
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) wreg[kt][ch] = __builtin_amdgcn_raw_buffer_load_b128(rsW, base + ch * 64, kt * 128, 0);
    }
    __builtin_amdgcn_sched_barrier(0);                              // (the panel's pieces stay behind these loads and together)
    {
        const int lrow = lane >> 3, lslot = lane & 7, srcslot = lslot ^ lrow;      // A pieces: 8 rows x 8 slots per 1 KiB, swizzle on the source
#pragma unroll
        for (int kt = 0; kt < FR_NT; ++kt)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int piece = wave * 2 + j;
                const int gm = m0 + piece * 8 + lrow;
                const uint32_t off = gm < p.M ? (uint32_t)gm * (uint32_t)p.lda * 2u + srcslot * 16 : bytesA;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr)(smem + kt * 16384 + piece * 1024), 16, off, kt * 128, 0, 0);
            }
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- row statistics: the sums of gemm_dma_kernel<LNF = 2>, handed over through LDS behind the panel (published by the first barrier)
    float2* ls = reinterpret_cast<float2*>(smem + FR_PANEL);
    {
        float su = 0.f, sq = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) { su += pre[u].x; sq += pre[u].y; }
        su += __shfl_xor(su, 1); sq += __shfl_xor(sq, 1);
        su += __shfl_xor(su, 2); sq += __shfl_xor(sq, 2);
        // (written through asm: ahead of a store to LDS the compiler waits for every LDS-DMA in flight -- the whole panel)
        const uint32_t ls_off = (uint32_t)(uintptr_t)(lds_ptr)(ls + srow);
        const uint64_t pair = ((uint64_t)__builtin_bit_cast(uint32_t, sq) << 32) | __builtin_bit_cast(uint32_t, su);
        if (sq4 == 0) asm volatile("ds_write_b64 %0, %1" ::"v"(ls_off), "v"(pair) : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }

    // ---- steps, the epilogue of step t inside step t + 1; `prev*` is the step whose epilogue is still owed
    auto n_of = [&](int t) { return sb_of(t) * 16 + g * 4; };
    int np = n_of(0);
    f32x4 s4p = s4, t4p = t4;
    f32x4 prev1[1];
    int t = 1;
    bool owed1 = true;                                          // the owed step is a shared one (1 fragment: `wave`)
    if (full > 0) {
        f32x4 prev[8];
        fr_step<8, true>(smem, rsW, wreg, w_base(1), 0, lr, g, prev);
#pragma unroll 1
        for (; t < full; ++t) {
            const f32x4 s4c = fold_vec(e.ln_s, t), t4c = fold_vec(e.ln_t, t);
            f32x4 acc[8];
            fr_step<8, false, 8>(smem, rsW, wreg, w_base(t + 1), 0, lr, g, acc, [&](int i) { fr_epi_frag(prev[i], p, e, ls, m0, i, np, s4p, t4p, lr); });
#pragma unroll
            for (int i = 0; i < 8; ++i) prev[i] = acc[i];
            np = n_of(t); s4p = s4c; t4p = t4c;
        }
        if (t < steps) {
            const f32x4 s4c = fold_vec(e.ln_s, t), t4c = fold_vec(e.ln_t, t);
            fr_step<1, false, 8>(smem, rsW, wreg, w_base(t + 1), wave, lr, g, prev1, [&](int i) { fr_epi_frag(prev[i], p, e, ls, m0, i, np, s4p, t4p, lr); });
            np = n_of(t); s4p = s4c; t4p = t4c;
            ++t;
        } else {
            fr_epilogue<8>(prev, p, e, ls, m0, 0, np, s4p, t4p, lr);
            owed1 = false;
        }
    } else {
        fr_step<1, true>(smem, rsW, wreg, w_base(1), wave, lr, g, prev1);
    }
    if (owed1) {
#pragma unroll 1
        for (; t < steps; ++t) {
            const f32x4 s4c = fold_vec(e.ln_s, t), t4c = fold_vec(e.ln_t, t);
            f32x4 acc[1];
            fr_step<1, false, 1>(smem, rsW, wreg, w_base(t + 1), wave, lr, g, acc, [&](int) { fr_epi_frag(prev1[0], p, e, ls, m0, wave, np, s4p, t4p, lr); });
            prev1[0] = acc[0];
            np = n_of(t); s4p = s4c; t4p = t4c;
        }
        fr_epi_frag(prev1[0], p, e, ls, m0, wave, np, s4p, t4p, lr);
    }
}

}  // namespace pk
