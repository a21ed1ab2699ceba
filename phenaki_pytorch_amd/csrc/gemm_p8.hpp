// Two-group main loop (bf16): 256 x 256 macro-tile, 8 waves (2 x 4), ONE workgroup per CU, two phases of 32 MFMAs per k-tile, LDS-DMA HALF-tiles
// (128 rows x 128 B = 16 KB) in a ring of 8, one counted vmcnt per phase, two 4-wave groups a barrier apart.  Same operand image (128-byte LDS rows,
// 16-B slot ^ (row & 7) on the DMA source and on the read), same fragment geometry and the same transposed product (lane = 4 consecutive output
// columns of one row) as gemm_dma.hpp, so every epilogue of gemm.hip applies unchanged to a quadrant of the tile.  gemm.hip drives it as variant 50
// (gemm_p8_kernel) and as pk_gemm_splitk's tile = 2 (gemm_p8_splitk_kernel).
//
// Why this shape (profiles/gemm_vendor_r06.txt): the 128 x 128 ring waits for a WHOLE k-tile, passes a workgroup barrier and consumes it; its MFMA
// pipe idles through wait + barrier + DMA issue (28 % busy, profiles/gemm_pmc_r02.txt) and two co-resident workgroups only partly hide that in each
// other.  Here
//   * a wave owns 128 x 64 of the output as 2 x 2 QUADRANTS of 64 x 32: quadrant (a, b) = rows a*128 + wr*64 .. +64, columns b*128 + wc*32 .. +32 --
//     every wave reads from all four half-tiles (A0, A1, B0, B1) of a k-tile, 12 KB of fragments per 64 MFMAs (the 128 x 128 8-wave loop: 6 KB per 16);
//   * a phase = [load part: DMA issue, this phase's fragment reads, vmcnt, lgkmcnt(0)] s_barrier [32 MFMAs of two quadrants] s_barrier.  Waves 4-7 run
//     one barrier behind waves 0-3, and wave w shares its SIMD with wave w + 4, so on every SIMD one wave's MFMAs run beside the other's LDS / DMA
//     issue (matrix beside memory, the complementary pairing);
//   * ring slots of k-tile t: 4 * (t & 1) + {0: B0, 1: B1, 2: A0, 3: A1};
//   * phase 0: issues A1 of k-tile t + 1, reads B0, B1, A0 (16 x ds_read_b128), 32 MFMAs of quadrants (0,0), (0,1);
//     phase 1: issues B0, B1, A0 of k-tile t + 2 (their slots died with phase 0's reads), reads A1 (8), 32 MFMAs of (1,1), (1,0) -- A1's fragments
//     replace A0's, both B fragment sets stay in registers across the k-tile;
//   * every fragment read is retired (lgkmcnt(0)) BEFORE its phase's first barrier, so the later group's reads of a slot precede the earlier group's
//     re-fill of it by a barrier: B0 / B1 / A0 of k-tile t are read before phase 0's first barrier and re-filled after its second; A1 of k-tile t - 1
//     is read before phase 1's first barrier and its slot re-filled (A1 of t + 1) after phase 1's second;
//   * a half-tile is 2 DMA pieces per wave.  One vmcnt(8) per phase: phase 0 (10 pieces in flight) retires A1 of THIS k-tile (issued a whole k-tile
//     earlier, read in phase 1), phase 1 (14 in flight) retires B0 / B1 / A0 of k-tile t + 1 (issued a k-tile earlier, read in the next phase 0).  A
//     wave's vmcnt covers its own pieces; the barrier behind it covers the other waves'.  Tail: with nothing issued for t + 2 phase 1 waits with
//     vmcnt(2) (A1 of t + 1 stays in flight), the last k-tile with vmcnt(0); the prologue issues k-tile 0 whole and B0 / B1 / A0 of k-tile 1.
// Accumulators: acc[a][b][i][j] = 16 x 16 block (i, j) of quadrant (a, b); C row = m0 + a*128 + wr*64 + i*16 + (lane & 15),
// column = n0 + b*128 + wc*32 + j*16 + (lane >> 4)*4 + r -- i.e. gemm_epilogue<bf16, 4, 2, 4> at (m0 + a*128, n0 + b*128).
//
// Lineage (measurements: profiles/gemm_p8_r06.txt; the file, struct and kernel names keep the first form's "p8"):
//   * the first form had 8 phases per k-tile-pair (4 per k-tile, 16 MFMAs and one half-tile of DMA each).  With NO loads at all its barrier skeleton
//     tops out at 1.6 PF -- every s_barrier costs the SIMD a ~60-80-cycle MFMA bubble, 8 of them per 2048 MFMA-cycles -- so the phases were made
//     twice as long and the 8-phase loop removed.  profiles/gemm_p8_r06.txt.
//   * a split-bf16 instantiation (f32 A rows split into (hi, lo) planes right after the ds_reads, host-packed W planes, three MFMAs per fragment
//     pair) was bit-identical to variant 24 and is NOT used: that mode is bound by its MFMA count, not by the fill (8192^3 390 vs 352 TF-equivalent,
//     FF1 at 4608 rows 107 vs 61 us).  Removed; this struct is bf16 only.  profiles/gemm_p8_r06.txt.
//   * all 24 fragment reads of a k-tile in phase 0 (+32 VGPRs: 250), all 8 DMA pieces of k-tile t + 2 in phase 1, one vmcnt(8) per k-tile -- built on
//     the reading that a DMA piece beside ds_read traffic is what makes a load part long; bit-identical, 1.323 vs 1.309 PF at 8192^3 and equal on the
//     K = 512 shapes: no gain, removed.  profiles/gemm_p8_r06.txt.
//   * a persistent tile-stream form -- one workgroup per CU walking a tile list with the ring running on across tile boundaries, the next tile's
//     first k-tiles prefetched under the current tile's last, a register-lean epilogue between -- was parity-green and SLOWER than one tile per
//     workgroup on every shape (8192^3 1.13-1.19 vs 1.33-1.35 PF; 36864 x 2736 x 512 with the GEGLU epilogue 211 vs 183 us, the 128 x 128 loop 148):
//     vmcnt counts the epilogue's stores in order with the DMA pieces, so the first counted wait behind an epilogue waits for the stores'
//     acknowledgements; the per-tile offsets no longer fit beside 128 accumulators + 64 fragment registers and have to be rebuilt per DMA piece in
//     the load part of a phase, which is this loop's critical path.  Removed.  profiles/gemm_p8_r06.txt.
//   * the timing ablations behind those numbers (no DMA, no reads, no stagger, no s_setprio, other issue orders, 32x32x16 MFMAs, extra VGPR loads)
//     were compile-time switches of this file up to commit dad914b.  profiles/gemm_p8_r06.txt.
#pragma once
#include "gemm_dma.hpp"

namespace pk {

struct GemmP8 {
    static constexpr int BM = 256, BN = 256, THREADS = 512, ROWB = 128;
    static constexpr int BK = ROWB / (int)sizeof(bf16);   // 64
    static constexpr int CH = BK / 32;
    static constexpr int HALF = 128 * ROWB;               // one half-tile: 16 KB = 16 DMA pieces of 1 KiB, 2 per wave
    static constexpr int SMEM = 8 * HALF;
    typedef __attribute__((address_space(3))) void* lds_ptr;
    typedef f32x4 QuadAcc[4][2];
    typedef QuadAcc Acc[2][2];
    enum { B0 = 0, A0 = 1, B1 = 2, A1 = 3 };              // half-tile types: bit 0 = operand (0: W, 1: A), bit 1 = which 128 rows

    struct Ctx {
        __amdgpu_buffer_rsrc_t rsA, rsW;
        uint32_t bytesA, bytesW;
        uint32_t offA[2][2], offW[2][2];                 // [half][piece] per-lane source offsets at k = 0
        int nt, rot;
        bool slot_in_tail;
        char* smem;
        int piece0;                                       // wave * 2: first DMA piece of a half-tile this wave issues
        int rdA, rdB;                                     // per-lane LDS byte offsets of the fragment reads inside a half-tile, chunk 0 (chunk 1: ^ 64)
    };

    // half-tile TYPE of k-tile kt into ring slot SLOT
    static __device__ __forceinline__ void issue(const int TYPE, const int SLOT, const Ctx& c, int kt) {
        int kk = kt + c.rot;
        if (kk >= c.nt) kk -= c.nt;
        const int koff = kk * ROWB;
        const bool cut = kk == c.nt - 1 && !c.slot_in_tail;
        char* base = c.smem + SLOT * HALF + c.piece0 * 1024;
        const int h = TYPE >> 1;
#pragma unroll
        for (int pi = 0; pi < 2; ++pi) {
            if (TYPE & 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(c.rsA, (lds_ptr)(base + pi * 1024), 16, cut ? c.bytesA : c.offA[h][pi], koff, 0, 0);
            else          __builtin_amdgcn_raw_ptr_buffer_load_lds(c.rsW, (lds_ptr)(base + pi * 1024), 16, c.offW[h][pi], koff, 0, 0);
        }
    }

    // NF = 4: A fragments (rows of the wave's 64-row sub-tile), NF = 2: W fragments (its 32 columns)
    template <int SLOT, int NF>
    static __device__ __forceinline__ void read_frags(const Ctx& c, int rd, Frag<bf16> (&f)[NF][CH]) {
        const char* s = c.smem + SLOT * HALF;
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) f[i][ch].v = *reinterpret_cast<const u32x4*>(s + ((rd + i * 16 * ROWB) ^ (ch * 64)));
    }

    static __device__ __forceinline__ void quad(f32x4 (&q)[4][2], const Frag<bf16> (&fa)[4][CH], const Frag<bf16> (&fb)[2][CH]) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) q[i][j] = mma(fb[j][ch], fa[i][ch], q[i][j]);
        __builtin_amdgcn_s_setprio(0);
    }

    static __device__ __forceinline__ void bar() {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    }

    // a_nrows = physical rows behind p.A
    static __device__ __forceinline__ void setup(Ctx& c, const GemmOperands& p, int a_nrows, int m0, int n0, char* smem) {
        const int tid = threadIdx.x, lane = tid & 63;
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int wr = wave >> 2, wc = wave & 3, g = lane >> 4, lr = lane & 15;
        constexpr int SZ = (int)sizeof(bf16);
        c.smem = smem;
        c.piece0 = wave * 2;
        c.bytesA = (uint32_t)a_nrows * (uint32_t)p.lda * SZ;
        c.bytesW = (uint32_t)p.N * (uint32_t)p.ldw * SZ;
        c.rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.A), 0, c.bytesA, 0x00020000);
        c.rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.W), 0, c.bytesW, 0x00020000);
        const int lrow = lane >> 3, lslot = lane & 7, srcslot = lslot ^ (lrow & 7);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) {
                const int row = h * 128 + wave * 16 + pi * 8 + lrow;
                int gm = m0 + row;
                const bool ok = gm < p.M;
                if (ok && p.a_rows) gm = p.a_rows[gm];
                c.offA[h][pi] = ok ? (uint32_t)gm * (uint32_t)p.lda * SZ + srcslot * 16 : c.bytesA;
                const int gn = n0 + row;
                c.offW[h][pi] = gn < p.N ? (uint32_t)gn * (uint32_t)p.ldw * SZ + srcslot * 16 : c.bytesW;
            }
        c.nt = (p.K + BK - 1) / BK;
        c.rot = (p.krot && c.nt > 1) ? (int)(((blockIdx.x >> 3) + blockIdx.y) % (unsigned)c.nt) : 0;
        const int ktail_bytes = (p.K * SZ) % ROWB;
        c.slot_in_tail = ktail_bytes == 0 || srcslot * 16 < ktail_bytes;
        // fragment reads: row (base + lr) of a half-tile, 16-B slot (ch*4 + g) ^ (row & 7); row bases are multiples of 16, so row & 7 = lr & 7
        c.rdA = (wr * 64 + lr) * ROWB + ((g ^ (lr & 7)) << 4);
        c.rdB = (wc * 32 + lr) * ROWB + ((g ^ (lr & 7)) << 4);
    }

    // one k-tile (ring parity E = kt & 1)
    template <int E>
    static __device__ __forceinline__ void ktile(const Ctx& c, int kt, Acc& acc, Frag<bf16> (&fa)[4][CH], Frag<bf16> (&fb0)[2][CH], Frag<bf16> (&fb1)[2][CH]) {
        constexpr int S = 4 * E, SN = 4 * (E ^ 1);
        const bool more1 = kt + 1 < c.nt, more2 = kt + 2 < c.nt;
        // ---- phase 0
        if (more1) issue(A1, SN + 3, c, kt + 1);
        read_frags<S + 0, 2>(c, c.rdB, fb0);
        read_frags<S + 1, 2>(c, c.rdB, fb1);
        read_frags<S + 2, 4>(c, c.rdA, fa);
        if (more1) wait_vmcnt<8>(); else wait_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        bar();
        quad(acc[0][0], fa, fb0);
        quad(acc[0][1], fa, fb1);
        bar();
        // ---- phase 1
        if (more2) { issue(B0, S + 0, c, kt + 2); issue(B1, S + 1, c, kt + 2); issue(A0, S + 2, c, kt + 2); }
        read_frags<S + 3, 4>(c, c.rdA, fa);
        if (more2) wait_vmcnt<8>(); else if (more1) wait_vmcnt<2>(); else wait_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        bar();
        quad(acc[1][1], fa, fb1);
        quad(acc[1][0], fa, fb0);
        bar();
    }

    // acc must be zero-initialised by the caller
    static __device__ __forceinline__ void run(const GemmOperands& p, int a_nrows, int m0, int n0, char* smem, Acc& acc) {
        Ctx c;
        setup(c, p, a_nrows, m0, n0, smem);
        const int wr = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8);
        // ---- prologue: k-tile 0 whole, B0 / B1 / A0 of k-tile 1
        issue(B0, 0, c, 0); issue(B1, 1, c, 0); issue(A0, 2, c, 0); issue(A1, 3, c, 0);
        if (c.nt > 1) { issue(B0, 4, c, 1); issue(B1, 5, c, 1); issue(A0, 6, c, 1); wait_vmcnt<8>(); }
        else wait_vmcnt<2>();
        bar();
        if (wr == 1) bar();                               // waves 4-7 run one barrier behind
        Frag<bf16> fa[4][CH], fb0[2][CH], fb1[2][CH];
        for (int kt = 0; kt < c.nt; kt += 2) {
            ktile<0>(c, kt, acc, fa, fb0, fb1);
            if (kt + 1 < c.nt) ktile<1>(c, kt + 1, acc, fa, fb0, fb1);
        }
        if (wr == 0) bar();
        bar();                                            // the ring is dead: callers may reuse smem
    }
};

}  // namespace pk
