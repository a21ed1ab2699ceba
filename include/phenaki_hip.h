/* phenaki_hip.h -- C ABI of libphenaki_hip.so, the MI355X (gfx950) kernels behind the Phenaki hot path.
 *
 * The reference (lucidrains/phenaki-pytorch) has no FFI: its boundary is the Python nn.Module surface
 * (CViViT / MaskGit / TokenCritic / Phenaki).  This library is what those modules' forward passes bind
 * in the MI355X build (phenaki_pytorch_amd/_lib.py, ctypes); every entry point names the reference
 * expression it replaces (paths relative to /root/reference/phenaki_pytorch/).
 *
 * Conventions
 *   - all pointers are DEVICE pointers owned by the caller; kernels never allocate or free;
 *   - `stream` is a hipStream_t (0 = default stream); every call is asynchronous on it, no hidden syncs;
 *   - return value: 0 on success, negative on error (no exceptions cross this boundary):
 *       PK_EINVAL (-1) bad shape/size/flag, PK_EALIGN (-2) pointer/stride alignment, PK_ELAUNCH (-3) HIP launch error;
 *   - `dtype`: 0 = exact f32 (f32 MFMA, bit-for-bit an fmaf chain), 1 = bf16 MFMA inputs with f32 accumulation.
 *     "T" below means float for dtype 0 and bf16 (uint16 storage, round-to-nearest-even) for dtype 1;
 *     2 = split-bf16 ("bf16x3", pk_gemm[_ex] / pk_attn_prep / pk_attn_fwd / pk_vocab_sample / pk_vocab_ce): every product is
 *     accumulated as hi.hi + hi.lo + lo.hi on the bf16 matrix cores with x = hi + lo, hi = bf16(x), lo = bf16(x - hi)
 *     (~1e-5 per product; held to the f32 tolerances).  Activations stay f32 (T = float, a_is_f32 / out_is_f32 = 1);
 *     W [N][ldw] is the PRE-SPLIT image of the zero-padded f32 weight: per row and per block of 32 k-elements 128 bytes =
 *     [hi x 32 | lo x 32] bf16 (ldw counted in 4-byte units, a multiple of 32; _lib.split_planes); the attention operand
 *     images Qp / Kp / Vt use the same blocked (hi | lo) format per row (same sizes as dtype 0, 128-byte aligned bases).
 *     LDS-DMA main loops only; LayerNorm fold (ln_s / ln_t), row statistics (stats_out / ln_stats) and dup_rows work as for dtype 1
 *     (round 4; the rows ARE f32, so no C2 copy exists or is needed);
 *   - activations in HBM are f32 unless a parameter says T; rows are row-major with an explicit leading
 *     dimension (ld*, in elements);
 *   - dim_head is fixed at 64 in the attention kernels.
 */
#ifndef PHENAKI_HIP_H
#define PHENAKI_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PK_OK 0
#define PK_EINVAL (-1)
#define PK_EALIGN (-2)
#define PK_ELAUNCH (-3)

/* C = act(A @ W^T + bias) (+ res).  Replaces every nn.Linear on the path: attention.py:50-52 (FeedForward,
 * act 1 = GEGLU on interleaved (value, gate) column pairs -> C is [M][N/2]), attention.py:117-119 (to_q/to_kv/to_out),
 * attention.py:243-252 (CPB MLP, act 2 = LeakyReLU(0.1); act 3 = ReLU: the VGG16 classifier, cvivit.py:349-352), cvivit.py:276,283 (patch embed), cvivit.py:328,333
 * (to_pixels), phenaki_pytorch.py:147 (to_logits).
 * A [M][lda] is f32 (a_is_f32) or T; W [N][ldw] is T; bias [N] f32 or NULL; res [M][ldr] f32 or NULL;
 * C is f32 (out_is_f32) or T; a_rows (or NULL) gathers A rows: logical row m reads A[a_rows[m]].
 * act 1 (GEGLU) with a residual is refused (PK_EINVAL): the pair is stored before the residual add, and no call site wants the fusion. */
int pk_gemm(int dtype, int a_is_f32, const void* A, int lda, const void* W, int ldw, int M, int N, int K,
            const float* bias, const float* res, int ldr, void* C, int ldc, int out_is_f32, int act,
            const int* a_rows, void* stream);

/* pk_gemm with an explicit main-loop variant (0 = automatic; 1/2 = register-staged 64x64 / 128x128 tiles; 8, 9, 24, 27, 33, 3 = the
 * LDS-DMA ring variants that survived the round-1 sweep; 50 (bf16, round 6) = the 256x256 two-group loop of csrc/gemm_p8.hpp, what `automatic` picks for
 * K >= 2048 with >= 512 such tiles; see csrc/gemm.hip) and the number of physical rows behind a gathered A (bounds of the DMA descriptor).
 * The DMA variants need A in T and ldw >= K rounded up to the k-tile (64 bf16 / 32 f32) with zero padding.
 * C2 (bf16 [M][ldc2], or NULL): a second copy of an f32 result for the next GEMM's LDS-DMA operand (dtype 1 only).
 * ln_s / ln_t ([N] f32, or both NULL): the LayerNorm that precedes this nn.Linear in the reference (attention.py:47,142,
 * cvivit.py:277) folded into it -- A holds the UN-normalised rows x, W holds gamma (.) W, and the epilogue applies
 *   LN(x) W^T = rstd * (x (gamma.W)^T - mean * ln_s) + ln_t,  ln_s[n] = sum_k gamma[k] W[n][k],  ln_t[n] = sum_k beta[k] W[n][k]
 * with mean / rstd (biased variance over K, ln_eps inside the sqrt) taken from the A tiles of the main loop; then bias / act / res.
 * row_off [M] / col_off [N] (int32 element offsets, or both NULL): scattered f32 output, element (m, n) -> C[row_off[m] + col_off[n]]
 * with col_off[n + r] = col_off[n] + r inside every aligned group of 4 columns -- the un-patchify 'b t h w (c pt p1 p2) -> b c (t pt)
 * (h p1) (w p2)' of cvivit.py:326-334 is such a map, so to_pixels writes the video in place (no res / C2 / GEGLU with it).
 * stats_out [M][ceil(N/32)][2] f32 (or NULL): every 32-column chunk of every output row also leaves (sum, sum of squares) of its values
 * -- as stored in C2 when given, else in C -- for the LayerNorm-folded GEMM that reads those rows next; that GEMM passes the buffer as
 * ln_stats [M][ceil(K/32)][2] beside ln_s / ln_t and takes mean / rstd from it instead of from its own main loop (LDS-DMA variants
 * 8 / 24 / 33 / f32 3 only; partials are added in index order, so results do not depend on scheduling).
 * dup_rows (0, or >= M): every output row m of C (and C2) is also written at row m + dup_rows -- the to_out GEMM of the first
 * self-attention block of a classifier-free-guidance batch writes the cond and the null copy of the residual stream at once
 * (phenaki_pytorch.py:149-161: both forwards see the same ids; they differ from the first cross-attention on). */
int pk_gemm_ex(int dtype, int a_is_f32, const void* A, int lda, const void* W, int ldw, int M, int N, int K,
               const float* bias, const float* res, int ldr, void* C, int ldc, int out_is_f32, int act,
               const int* a_rows, int a_nrows, int variant, void* C2, int ldc2, const float* ln_s, const float* ln_t,
               float ln_eps, const int* row_off, const int* col_off, float* stats_out, const float* ln_stats, int dup_rows,
               void* stream);
/* the variant `0 = automatic` resolves to for a shape (host-only helper; used to label kernels in bench.py) */
int pk_gemm_auto_variant(int dtype, int a_is_f32, int M, int N, int K, int lda, int ldw, int a_nrows);

/* y = LayerNorm(x) * gamma (+ beta), eps inside the sqrt, biased variance.  attention.py:29-36 (gamma-only
 * LayerNorm, beta NULL or the zero buffer), attention.py:47 and cvivit.py:277,284 (nn.LayerNorm).
 * out (T if out_kind == 1 else f32) and/or out2 (f32) receive y; raw (T, optional) receives x itself (the
 * un-normalised K/V source of attention.py:140-144).  OUTPUT rows may be remapped: grp > 0:
 * r -> (r / grp) * gstride + goff + r % grp  (the first-frame / rest-frames concat of cvivit.py:549); pb > 0: rows
 * seen as (a, b, c), b < pb, c < pc, land at (a, c, b) ('b t (h w) <-> b (h w) t', cvivit.py:468,472,488,496). */
int pk_layernorm(const float* x, int ldx, const float* gamma, const float* beta, float eps, void* out, int ldo,
                 int out_kind, float* out2, int ldo2, void* raw, int ldraw, int M, int D, int grp, int gstride,
                 int goff, int pb, int pc, void* stream);

/* cvivit.py:273-285: Rearrange 'b c (t pt) (h p1) (w p2) -> b t h w (c pt p1 p2)' of frames [f0, f0 + nt*pt) of the
 * (B,C,F,H,W) f32 video, fused with nn.LayerNorm(P), P = C*pt*ph*pw; out[(b,t,h,w)][P] is T (out_kind 1) or f32.
 * weight = bias = NULL: the rearranged rows themselves (no LayerNorm). */
int pk_patchify_ln(const float* video, int B, int C, int F, int H, int W, int f0, int nt, int pt, int ph, int pw,
                   const float* weight, const float* bias, float eps, void* out, int ldo, int out_kind, void* stream);

/* cvivit.py:273-285 up to the Linear, bf16 operands, ONE launch for both frame groups (SURVEY.md 2a "K1"): the patch rows are
 * gathered from the (B,C,F,H,W) f32 video inside the GEMM's A-tile producer (no patch matrix in HBM) and nn.LayerNorm(P) is folded in:
 *   out_g[(b,tt,hh,ww)][n] = rstd * (sum_k bf16(x_k - c) * W_g[n][k] - mean' * s_g[n]) + t_g[n]
 * with c a per-patch centre (below), mean' / rstd the f32 statistics of x - c over the P = C*pt*ph*pw patch features (biased variance,
 * eps inside the sqrt), W_g [N][ldw_g] bf16 = gamma (.) W zero-padded along K to 64, s_g[n] = sum_k W_g[n][k], t_g[n] = sum_k beta[k]
 * W[n][k] + bias[n].  Group g covers frames [f0_g, f0_g + nt_g*pt_g) with pt_g frames per patch (ngroups = 1: group 0 only; pass the
 * long-K group first).  pw a power of two in 8..128, P % 192 == 0, video < 4 GiB;
 * c = the mean of the patch's first 32 features.  The caller applies the nn.LayerNorm(dim) that follows. */
int pk_patch_embed(const float* video, int B, int C, int F, int H, int W, int ph, int pw, int N, float eps, int ngroups,
                   const void* W0, int ldw0, const float* s0, const float* t0, float* out0, int f00, int nt0, int pt0,
                   const void* W1, int ldw1, const float* s1, const float* t1, float* out1, int f01, int nt1, int pt1,
                   int ldo, void* stream);

/* The same product as ROW PANELS x ALL COLUMNS x K-SLICES (round 4; cvivit.py:273-285): a workgroup owns 128 patch rows, all N <= 512 output
 * columns and one K-slice of 1024 features -- the f32 video is read exactly once, 204 workgroups at B = 8.  pk_patch_embed_splitk writes, per
 * group, the raw partial products part_g [slices_g][rows_g][N] f32 (sum_k bf16(x_k - c) W_g[n][k] over the slice) and the partial row statistics
 * stats_g [slices_g][rows_g][2] f32 (sum, sum of squares of x - c); slices_g = pk_patch_embed_slices(C*pt_g*ph*pw).  pk_patch_embed_finish adds
 * the slices in index order, applies the folded nn.LayerNorm(P) (s, t = W beta + bias, eps1, K = P) AND the nn.LayerNorm(N) that follows
 * (gamma2, beta2, eps2), writing the token rows: out2 f32 and / or out bf16, row r -> (r / remap_in) * remap_out + remap_off + r % remap_in. */
int pk_patch_embed_slices(int K);
int pk_patch_embed_splitk(const float* video, int B, int C, int F, int H, int W, int ph, int pw, int N, int ngroups,
                          const void* W0, int ldw0, float* part0, float* stats0, int f00, int nt0, int pt0,
                          const void* W1, int ldw1, float* part1, float* stats1, int f01, int nt1, int pt1, void* stream);
int pk_patch_embed_finish(const float* part, const float* stats, int nslices, int rows, int N, int K, const float* s, const float* t,
                          float eps1, const float* gamma2, const float* beta2, float eps2, float* out2, int ldo2, void* out, int ldo,
                          int remap_in, int remap_out, int remap_off, void* stream);
/* pk_patch_embed_finish for BOTH frame groups in one launch (round 5): g[0 .. ngroups) carry the per-group fields above, every group writes the same
 * out2 / out token buffers through its own row remap. */
typedef struct {
    const float* part; const float* stats; int nslices, rows, K;
    const float* s; const float* t; float eps1;
    const float* gamma2; const float* beta2; float eps2;
    int remap_in, remap_out, remap_off;
} pk_patch_finish_group;
int pk_patch_embed_finish_groups(const pk_patch_finish_group* g, int ngroups, int N, float* out2, int ldo2, void* out, int ldo, void* stream);


/* cvivit.py:326-334: Rearrange 'b t h w (c pt p1 p2) -> b c (t pt) (h p1) (w p2)' into frames [f0, f0 + nt*pt). */
int pk_unpatchify(const float* pix, int ldp, float* video, int B, int C, int F, int H, int W, int f0, int nt,
                  int pt, int ph, int pw, void* stream);

/* cvivit.py:585-589 in patch layout: dst[(b,tt,hh,ww)][(c,dt,y,x)] = fmask[b][f0 + tt*pt + dt] ? src[..] : 0 for a (rows, P) f32 matrix
 * (fmask (B, F) uint8; dst may be src): the frame mask of variable-length training where the training step takes its loss (train_cvivit.py). */
int pk_patch_frame_mask(const float* src, long long lds, float* dst, long long ldd, const unsigned char* fmask, int B, int C, int F, int H, int W,
                        int f0, int nt, int pt, int ph, int pw, void* stream);

/* Numerator of the reconstruction loss of cvivit.py:585-591 (F.mse_loss(video, recon), optionally over the frames a
 * (B, F) mask keeps): partials[i], i < PK_SQDIFF_BLOCKS, are per-workgroup double sums of (a - b)^2 over two contiguous
 * (B, C, F, H, W) f32 videos; the caller adds them and divides by the kept element count. */
#define PK_SQDIFF_BLOCKS 1024
int pk_sqdiff_partials(const float* a, const float* b, const unsigned char* fmask, int B, int C, int F, int H, int W,
                       double* partials, void* stream);

/* attention.py:57-85 + residual of attention.py:323: out = x + bias + depthwise_conv3d_3x3x3(zero-padded x) on the
 * channels-last (B,T,H,W,D) reinterpretation of the token buffer; time pad (2,0) if causal else (1,1).
 * wt is dsconv.weight (D,1,3,3,3) pre-transposed to [27][D].  Not in-place. */
int pk_peg(const float* x, const float* wt, const float* bias, float* out, void* out_t, int B, int T, int H, int W, int D,
           int causal, void* stream);       /* out_t: optional bf16 copy of out (the next GEMM's operand) */

/* LFQ (vector-quantize-pytorch, un-vendored; call sites cvivit.py:570 and :439; restated in oracle/lfq.py).
 * encode: proj = x @ Wp^T + bp (f32), ids = sum_k (proj_k > 0) << (cd-1-k); proj (M x cd) optional output.
 * decode: out = (bit ? +1 : -1) @ Wo^T + bo,  Wo is [D][cd].  ids_prime (or NULL): row (b, i) of the M = nb * (n_prime + n) rows takes
 *   its id from ids_prime[b][i] for i < n_prime and ids[b][i - n_prime] otherwise (phenaki_pytorch.py:535-536: the primed tokens are
 *   prepended before decoding -- no concatenated copy); pb, pc > 0: row (a, b, c) is written at (a, c, b), the '(b h w) t' order
 *   the decoder's temporal transformer reads (cvivit.py:482), pb = pc = 0: identity. */
int pk_lfq_encode(const float* x, int ldx, const float* wp, const float* bp, long long* ids, float* proj,
                  int M, int D, int cd, void* stream);
int pk_lfq_decode(const long long* ids, const float* wo, const float* bo, float* out, int M, int D, int cd,
                  const long long* ids_prime, int n_prime, int n, int pb, int pc, void* stream);

/* LFQ training-mode auxiliary loss (third return of `self.vq(tokens)`, cvivit.py:570, added to the GAN generator objective at cvivit.py:666;
 * the published vector-quantize-pytorch LFQ.forward, restated in oracle/lfq.py):
 *   aux = w_e (mean_i H(prob_i) - gamma H(mean_i prob_i)) + w_c mean (z - sign(z) scale)^2,  prob_i = softmax over the 2^cd sign codes of
 *   2 T <z_i, code>,  H(p) = sum -p log(max(p, 1e-5)),  z = proj (M, cd) = project_in(x).
 * The (M, 2^cd) probability matrix is never formed: prob_i(u, v) = a_i[u] b_i[v] over the high / low halves of the bits (hi = ceil(cd / 2),
 * lo = cd / 2; code index = sum_k bit_k 2^(cd-1-k), MSB first as the module's `mask`; alpha = 4 T scale; 2 <= cd <= 16).
 *   pk_lfq_aux_prep:     A (M, 2^hi), B (M, 2^lo) factor rows; ent[i] = H(prob_i); commit[i] = sum_k (z_ik - sign(z_ik) scale)^2
 *   (host: Q = A^T B by pk_bmm = M times the batch distribution)
 *   pk_lfq_aux_codebook: hc_part[pk_lfq_aux_parts(cd)] = partial sums of H(Q inv_n); G = coef * dH/dq at q = Q inv_n  (2^hi x 2^lo)
 *   (host: GA = B G^T, GB = A G by pk_bmm)
 *   pk_lfq_aux_grad:     dproj (M, cd) = d aux / d z  with wen = w_e / M, wc2 = 2 w_c / (M cd), coef above = -w_e gamma / M
 *   pk_lfq_aux_finish:   out[0] = aux, out[1] = mean_i H(prob_i), out[2] = H(batch distribution), out[3] = commitment (fixed summation order). */
int pk_lfq_aux_parts(int cd);
int pk_lfq_aux_prep(const float* proj, int M, int cd, float alpha, float scale, float* A, float* B, float* ent, float* commit, void* stream);
int pk_lfq_aux_codebook(const float* Q, int cd, float inv_n, float coef, float* G, float* hc_part, void* stream);
int pk_lfq_aux_grad(const float* proj, const float* GA, const float* GB, int M, int cd, float alpha, float scale, float wen, float wc2,
                    float* dproj, void* stream);
int pk_lfq_aux_finish(const float* ent, const float* commit, int M, const float* hc_part, int cd, float w_e, float gamma, float w_c, float* out,
                      void* stream);

/* Training step of the cosine-sim VectorQuantize (constructed at cvivit.py:321, called at cvivit.py:568-570; the un-vendored vector-quantize-pytorch
 * module in training mode, semantics restated in DESIGN.md "VectorQuantize training"): straight-through output q = E[ids], commitment loss
 * w mean_kept (q - x)^2, EMA update of cluster_size / embed_avg / embed from the kept rows.  x, xn = l2norm(x), y, dy, dx are contiguous (M, D) f32,
 * E / embed_avg / embed contiguous (V, D) f32, D % 4 == 0 and D <= 1024, 16-byte aligned bases; ids (M,) int64; keep (M,) bytes, NULL = every row kept.
 * Every kernel tests 0 <= id < V on the device and treats a row with another id as dropped (it is never used as an index).
 *   pk_vq_hist:            counts[c] (V int32, ZEROED by the caller) += #{kept r : ids[r] = c} (integer atomics: order-independent).  check_ids != 0:
 *                          the ids are first copied to the host (synchronises the stream) and an id outside [0, V) is PK_EINVAL with nothing launched.
 *   pk_vq_scan:            offsets = cursor = exclusive scan of counts; cluster_size = decay cluster_size + (1 - decay) counts in place;
 *                          S[0] = sum_c cluster_size[c] in a fixed order (one workgroup, no host read).
 *   pk_vq_fill:            rows[atomicAdd(cursor[id], 1)] = r for every kept row: code c's rows are rows[offsets[c] .. + counts[c]), in any order.
 *   pk_vq_codebook_update: per code c, sum[c] = sum of xn[r] over its rows in ASCENDING r (bit-reproducible), embed_avg[c] = decay embed_avg[c] +
 *                          (1 - decay) sum[c], embed[c] = l2norm(embed_avg[c] / ((cluster_size[c] + eps) / (S + V eps) S)) (l2norm eps 1e-12); in place.
 *   pk_vq_gather_commit:   y[r] = E[ids[r]]; rowsq[r] = sum_d (y - x)^2 for kept rows, 0 for dropped ones (summed by pk_colsum).
 *   pk_vq_commit_bwd:      dx = dy + coef * coef_dev[0] (coef_dev NULL: 1) * keep[r] * (x[r] - q[r]), q = the y of pk_vq_gather_commit (the codebook
 *                          itself has been updated in place by the time the backward pass runs, so the gather is not repeated from it). */
int pk_vq_hist(const long long* ids, const unsigned char* keep, int M, int V, int* counts, int check_ids, void* stream);
int pk_vq_scan(const int* counts, int V, float decay, float* cluster_size, int* offsets, int* cursor, float* S, void* stream);
int pk_vq_fill(const long long* ids, const unsigned char* keep, int M, int V, int* cursor, int* rows, void* stream);
int pk_vq_codebook_update(const float* xn, const int* counts, const int* offsets, const int* rows, const float* cluster_size, const float* S,
                          int M, int V, int D, float decay, float eps, float* embed_avg, float* embed, void* stream);
int pk_vq_gather_commit(const float* x, const float* E, const long long* ids, const unsigned char* keep, int M, int V, int D, float* y,
                        float* rowsq, void* stream);
int pk_vq_commit_bwd(const float* dy, const float* x, const float* q, const unsigned char* keep, int M, int D, float coef, const float* coef_dev,
                     float* dx, void* stream);

/* Upkeep of the same codebook (the published module's threshold_ema_dead_code and kmeans_init; semantics restated in DESIGN.md "VectorQuantize
 * upkeep", parity unpinned).  A row is chosen as pick(b, j, n) = ((b mod n) + j P) mod n, P = 2^31 - 1, in 64-bit integers, among the n kept rows
 * in ascending order: kept / n_keep are the list and its length ON THE DEVICE (pk_vq_compact_keep), both NULL = every row kept (n = M).  b >= 0
 * is a host integer.  Every index made from device data (jrank, n_keep, kept[]) is range-tested before use; a failed test leaves the EMA result.
 *   pk_vq_compact_keep:           kept[0 .. n) = the rows with keep[r] != 0, ascending (M int32); n_keep[0] = n.  One workgroup.
 *   pk_vq_scan_expire:            pk_vq_scan, and jrank[c] (V int32) = #{c' < c : cluster_size[c'] < threshold} where the post-EMA
 *                                 cluster_size[c] < threshold (strict), -1 elsewhere.  S and cluster_size are exactly pk_vq_scan's.
 *   pk_vq_codebook_update_expire: pk_vq_codebook_update, except that a code with jrank[c] = j >= 0 gets embed[c] = xn[r] (bit for bit),
 *                                 embed_avg[c] = reset * xn[r], cluster_size[c] = reset, r = the j-th chosen row.
 *   pk_vq_pick_rows:              out[c] = xn[the c-th chosen row], c < V (the k-means seeds; the published module samples them).
 *   pk_vq_kmeans_means:           one k-means mean update after hist / scan / fill on the assignment: means[c] = l2norm(sum of xn over code c's
 *                                 rows, ascending) where counts[c] > 0, untouched elsewhere.  embed_avg / cluster_size non-NULL (both or neither):
 *                                 also embed_avg[c] = means[c] * counts[c], cluster_size[c] = counts[c] (the initialised state). */
int pk_vq_compact_keep(const unsigned char* keep, int M, int* kept, int* n_keep, void* stream);
int pk_vq_scan_expire(const int* counts, int V, float decay, float threshold, float* cluster_size, int* offsets, int* cursor, float* S, int* jrank,
                      void* stream);
int pk_vq_codebook_update_expire(const float* xn, const int* counts, const int* offsets, const int* rows, float* cluster_size, const float* S,
                                 const int* jrank, const int* kept, const int* n_keep, int M, int V, int D, float decay, float eps, float reset,
                                 long long b, float* embed_avg, float* embed, void* stream);
int pk_vq_pick_rows(const float* xn, const int* kept, const int* n_keep, int M, int V, int D, long long b, float* out, void* stream);
int pk_vq_kmeans_means(const float* xn, const int* counts, const int* offsets, const int* rows, int M, int V, int D, float* means, float* embed_avg,
                       float* cluster_size, void* stream);

/* Text-encoder support (reference t5.py:64-103 calls HuggingFace T5EncoderModel; the T5 v1.1 encoder layers are built
 * from pk_gemm, pk_attn_prep with q_scale = k_scale = NULL (plain dot-product attention: no l2norm, q * scale), pk_attn_fwd and these two):
 * pk_rmsnorm: T5LayerNorm, y = x * rsqrt(mean(x^2) + eps) * w (f32 statistics, no mean subtraction, no bias); rows with rowmask[row] == 0
 *   (or NULL: none) are written as zeros (the masked_fill of t5.py:97-100); out is T (out_kind 1) or f32.
 * pk_gated_gelu_tanh: out[m][f] = gelu_new(h[m][f]) * h[m][F + f] for h (M, >= 2F) f32 -- T5DenseGatedActDense's activation on the output
 *   of one GEMM against [wi_0 ; wi_1]. */
int pk_rmsnorm(const float* x, int ldx, const float* w, float eps, const unsigned char* rowmask, void* out, int ldo, int out_kind,
               int M, int D, void* stream);
int pk_gated_gelu_tanh(const float* h, int ldh, void* out, int ldo, int out_kind, int M, int F, void* stream);

/* cvivit.py:472 (the encoder's final norm_out) fused with the LFQ of cvivit.py:570: ids[orow] = LFQ(LayerNorm(x[row]) * gamma
 * (+ beta)) in one pass over x, cd <= 16; orow = the (a, b, c) -> (a, c, b) row permutation of pk_layernorm (pb = 0: identity).
 * tokens (f32 [M][ldt], or NULL) receives the normalised rows, proj ([M][cd], or NULL) the pre-sign projections. */
int pk_layernorm_lfq(const float* x, int ldx, const float* gamma, const float* beta, float eps, const float* wp,
                     const float* bp, long long* ids, float* tokens, int ldt, float* proj, int M, int D, int cd,
                     int pb, int pc, void* stream);

/* rows of x scaled to unit l2 norm (F.normalize, eps 1e-12), out in T (out_kind 1) or f32: the query side of the cosine-sim
 * VectorQuantize lookup (cvivit.py:321).  x 16-byte aligned, out 16-byte (f32) / 8-byte (T) aligned, else PK_EALIGN. */
int pk_l2norm_rows(const float* x, int ldx, void* out, int ldo, int out_kind, int M, int D, void* stream);

/* phenaki_pytorch.py:194-197, 290-291 (+ the prime-token concat of :500): S sequences of n_tot = n_prime + n positions,
 * out[s*n_tot + i] = token_emb[id] + pos_emb[i] with id = ids_prime[b][i] for i < n_prime (NULL if n_prime == 0), else
 * ids[b][i - n_prime], b = s % nb -- the cond and null replicas of a classifier-free-guidance batch (S = 2 nb) share ids. */
int pk_embed(const long long* ids_prime, int n_prime, const long long* ids, int n, int nb, const float* tok,
             const float* pos, float* out, void* out_t, int S, int D, void* stream);       /* out_t: optional bf16 copy */

/* attention.py:257-272 first CPB layer: out[(i,j)][D] = leaky_relu(W0 @ (sign(rel) log(|rel|+1)) + b0, 0.1) over the
 * flattened (d0,d1,d2) grid; nd = 2 uses (d1,d2) with d0 = 1. */
int pk_cpb_input(const float* w0, const float* b0, float* out, int d0, int d1, int d2, int nd, int D, void* stream);

/* attention.py:146-157: head split, null-kv prepend, l2norm (k after the concat), q/k scales, sim scale folded in q;
 * writes Qp [S][h][nq_pad][dh], Kp [S][h][nk_pad][dh], Vt [S][h][dh][nk_pad] in T (dh = dim_head; 64 for pk_attn_prep), i.e.
 * S*h*nq_pad*dh and twice S*h*nk_pad*dh elements. pk_attn_pads gives the pads (they do not depend on dim_head).
 * kv == NULL prepares the query side only (cross-attention K/V cached across sampling steps).
 * pk_attn_prep_dh: the same for dim_head = 32 | 64 | 128 (any other width: PK_EINVAL); q / kv hold h heads of dim_head columns, null_kv is
 * [h][2*nnull][dim_head], q_scale / k_scale [dim_head].  dtype 2 images keep their 128-byte blocks of 32 elements (a row is dim_head / 32
 * blocks), the bases sit on a 128-byte boundary.  pk_attn_prep is pk_attn_prep_dh(64, ...). */
int pk_attn_pads(int nq, int n_kv, int nnull, int* nq_pad, int* nk_pad);
int pk_attn_prep(int dtype, const float* q, int ldq, const float* kv, int ldkv, const float* null_kv,
                 const float* q_scale, const float* k_scale, float scale, void* Qp, void* Kp, void* Vt,
                 int S, int h, int nq, int n_kv, int nnull, void* stream);
int pk_attn_prep_dh(int dim_head, int dtype, const float* q, int ldq, const float* kv, int ldkv, const float* null_kv,
                    const float* q_scale, const float* k_scale, float scale, void* Qp, void* Kp, void* Vt,
                    int S, int h, int nq, int n_kv, int nnull, void* stream);

/* attention.py:142-157 in ONE launch (dtype 1 = bf16: bf16 rows / weights / images; dtype 2 = split-bf16, round 4: f32 rows split in
 * registers, host-split weight planes as for pk_gemm, images written pre-split as for pk_attn_prep(dtype 2)): to_q (A = xq = LayerNorm(x)) and to_kv (A = xkv = the un-normalised x, or NULL
 * for the query side only) as one MFMA GEMM whose epilogue does the head split, l2norm, q/k scales (sim scale folded in
 * q) and the V transpose, writing Qp / Kp / Vt (layouts above) directly: the f32 q / kv matrices never reach HBM and
 * pk_attn_prep is not needed.  Self-attention only on the kv side (no null keys); M = S * nseq rows. */
int pk_qkv_project(int dtype, const void* xq, const void* xkv, int ld, const void* wq, const void* wkv, int ldw, int S, int nseq,
                   int h, int K, const float* q_scale, const float* k_scale, float scale, void* Qp, void* Kp, void* Vt,
                   int nq_pad, int nk_pad, const float* q_ln_s, void* stream);
/* q_ln_s ([h*64] f32, or NULL): the attention's LayerNorm folded into to_q -- xq then holds the un-normalised rows (= xkv), wq holds
 * gamma (.) Wq and q_ln_s its row sums; q = l2norm(x (gamma.Wq)^T - mean(x) q_ln_s) (the l2norm cancels the LayerNorm's rstd). */

/* attention.py:142-182 for SHORT self-attention sequences (n <= 64, no null keys, no key mask; dtype 1 bf16 / 2 split-bf16) in ONE launch: the
 * to_q / to_kv projections, l2norm + scales, and softmax(q k^T + bias (+ ALiBi, causal)) v -- what pk_qkv_project + pk_attn_fwd
 * compute, without Qp / Kp / Vt ever reaching HBM.  A workgroup owns one head of floor(64 / n) whole sequences.  xq = LayerNorm(x)
 * rows, xkv = x rows (both [S*n][ld], bf16 / f32 by dtype); bias [h][n][n] f32 or NULL; slopes [h] with causal; O [S*n][ldo] (bf16 / f32),
 * heads merged.  dtype 2 stages q^ / k^ / v^T as (hi, lo) bf16 planes in LDS and computes every product as three MFMAs. */
int pk_qkv_attn(int dtype, const void* xq, const void* xkv, int ld, const void* wq, const void* wkv, int ldw, int S, int n, int h, int K,
                const float* q_scale, const float* k_scale, float scale, const float* bias, long bias_hstride, int bias_ld,
                const float* slopes, int causal, void* O, int ldo, const float* q_ln_s, void* stream);

/* Cross-attention against CACHED key / value images (the step-invariant text context, attention.py:142-182 with context) in ONE launch:
 * to_q (+ the folded LayerNorm, q_ln_s as in pk_qkv_project) + l2norm + softmax(q k^T (+ key mask)) v.  Kp / Vt are the images
 * pk_attn_prep wrote (same dtype) for nnull + n_kv <= 64 keys (nk_pad from pk_attn_pads); n % 64 == 0; kmask [S][n_kv] uint8 or NULL;
 * O bf16 (dtype 1) / f32 (dtype 2).  Kp / Vt are S * h * nk_pad * 64 elements each.  PRECONDITION: the Vt columns of the pad keys
 * nnull + n_kv .. nk_pad - 1 hold finite values (pk_attn_prep zero-fills them; pk_qkv_project does NOT write them): the kernel gives
 * them the weight 0 and 0 * NaN is NaN.  The pad rows of Kp may hold anything. */
int pk_q_attn_cached(int dtype, const void* xq, int ld, const void* wq, int ldw, int S, int n, int h, int K, const float* q_scale, float scale,
                     const float* q_ln_s, const void* Kp, const void* Vt, int nk_pad, int n_kv, int nnull,
                     const unsigned char* kmask, void* O, int ldo, void* stream);

/* attention.py:157-182: softmax(sim + bias (+ key mask, + ALiBi, causal)) @ v, heads merged: O[(s,i)][hh*dh + d] (dh = 64 for pk_attn_fwd).
 * bias[hh][i][j] is over the real (non-null) keys; kmask [S][n_kv] uint8 (1 = keep); slopes [h] with causal.
 * pk_attn_fwd_dh / pk_attn_fwd_lse_dh: the same on the images of pk_attn_prep_dh(dim_head, ...), dim_head = 32 | 64 | 128 (else PK_EINVAL).
 * 64 is pk_attn_fwd / pk_attn_fwd_lse.  32 and 128 always run on the LDS-free kernel: bias_tab, a finite score_bound or a dropout site
 * is PK_EINVAL there (the LDS-staged kernels, the fused projection kernels and the backward kernels are built for 64).
 * dtype 0 and 2 write O as f32: out_is_f32 = 0 is PK_EINVAL with them. */
int pk_attn_fwd(int dtype, const void* Qp, const void* Kp, const void* Vt, const float* bias, long bias_hstride,
                int bias_ld, const unsigned char* kmask, const float* slopes, int causal, void* O, int ldo,
                int out_is_f32, int S, int h, int nq, int n_kv, int nnull, const float* bias_tab, int tab_len,
                const int* pos_code, int code_off, int tab_run4, float score_bound, void* stream);
int pk_attn_fwd_dh(int dim_head, int dtype, const void* Qp, const void* Kp, const void* Vt, const float* bias, long bias_hstride,
                   int bias_ld, const unsigned char* kmask, const float* slopes, int causal, void* O, int ldo,
                   int out_is_f32, int S, int h, int nq, int n_kv, int nnull, const float* bias_tab, int tab_len,
                   const int* pos_code, int code_off, int tab_run4, float score_bound, void* stream);
/* a dropout site of the training kernels (the dropout paragraph further down): stream (seed, offset), keep_thr in [1, 256], scale = 1 / (1 - keep_thr / 256).
 * Every entry point that takes one takes NULL for no dropout. */
typedef struct pk_dropout { unsigned long long seed, offset; int keep_thr; float scale; } pk_dropout;
/* The training forward (attention.py:157-182 under autograd): the same product, and lse[(s h + hh) nq + i] = log sum_j exp(score row i) for the
 * backward kernels (pk_attn_bwd_ws with bit 1 of its flag word set skips the pass that recomputed it).  LDS-free kernel; no bias table / score bound.
 * drop = attn_dropout (attention.py:177): the softmax statistics and lse are those of the undropped probabilities, the P that multiplies V is masked
 * by the keep function of (seed, offset) and O is scaled by `scale`.  With a site every shape runs on the LDS-free kernel (the LDS-staged forms serve
 * p = 0 only) and S h nq <= 2^32 - 1.  pk_attn_bwd_ws with the same site is its backward. */
int pk_attn_fwd_lse(int dtype, const void* Qp, const void* Kp, const void* Vt, const float* bias, long bias_hstride,
                    int bias_ld, const unsigned char* kmask, const float* slopes, int causal, void* O, int ldo,
                    int out_is_f32, int S, int h, int nq, int n_kv, int nnull, float* lse, const pk_dropout* drop, void* stream);
int pk_attn_fwd_lse_dh(int dim_head, int dtype, const void* Qp, const void* Kp, const void* Vt, const float* bias, long bias_hstride,
                       int bias_ld, const unsigned char* kmask, const float* slopes, int causal, void* O, int ldo,
                       int out_is_f32, int S, int h, int nq, int n_kv, int nnull, float* lse, const pk_dropout* drop, void* stream);
/* score_bound: an upper bound of sim + bias over every (head, query, key), or NaN.  q^ and k^ are unit vectors times q_scale / k_scale,
 * so |sim| <= scale * max_d |q_scale_d k_scale_d| and the caller knows the maximum of its bias: with a finite bound (and no key
 * mask, not causal, bf16, >= 64 queries and keys) the softmax numerators are p = 2^(s log2(e) - ceil(bound log2(e))) -- no running
 * maximum, no cross-lane max, no accumulator rescale per key tile (the same softmax: it is shift-invariant; an integer shift of
 * the exponent keeps every mantissa, hence the bf16 rounding of p, independent of the tiling).  NaN: running-max flash loop.
 * tab_run4: 1 when pos_code[4k + r] == pos_code[4k] + r for every k (last grid dimension a multiple of 4): the kernel then fetches the
 * 4 table entries of 4 consecutive keys with two 8-byte LDS reads.
 * bias_tab ([h][tab_len] f32, or NULL; then bias must be NULL): the relative-position form of the continuous position bias
 * (attention.py:229-275), bias[hh][i][j] = bias_tab[hh][pos_code[i] - pos_code[j] + code_off] with pos_code [n] int32 -- staged
 * in LDS by the bf16 kernel for nq = n_kv >= 64 (self-attention, no null keys / mask / causal); other shapes: PK_EINVAL. */

/* attention.py:128-182 for short self-attention sequences (n <= 64, no null keys: the C-ViViT spatial / temporal layers)
 * straight from the projection outputs q [S*n][ldq], kv [S*n][ldkv]: one launch instead of pk_attn_prep + pk_attn_fwd;
 * f32 arithmetic in both precision modes; O f32 (out_kind 0) or bf16 (1). */
int pk_attn_small(const float* q, int ldq, const float* kv, int ldkv, const float* q_scale, const float* k_scale,
                  float scale, const float* bias, long bias_hstride, int bias_ld, const unsigned char* kmask,
                  const float* slopes, int causal, void* O, int ldo, int out_kind, int S, int h, int n, void* stream);

/* phenaki_pytorch.py:155-161 applied to the trunk outputs: e = null + (cond - null) * scale for the non-prime
 * positions; x rows are [cond sequences | null sequences] of n_tot tokens; rows (or NULL) selects output rows
 * (flat b * (n_tot - n_prime) + i). */
int pk_cfg_mix(const float* x, int ldx, int nb, int n_tot, int n_prime, const int* rows, int nrows, float scale,
               int has_null, void* out, int ldo, int out_is_f32, int D, void* stream);
/* pk_cfg_mix for P conditional branches and a base branch (phenaki_pytorch.py:149-161 generalised: negative prompts, prompt blends,
 * per-sample guidance scales).  x holds (P + has_base) * nb sequences laid out [cond_0 | .. | cond_{P-1} | base], the order of pk_cfg_mix's
 * [cond | null].  coef: device f32 [(P + 1) * nb], the table row of the current step: rows 0..P-1 hold the blend weights a[k][b], row P the
 * guidance scale g[b].  Per sample b:
 *     cbar = e_0 (P == 1: no multiply)  |  sum_k a[k][b] e_k, k ascending (P > 1);      out = e_base + (cbar - e_base) * g[b]
 * has_base == 0 writes cbar alone (a blend at scale 1; row P of coef is not read).  rows / nrows / n_prime / out_is_f32 / the 16-byte
 * accesses are pk_cfg_mix's; the mix is its f32 expression: P == 1 is bit-identical to pk_cfg_mix at equal scales.
 * PK_EINVAL before any launch: P outside 1..3, coef == NULL, D % 4 != 0, has_base == 0 with P == 1. */
int pk_guidance_mix(const float* x, int ldx, int nb, int n_tot, int n_prime, const int* rows, int nrows, const float* coef, int P,
                    int has_base, void* out, int ldo, int out_is_f32, int D, void* stream);

/* phenaki_pytorch.py:213 + 88-93 + 506-509 + 547-550, never materialising logits: per row
 * pred = argmax(logits / max(T,1e-10) + gumbel(U)), optional (max, sum exp) for 1 - softmax[pred].
 * U != NULL: PARITY mode, uniform noise read from U[row][V]; U == NULL: counter-hash noise from `seed` (+ *seed_dev when
 * seed_dev != NULL: a device-resident 64-bit word read at run time, so a captured hipGraph replays with fresh noise).
 * need_lse is a flag word: bit 0 = keep the softmax statistics, bit 1 = no noise at all (plain argmax of A @ W^T + bias:
 * the cosine-sim codebook lookup of the VectorQuantize path, cvivit.py:321,568-570).
 * partials: 5 * pk_vocab_ntiles(V) * M 4-byte words of workspace consumed by pk_vocab_reduce, which writes
 * pred[r], ids[r] = where(mask[r], pred, ids[r]) and scores[r] = where(mask[r], 1 - p, -1e4). */
int pk_vocab_ntiles(int V);
int pk_vocab_sample(int dtype, const void* A, int lda, const void* W, int ldw, const float* bias, int M, int V, int D,
                    float temperature, const float* U, const int* rows, unsigned long long seed,
                    const unsigned long long* seed_dev, int need_lse, void* partials, void* stream);
/* PARITY sampling on torch's own device RNG stream (SURVEY.md 7 "phase 2"): the gumbel noise of logical row r, column v is bit for bit
 * what `torch.zeros(rows_total, V, device=...).uniform_(0, 1)[r][v]` holds for a generator at (torch_seed, philox_offset) -- the reference's
 * gumbel_noise(logits), phenaki_pytorch.py:88-93 -- generated in the epilogue (Philox4x32-10 with ATen's element -> (subsequence, counter, word)
 * map, csrc/common.hpp torch_uniform); philox_stride = 256 * min(#CUs * (max threads per CU / 256), ceil(rows_total * V / 256)), the caller
 * advances the generator by 4 * ceil(rows_total * V / (4 * philox_stride)).  A seeded reference run on the same GPU draws the same noise. */
int pk_vocab_sample_philox(int dtype, const void* A, int lda, const void* W, int ldw, const float* bias, int M, int V, int D, float temperature,
                           const int* rows, unsigned long long torch_seed, unsigned long long philox_offset, unsigned int philox_stride,
                           int need_lse, void* partials, void* stream);
int pk_vocab_reduce(const void* partials, int M, int V, const int* rows, const unsigned char* mask, long long* ids,
                    long long* pred, float* scores, int need_lse, void* stream);
/* Top-k filtered sampling on the f32 logits of a row slab (the reference's top_k helper, phenaki_pytorch.py:95-101, in front of
 * gumbel_sample; Phenaki.sample(filter_thres=, top_k=)).  logits [M][ldl] f32 = pk_gemm of the head's operands.  Per row m:
 *     cut  = the k-th largest of logits[m][0..V), counting multiplicity (k == V: -inf, no select);
 *     kept = { v : logits[m][v] >= cut } as floats (-0.0 == +0.0); exact ties at the cut are ALL kept, so |kept| may exceed k
 *            (torch.topk keeps an arbitrary k of them: the one difference);
 *     pred = argmax over kept v of the noisy logit, pk_vocab_sample's expressions: U != NULL reads u from U[lrow][V] (PARITY), else the
 *            counter hash at (seed (+ *seed_dev), lrow * V + v), the draws pk_vocab_sample makes for the same (seed, logical row, column);
 *            T = max(temperature, 1e-10f); the first maximum wins.  lrow = rows ? rows[m] : row_base + m.
 * need_lse is pk_vocab_sample's flag word: bit 0 = also max and sum exp over ALL V columns (the score stays the unfiltered distribution's
 * 1 - softmax[pred]), bit 1 = no noise.  The write-out is pk_vocab_reduce's at r = lrow: pred[r], ids[r] = where(mask[r], pred, ids[r]),
 * scores[r] = where(mask[r], 1 - p, -1e4) (bit 0 only).  cut_out [M] f32 / kept_out [M] int32 (or NULL): the row's cut and kept count.
 * One workgroup of 1024 lanes holds a row in registers; exact MSB-first radix select; fixed-order reductions: two calls agree bit for bit.
 * PK_EINVAL before any launch: k < 1 or k > V; V < 4, V > 65536 or V % 4; ldl < V or ldl % 4; M <= 0; logits or pred NULL; scores without
 * bit 0; rows together with row_base != 0.  PK_EALIGN: logits or U off 16 bytes. */
int pk_logits_topk_sample(const float* logits, long long ldl, int M, int V, int k, float temperature,
                          const float* U, const int* rows, int row_base, unsigned long long seed,
                          const unsigned long long* seed_dev, int need_lse /* bit 0 lse | bit 1 no noise */,
                          const unsigned char* mask, long long* ids, long long* pred, float* scores,
                          float* cut_out, int* kept_out, void* stream);
/* Nucleus (top-p) and min-p filtered sampling on the same logits (Phenaki.sample(top_p=, min_p=)); the reference has neither.  Everything
 * pk_logits_topk_sample says about logits, U, rows, row_base, seed, seed_dev, need_lse, mask, ids, pred, scores and the write-out holds.
 * Per row, l[v] the f32 logit, T = max(temperature, 1e-10f), inv_t = 1.0f / T, lmax the row maximum:
 *     arg[v] = (l[v] - lmax) * inv_t in f32;  w[v] = __expf(arg[v]);  q[v] = (unsigned long long)(w[v] * 2^40), the fixed-point mass
 *              (at most 2^40 per column, at most 2^56 over V <= 65 536 columns).
 * The filters apply in the order temperature, top-k, top-p, min-p and the result is their intersection:
 *     1. top-k: cut_k = the k-th largest logit counting multiplicity, S = { v : l[v] >= cut_k };  k == V: no top-k.
 *     2. top-p: Z_S = sum_{v in S} q[v];  cut_p = the largest row value c such that sum_{v in S, l[v] >= c} q[v] >= top_p * Z_S: the smallest
 *        descending prefix of S that reaches the share top_p of S's own mass.  Exact ties at the cut are all kept.  The product and the
 *        comparison are done in double.  top_p == 1: no nucleus.  The maximum has q = 2^40 > 0: at least one column is kept.
 *     3. min-p: v passes iff arg[v] >= (float)log((double)min_p) (taken on the host side of this entry point): the f32 arg is compared,
 *        not w; arg is non-decreasing in l, so what passes is upward-closed.  min_p == 0: none.
 *     4. kept = S & { l >= cut_p } & { min-p passes } = { v : l[v] >= cut }, cut the smallest kept logit: cut_out[m] (-inf when no filter
 *        is active), kept_out[m] the count.
 *     5. the draw and the score are pk_logits_topk_sample's: pred = argmax over kept v of the noisy logit, first maximum; the score stays
 *        1 - softmax[pred] over ALL V columns at temperature 1.
 * The nucleus is that of softmax(l / T) at the step's annealed temperature, the distribution the gumbel arg-max samples from; at
 * temperature 0 (the clamp) it is the row maximum and its exact ties.
 * The mass is accumulated as 64-bit integers (integer LDS atomics, four 8-bit MSB-first passes over the keys >= cut_k): no float atomics,
 * every reduction in a fixed order, two calls agree bit for bit.  top_p == 1 && min_p == 0 gives pk_logits_topk_sample's bits for the same k.
 * PK_EINVAL before any launch: top_p not in (0, 1] or NaN; min_p not in [0, 1) or NaN; whatever pk_logits_topk_sample refuses.  PK_EALIGN
 * as there.  Finite logits only. */
int pk_logits_nucleus_sample(const float* logits, long long ldl, int M, int V, int k, float top_p, float min_p, float temperature,
                             const float* U, const int* rows, int row_base, unsigned long long seed,
                             const unsigned long long* seed_dev, int need_lse /* bit 0 lse | bit 1 no noise */,
                             const unsigned char* mask, long long* ids, long long* pred, float* scores,
                             float* cut_out, int* kept_out, void* stream);

/* The masked-token cross entropy of phenaki_pytorch.py:640-643 without the logits: after a pk_vocab_sample call with
 * need_lse bit 0 set, loss[m] = logsumexp_v(logits[m][:]) - logits[m][targets[r]] with r = rows ? rows[m] : m, where the
 * target logit is the dot product of row m of A with row targets[r] of W (+ bias) -- same A / W / bias as that call. */
int pk_vocab_ce(int dtype, const void* partials, int M, int V, const void* A, int lda, const void* W, int ldw,
                const float* bias, int D, const long long* targets, const int* rows, float* loss, float* lse_out, void* stream);
/* The regularised form of that loss: label smoothing eps = label_smoothing in [0, 1) (torch's F.cross_entropy(label_smoothing=): eps is spread
 * over all V classes, the target included) and the PaLM z-loss with weight zeta = z_loss_weight >= 0,
 *     loss[m] = lse_m - (1 - eps) logit[m][t_m] - eps zbar_m + zeta lse_m^2,     zbar_m = mean_v logit[m][v] = A[m] . wbar + bbar,
 * one more D-long dot product per row.  wbar [D] f32 / bbar [1] f32: the means over the V rows of W and over the bias, left on the device by
 * pk_vocab_weight_mean (the host never reads them); they may be NULL when label_smoothing == 0.  lse_out is the plain log-sum-exp.
 * label_smoothing outside [0, 1), z_loss_weight < 0 or not finite, wbar / bbar == NULL with label_smoothing > 0: PK_EINVAL.
 * pk_vocab_ce is the (0, 0, NULL, NULL) call: it launches the same kernel it always did. */
int pk_vocab_ce_reg(int dtype, const void* partials, int M, int V, const void* A, int lda, const void* W, int ldw,
                    const float* bias, int D, const long long* targets, const int* rows, float* loss, float* lse_out,
                    float label_smoothing, float z_loss_weight, const float* wbar, const float* bbar, void* stream);
/* wbar[c] = mean_v W[v][c] (c < D) and bbar[0] = mean_v bias[v] of a vocabulary head, from the operand image W [V][ldw] exactly as the head's
 * main loop reads it (dtype 0 f32, 1 bf16, 2 the split-bf16 planes as hi + lo: ldw % 32 == 0).  One streaming pass, two launches, a fixed
 * summation order without atomics: two calls agree bit for bit.  Only wbar[0, D) and bbar[0] are written.
 * workspace: pk_vocab_weight_mean_words(dtype, V, D) 4-byte words.  D and ldw multiples of 4 (bf16: 8), W 16-byte aligned. */
int pk_vocab_weight_mean_words(int dtype, int V, int D);
int pk_vocab_weight_mean(int dtype, const void* W, int ldw, const float* bias, int V, int D, float* wbar, float* bbar, void* workspace,
                         void* stream);
/* The validation statistics of the vocab head (what a MaskGIT-style model is judged by: masked-token perplexity, top-k accuracy, the rank
 * of the true token, the entropy of the predictive distribution) in one pass over the vocabulary, again without the logits; same A / lda /
 * W / ldw / bias / M / V / D / rows as pk_vocab_sample, no noise, no temperature, no atomics.  pk_vocab_eval first forms the target logit
 * t[m] = A[m] . W[targets[r]] + bias[targets[r]] (r = rows ? rows[m] : m, the dot product of pk_vocab_ce), then runs the tiled 128 x 128
 * vocabulary kernel with an epilogue that leaves per (row, tile) the plain arg-max (first maximum wins), max, sum exp(l - max),
 * sum exp(l - max) l and `greater`, the number of columns v != targets[r], v < V, with l_v > t[m] -- the target's own column is left out by
 * INDEX, its MFMA value and t[m] may differ in the last bits.  workspace: pk_vocab_eval_words(V) * M 4-byte words.
 * pk_vocab_eval_reduce folds the tiles of that workspace in a fixed order into per-row outputs, each [M] or NULL: pred (arg-max), lse,
 * nll = lse - t, rank = sum of `greater` (exact; top-k accuracy is rank < k) and entropy = lse - sum_v p_v l_v in nats.  Two calls on the
 * same inputs agree bit for bit.  A target outside [0, V) reads no weight row: its nll is nan and its rank 0. */
int pk_vocab_eval_words(int V);
int pk_vocab_eval(int dtype, const void* A, int lda, const void* W, int ldw, const float* bias, int M, int V, int D,
                  const long long* targets, const int* rows, void* workspace, void* stream);
int pk_vocab_eval_reduce(const void* workspace, int M, int V, long long* pred, float* lse, float* nll, int* rank, float* entropy,
                         void* stream);

/* pk_vocab_ce's lse_out ([M] f32 or NULL): logsumexp of every row, kept for the backward pass below.
 *
 * Backward of that cross entropy (first training kernel; phenaki_pytorch.py:640-643 under autograd), one slab of
 * Vs vocabulary columns [v0, v0 + Vs) at a time: logits [M][ldl] f32 holds the slab's recomputed logits (pk_gemm of the same A / W rows
 * / bias); g[m][v] = (exp(logit - lse[m]) - [v0 + v == targets[r]]) * scale (r = rows ? rows[m] : m; scale = upstream gradient / number
 * of rows) is written to g [M][ldg] and, transposed with zeroed pad columns, to gT [Vs][ldgt] (ldgt >= M: the K-padded A operand of the
 * dW GEMM), both f32 or bf16 (out_bf16); db [Vs] (or NULL) receives the column sums of g.  The caller then runs dE += g W_slab and
 * dW_slab = gT E through pk_gemm: the (M, V) logits / probabilities never exist. */
int pk_ce_grad_slab(int out_bf16, const float* logits, int ldl, const float* lse, const long long* targets, const int* rows,
                    int M, int Vs, int v0, float scale, const float* scale_dev, void* g, int ldg, void* gT, int ldgt, float* db, void* stream);
/* scale_dev (or NULL): a device scalar multiplied into scale -- the upstream gradient of the loss, read on the device */
/* The gradient of the regularised loss (pk_vocab_ce_reg), same buffers:
 *     g[m][v] = (exp(logit - lse[m]) (1 + 2 zeta lse[m]) - (1 - eps) [v0 + v == targets[r]] - eps / V_total) * scale,
 * V_total the WHOLE vocabulary (v0 + Vs <= V_total), not the slab; dE, dW and db follow from g as before.  Argument errors as pk_vocab_ce_reg;
 * pk_ce_grad_slab is the (0, 0, -) call and launches the same kernel it always did. */
int pk_ce_grad_slab_reg(int out_bf16, const float* logits, int ldl, const float* lse, const long long* targets, const int* rows,
                        int M, int Vs, int v0, float scale, const float* scale_dev, void* g, int ldg, void* gT, int ldgt, float* db,
                        float label_smoothing, float z_loss_weight, int V_total, void* stream);

/* phenaki_pytorch.py:488-491: mask = zeros.scatter(1, scores.topk(k).indices, 1).bool(); ids = where(mask, mask_id, ids).
 * rows_out (B*k int32, or NULL) receives the flat positions b*n + i of the masked tokens: only those rows need the vocab
 * head in this step (pk_cfg_mix / pk_vocab_sample / pk_vocab_reduce take it as `rows`).  scores_next (B*n, or NULL; must
 * not alias scores) is filled with -1e4: the critic-less confidence scores where(mask, 1 - p, -1e4) of :547-550, whose
 * masked rows pk_vocab_reduce overwrites afterwards. */
int pk_topk_mask(const float* scores, int B, int n, int k, long long mask_id, unsigned char* mask, long long* ids,
                 int* rows_out, float* scores_next, void* stream);
/* pk_topk_mask with an exclusion mask and a per-row k: the re-masking step of infilling (Phenaki.sample(known_ids=, known_mask=)).
 *   k, row_off : device int32[B]; row_off is required when rows_out is given.
 *   known      : device uint8[B][n], nonzero = keep the token; NULL = nothing is excluded.
 *   scores     : NULL = all scores equal, so the rank of a free position is its index among the row's free positions (step 0: with
 *                k[b] = the row's free count this masks and lists every free position, a pure compaction).
 * mask[b][i] = 1 iff position i is free and fewer than k[b] FREE positions of row b rank before it (larger score, ties to the lower
 * index), 0 elsewhere, known positions included.  Known positions are excluded by index, not by score value: they are never ranked,
 * never counted in another position's rank, never masked, and their ids are never written.  ids = mask_id where masked, untouched
 * elsewhere.  rows_out[row_off[b] + rank] = b*n + i; nothing is written outside [row_off[b], row_off[b] + k[b]).  scores_next (B*n, or
 * NULL; must not alias scores) is -1e4 at EVERY position, as in pk_topk_mask.  Same geometry as pk_topk_mask (grid (B, ceil(n/64)), four
 * lanes per position, the row and its known bytes in 5 n bytes of dynamic LDS: n <= 12288).
 * PK_EINVAL before any launch: NULL k / mask / ids, B <= 0, n <= 0, n > 12288, rows_out without row_off, scores_next == scores.
 * k[b] above the row's free count cannot be seen without a device read: the caller guarantees k[b] <= free count (then every slot of
 * the row's rows_out range is written); the Python wrapper checks it where it holds the host counts. */
int pk_topk_mask_keep(const float* scores, int B, int n, const int* k, const int* row_off, const unsigned char* known,
                      long long mask_id, unsigned char* mask, long long* ids, int* rows_out, float* scores_next, void* stream);
/* Infill compositing (Phenaki.infill(composite=True)): out[b][c][p] = mask[b][p] ? gen[b][c][p] : src[b][c][p] over (B, C, P) f32 with
 * P = F*H*W pixels per channel; mask is uint8 (mask_batch, P) with mask_batch == B or 1 (shared by the batch).  A select: where the mask
 * is 0 the output holds the source's bits.  out is a buffer of its own. */
int pk_composite_mask(const float* gen, const float* src, const unsigned char* mask, float* out, int B, int C, long long P,
                      int mask_batch, void* stream);

/* phenaki_pytorch.py:246-263, 523-545: critic head Linear(dim,1) + CFG mix + noise_mult * (u - 0.5), prime dropped.
 * u [nb][n] U[0,1) draws, or NULL: drawn in the kernel from the counter hash of seed (+ *seed_dev, see pk_vocab_sample). */
int pk_critic_head(const float* x, int ldx, const float* w, const float* b, int D, int nb, int n_tot, int n_prime,
                   int has_null, float scale, const float* u, float noise_mult, unsigned long long seed,
                   const unsigned long long* seed_dev, float* out, void* stream);
/* pk_critic_head with pk_guidance_mix's table in place of scale / has_null (phenaki_pytorch.py:251-263 generalised): the head's scalar
 * outputs s_k of the rows [cond_0 | .. | cond_{P-1} | base] are mixed by the same formula, s = s_0 | sum_k a[k][b] s_k, then
 * s_base + (s - s_base) * g[b]; the row dot product is the device function pk_critic_head uses, so P == 1 is bit-identical to it.
 * Noise (u, the counter hash, seed_dev) as in pk_critic_head.  PK_EINVAL as pk_guidance_mix. */
int pk_critic_head_guided(const float* x, int ldx, const float* w, const float* b, int D, int nb, int n_tot, int n_prime,
                          const float* coef, int P, int has_base, const float* u, float noise_mult, unsigned long long seed,
                          const unsigned long long* seed_dev, float* out, void* stream);

/* ---- training step, SURVEY.md 8f row 1: backward of the MaskGit / TokenCritic trunk (phenaki_pytorch.py:562-687 under autograd; host side
 * phenaki_pytorch_amd/train.py).  Activations and gradients are f32; the matrix products are pk_gemm calls on operands laid down by pk_pack.
 *
 * pk_pack: f32 matrix -> GEMM operand image.  out[r][k] = (transpose ? src[k][r] : src[r][k]) for r < R, k < K, zero for K <= k < Kp; out has ldo
 *   elements per row; kind 0 f32, 1 bf16, 2 the split-bf16 image (128-byte aligned, ldo % 32 == 0).  dX = dY W takes W^T, dW = dY^T X takes
 *   dY^T as A and X^T as the "W" operand (the contraction index of pk_gemm is the contiguous one). */
int pk_pack(const float* src, long long lds, const int* rows, int R, int K, int transpose, void* out, long long ldo, int Kp, int kind, void* stream);
/* Several pk_pack jobs in ONE launch (round 6; the reference has no counterpart: under autograd each of these is an ATen transpose / cast inside
 * F.linear's backward, attention.py:45-53, :117-119).  A job = one output block, flags = transpose | kind << 1, alignment rules of pk_pack except
 * that `out` may be any 16-byte aligned position inside a 128-byte aligned kind-2 image (a column block of it); tile0 / tiles_x are filled in by
 * the library.  pk_pack_multi: count <= 8 HOST jobs, carried in the kernel arguments (the activation transposes of one backward block).
 * pk_pack_table_prepare + pk_pack_table: any number of jobs -- prepare fills a HOST array and returns the tile count of the launch (< 0: error),
 * the caller keeps a copy in DEVICE memory and replays it every step (the persistent operand images of a Transformer's weights). */
typedef struct PkPackJob {
    const float* src; void* out; long long lds, ldo; int R, K, Kp, flags, tile0, tiles_x;
} PkPackJob;
int pk_pack_multi(const void* jobs, int count, void* stream);
int pk_pack_table_prepare(void* jobs, int count);
int pk_pack_table(const void* dev_table, int count, int tiles, void* stream);
/* rows (or NULL) gathers SOURCE rows: out[r][k] = src[rows[k]][r] (transpose) / src[rows[r]][k].   pk_scatter_rows: dst[rows[m]] = src[m], m < M */
int pk_scatter_rows(const float* src, long long lds, const int* rows, float* dst, long long ldd, int M, int D, void* stream);
/* out[c] (accumulate ? += : =) scale * sum_r src[r][c], two deterministic stages (one launch when M <= 1024 and the rows are float4-addressable,
 * or M <= 256: the per-block partials of the backward kernels); work: pk_colsum_parts(M) * N floats */
int pk_colsum_parts(int M);
int pk_colsum(const float* src, long long ld, int M, int N, float scale, float* out, int accumulate, float* work, void* stream);
/* LayerNorm backward (attention.py:29-36, :47): dx = [add +] rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma; pg / pb (pb may be NULL):
 * (pk_ln_bwd_parts(M), D) per-block partials of dgamma = sum dy xhat / dbeta = sum dy, finished by pk_colsum */
int pk_ln_bwd_parts(int M);
int pk_layernorm_bwd(const float* x, long long ldx, const float* gamma, const float* dy, long long lddy, const float* add, long long ldadd,
                     float* dx, long long lddx, float* pg, float* pb, float eps, int M, int D, void* stream);
/* GEGLU on stored pre-activations h (M, >= goff + F): out = h[:, :F] * gelu(h[:, goff : goff + F]) (attention.py:40-43), and its backward.
 * drop = ff_dropout: out = geglu(h) o m * scale in the same pass; pk_geglu_bwd: dout o m * scale in front of the GEGLU derivative. */
int pk_geglu(const float* h, long long ldh, int goff, float* out, long long ldo, int M, int F, const pk_dropout* drop, void* stream);
int pk_geglu_bwd(const float* h, long long ldh, int goff, const float* dout, long long ldd, float* dh, long long lddh, int M, int F, const pk_dropout* drop,
                 void* stream);
/* ---- dropout of the training kernels (attention.py:45-52 ff_dropout behind GEGLU, attention.py:177 attn_dropout on the softmax probabilities).
 * A dropout site is a stream (seed, offset); whether element (row, col) of the site survives is a pure function of (seed, offset, row, col)
 * (csrc/common.hpp drop_keys / drop_row / drop_word / drop_keep; NumPy mirror phenaki_pytorch_amd/dropout.py), so masks are regenerated in the
 * backward kernels, never stored.  row / col are the factors of the logical element index row * cols + col: attention row = (s heads + h) n + i,
 * col = j over the nnull + n_kv keys (null keys first); feed-forward row = token row, col over the inner width.  An element is dropped iff its 8-bit
 * draw < keep_thr (p_eff = keep_thr / 256); survivors are multiplied by `scale`, which the host computes as 1 / (1 - p_eff) in ONE place
 * (dropout.py quantize).  keep_thr in [1, 256] for the kernels that apply a mask.  Statistically equivalent to torch's nn.Dropout, not its stream.
 * pk_dropout_mask: out (rows, cols) bytes, 1 = keep, for the index range [0, rows) x [0, cols) (keep_thr in [0, 256]; rows < 2^32). */
int pk_dropout_mask(unsigned long long seed, unsigned long long offset, int keep_thr, long long rows, int cols, unsigned char* out, void* stream);
/* dz = dy * (y > 0 ? 1 : slope): LeakyReLU backward from the activation's output (position-bias MLP, attention.py:243-247) */
/* the tokenizer's reconstruction step (cvivit.py:585-591 under autograd; the LFQ's straight-through estimator):
 * pk_scaled_diff: out = (a - b) * scale (* *scale_dev when given) over n floats (n % 4 == 0) -- d/da of (scale / 2) sum (a - b)^2;
 * pk_sign: out = z > 0 ? +value : -value (the code of an LFQ projection, cvivit.py:570 -> vector_quantize_pytorch LFQ.forward). */
int pk_scaled_diff(const float* a, const float* b, float scale, const float* scale_dev, float* out, long long n, void* stream);
int pk_sign(const float* z, float value, float* out, long long n, void* stream);
int pk_mul(const float* a, const float* b, float* out, long long n, void* stream);     /* out = a * b (may alias a), n % 4 == 0 */
int pk_leaky_bwd(const float* y, long long ldy, const float* dy, long long lddy, float* dz, long long lddz, int M, int N, float slope, void* stream);
/* PEG backward (attention.py:57-85 + residual :323): dx = dy + transposed stencil of dy; part (NULL: skip): (pk_peg_wgrad_parts(rows), 27, D)
 * partial tap gradients sum dy[pos] x[pos + tap], finished by pk_colsum over 27 D columns (the conv bias gradient is pk_colsum of dy) */
int pk_peg_adjoint(const float* dy, const float* wt, float* dx, int B, int T, int H, int W, int D, int causal, void* stream);   /* dx only, W in {4, 8, 16} (else PK_EINVAL) */
int pk_peg_wgrad_parts(long long rows);
int pk_peg_bwd(const float* dy, const float* x, const float* wt, float* dx, float* part, int B, int T, int H, int W, int D, int causal, void* stream);
/* token + position embedding backward (phenaki_pytorch.py:194-199, alpha = gradient_shrink_alpha): dpos (n, D) overwritten, dtok (zeroed by
 * the caller) += by f32 atomics */
int pk_embed_bwd(const float* dy, const long long* ids, float alpha, float* dtok, float* dpos, int S, int n, int D, void* stream);
/* position bias (attention.py:257-275): out[h][i][j] = tab[code[i] - code[j] + off][h] and its adjoint (dtab zeroed by the caller, f32 atomics) */
int pk_bias_gather(const float* tab, int ldt, const int* code, int off, float* out, int heads, int n, void* stream);
int pk_bias_scatter(const float* dbias, const int* code, int off, float* dtab, int ldt, int heads, int n, void* stream);
/* out[e] = sum_s src[s * stride + e], e < E (E % 4 == 0) */
int pk_sum_batch(const float* src, long long stride, int S, float* out, long long E, void* stream);
/* count <= 8 short column sums in one launch (the one-launch form of pk_colsum: M <= 8192, N % 4 == 0, 16-byte aligned rows; blk0 filled in by the library) */
typedef struct PkColsumJob { const float* src; float* out; long long ld; int M, N, blk0; float scale; } PkColsumJob;
int pk_colsum_multi(const void* jobs, int count, void* stream);
/* both job lists of a backward block (<= 8 each, either may be empty) in ONE launch */
int pk_reduce_multi(const void* sum_jobs, int nsum, const void* col_jobs, int ncol, void* stream);
/* count <= 8 pk_sum_batch jobs in one launch (E4 = E / 4; blk0 is filled in by the library): the K-slice partials of one block's weight gradients */
typedef struct PkSumJob { const float* src; float* out; long long stride, E4; int S, blk0; } PkSumJob;
int pk_sum_batch_multi(const void* jobs, int count, void* stream);
/* critic head + BCE-with-logits forward and backward in one pass (phenaki_pytorch.py:246-249, :673-676): logits / loss_rows (M) optional;
 * labels NULL: logits only; de = dz w with dz = (sigmoid(z) - y) scale; pw (pk_ln_bwd_parts(M), D) / pb (pk_ln_bwd_parts(M)) partials of dw / db */
int pk_bce_head(const float* e, long long lde, const float* w, const float* b, const float* labels, float scale, const float* scale_dev, float* logits, float* loss_rows,
                float* de, long long ldde, float* pw, float* pb, int M, int D, void* stream);
/* split-K product for the weight gradients (dW = dY^T X contracts over the rows of the batch): C[z] = A[:, z Kc : (z + 1) Kc] W[:, z Kc : (z + 1) Kc]^T,
 * Kc = K / splits (a multiple of the k-tile), z < splits, as `splits` partial (M, N) f32 matrices at C + z * M * ldc; add them with pk_sum_batch.
 * A: T for dtype 1, f32 for dtype 0 / 2; W: the operand image of the dtype.
 * bias ([N] or NULL) is added by slice 0 only (the sum of the slices carries it once); tile 0: 64 x 64 tiles, 1: 128 x 128 (long K-slices of a large
 * (M, N): the patch-embedding product of the exact-f32 / split-bf16 modes, K = 6144), 2 (dtype 1 only, round 6): 256 x 256 tiles on the two-group loop of
 * csrc/gemm_p8.hpp -- few tiles, long K. */
int pk_gemm_splitk(int dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, int splits, float* C, int ldc,
                   const float* bias, int tile, void* stream);
/* AdamW / Adam update of one parameter tensor (reference optimizer.py:11-37 hands MaskGit's parameters to torch.optim.AdamW / Adam):
 * m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; p = p (1 - lr wd) - lr / (1 - b1^step) * m / (sqrt(v / (1 - b2^step)) + eps); step = 1, 2, ... */
int pk_adamw(float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2, float eps, float wd, int step, long long n, void* stream);
/* the same update for `count` tensors sharing hyper-parameters and step in a handful of launches: table = HOST array of count x 5 64-bit
 * words {p, g, m, v, numel} (device pointers of contiguous f32 tensors).  Bit-identical to per-tensor pk_adamw calls. */
int pk_adamw_multi(const long long* table, int count, float lr, float beta1, float beta2, float eps, float wd, int step, void* stream);
/* the tail of a training step (reference cvivit_trainer.py:245-246, 268-269, 282; phenaki_trainer.py:380-381): global-norm gradient clipping and the
 * exponential moving average of a model's weights.  Tables are HOST arrays of 64-bit words, device pointers of contiguous f32 tensors, numel > 0;
 * the launches are packed as pk_adamw_multi packs them.  No atomics: no result depends on launch order or block scheduling.
 * pk_grad_sumsq_parts: the number of f32 partial sums pk_grad_sumsq writes for a table of count x {g, numel} (host only; < 0: an error code).
 * pk_grad_sumsq: partials[b] = the sum of squares of one fixed chunk of one gradient; nparts must be what pk_grad_sumsq_parts returned.
 * pk_grad_clip_coef: out[0] = total_norm = sqrt(the partials summed in index order, in double), out[1] = min(max_norm / (total_norm + 1e-6), 1)
 * in f32 -- the values of torch.nn.utils.clip_grad_norm_(norm_type = 2, error_if_nonfinite = False): a NaN norm gives a NaN coefficient.
 * pk_scale_multi: g = g * *coef_dev in place (one rounded multiply), the coefficient read from device memory.
 * pk_adamw_multi_scaled: pk_adamw_multi with every gradient element read as g * *gscale_dev (one rounded multiply): bit-identical to
 * pk_scale_multi followed by pk_adamw_multi, without writing the gradients.
 * pk_ema_multi: table of count x {ema, src, numel}; ema = ema + weight (src - ema); weight >= 1 stores src verbatim (an exact copy). */
int pk_grad_sumsq_parts(const long long* table, int count);
int pk_grad_sumsq(const long long* table, int count, float* partials, long long nparts, void* stream);
int pk_grad_clip_coef(const float* partials, long long nparts, float max_norm, float* out, void* stream);
int pk_scale_multi(const long long* table, int count, const float* coef_dev, void* stream);
int pk_adamw_multi_scaled(const long long* table, int count, float lr, float beta1, float beta2, float eps, float wd, int step,
                          const float* gscale_dev, void* stream);
int pk_ema_multi(const long long* table, int count, float weight, void* stream);
/* attention backward (attention.py:132-182).  pk_attn_train_prep: the f32 operands q^ = l2norm(q) q_scale scale -> Qh (S heads, n, 64),
 * k^ = l2norm([null_k ; k]) k_scale -> Kh, [null_v ; v] -> Vh (S heads, nnull + n_kv, 64) from the projection outputs q (S n, ldq), kv (S n_kv, ldkv).
 * pk_attn_bwd_ws: dQh / dKh / dVh from those, the forward output O (f32 or bf16) and dO; bias (heads, n, n_kv) / kmask (S, n_kv) cover the real keys;
 * dS (S heads, n, n_kv; optional) = the score gradient for the position-bias gradient (pk_sum_batch over S); lse / Drow: (S heads n) scratch;
 *   causal (attention.py:166-172, the C-ViViT temporal transformers): ALiBi slopes [heads] over all nnull + n keys and the causal mask;
 *   split_bf16: a flag word -- bit 0: the tile products on the bf16 matrix cores from (hi, lo) splits of the f32 operands (the bf16x3 / bf16 modes),
 *   else exact f32; bit 1: `lse` already holds every row's log-sum-exp (pk_attn_fwd_lse), else it is scratch the first kernel fills.
 *   pq / pk may be the two 64-column halves of ONE (1024, 128) buffer (pk == pq + 64: rows are then 128 floats apart) so that one pk_colsum finishes
 *   both; likewise pg / pb of pk_layernorm_bwd (pb == pg + D: rows 2 D apart).
 * pk_attn_train_prep_bwd: back through l2norm / scales / null keys: dq, dkv, partials pq / pk (1024, 64) of dq_scale / dk_scale, dnull (heads, 2 nnull, 64). */
int pk_attn_train_prep(const float* q, long long ldq, const float* kv, long long ldkv, const float* null_kv, const float* q_scale, const float* k_scale,
                       float scale, float* Qh, float* Kh, float* Vh, int S, int heads, int n, int n_kv, int nnull, void* stream);
int pk_attn_train_prep_bwd(const float* q, long long ldq, const float* kv, long long ldkv, const float* null_kv, const float* q_scale, const float* k_scale,
                           float scale, const float* dQh, const float* dKh, const float* dVh, float* dq, long long lddq, float* dkv, long long lddkv,
                           float* pq, float* pk, float* dnull, int S, int heads, int n, int n_kv, int nnull, void* stream);
/* work: a workspace of pk_attn_bwd_work(...) floats (0: none needed, NULL): with few key tiles (cross-attention on 14 keys: one tile per head) the
 * query tiles of a key tile are dealt to several workgroups whose partial dK^ / dV slabs are added in index order (deterministic).
 * drop: the site pk_attn_fwd_lse ran with (attention.py:177 under autograd): dP = (dO V^T) o m * scale, dS = P o (dP - D) with D = rowsum(dO o O) of
 * the dropped O, dV = (P o m * scale)^T dO; the optional dS output carries the mask too.  All three product forms of the flag word; the packed
 * short-sequence layout is not used; S heads n <= 2^32 - 1. */
int pk_attn_bwd_work(int S, int heads, int n, int n_kv, int nnull);
int pk_attn_bwd_ws(const float* Qh, const float* Kh, const float* Vh, const void* O, long long ldo, int o_bf16, const float* dO, long long lddo,
                   const float* bias, const unsigned char* kmask, const float* slopes, int causal, float* dQh, float* dKh, float* dVh, float* dS,
                   float* lse, float* Drow, int S, int heads, int n, int n_kv, int nnull, int split_bf16, float* work, long long work_floats,
                   const pk_dropout* drop, void* stream);

/* ---- the tokenizer's adversarial branch: cvivit.py:59-213 (Discriminator), :604-671 (hinge / gradient penalty / adaptive weight).
 * Images are CHANNELS-LAST pixel rows x[(b, y, x)][c] (f32, C % 4 == 0), so every nn.Conv2d (cvivit.py:115-127, 191) is pk_gemm on a patch matrix:
 * pk_im2col: cols[(b, yo, xo)][(ky * kw + kx) * C + c] = x[b][yo stride + ky - pad][xo stride + kx - pad][c], zero outside the image
 *   (3x3 / pad 1: the net convolutions; 1x1 / stride 2: conv_res; 2x2 / stride 2: Rearrange('b c (h p1) (w p2) -> b (c p1 p2) h w') + 1x1 conv);
 * pk_col2im: its adjoint in gather form (input gradient of the convolution; deterministic).
 * pk_nchw_to_rows / pk_rows_to_nchw: (B, C, H, W) <-> rows[(b, y, x)][Cp] with channels C..Cp-1 zero / dropped (mutually adjoint).
 * pk_pick_frames: pick_video_frame (cvivit.py:217-224) img[b] = video[b, :, frame[b]] (place = 0), or the adjoint into a zeroed video (place = 1);
 *   frame: B device int32 indices; an index outside [0, F) reads as a zero frame / is not written (never an out-of-bounds access).
 * pk_bmm: C[z] = op(A[z]) op(B[z]) (+ C[z]) in exact f32 for any shape / leading dimension / batch stride (elements): the fallback product of the
 *   second-order graph of gradient_penalty (cvivit.py:59-73) and of the 64-token attention block inside the discriminator (cvivit.py:166-168). */
int pk_im2col(const float* x, int B, int H, int W, int C, int kh, int kw, int stride, int pad, float* cols, long long ldc, void* stream);
int pk_col2im(const float* cols, long long ldc, int B, int H, int W, int C, int kh, int kw, int stride, int pad, float* dx, void* stream);
int pk_nchw_to_rows(const float* img, int B, int C, int H, int W, int Cp, float* rows, void* stream);
int pk_rows_to_nchw(const float* rows, int B, int C, int H, int W, int Cp, float* img, void* stream);
int pk_pick_frames(float* video, const int* frame, int B, int C, int F, int H, int W, float* img, int place, void* stream);
int pk_bmm(const float* A, long long lda, long long sA, int tA, const float* B, long long ldb, long long sB, int tB, float* C, long long ldc,
           long long sC, int batch, int M, int N, int K, int accumulate, void* stream);
/* Row-wise pieces of the discriminator's attention block WITH their second derivatives (gradient_penalty differentiates the input gradient through the
 * block: cvivit.py:59-73, 166-168; attention.py:29-36, 153-155, 176); one wave per row, contiguous f32 rows.
 * pk_row_softmax   mode 0: out = softmax(a);  1: out = a (b - <a, b>)  (a = y, b = dy: the backward);  2: out = c (b - <a, b>) - b <c, a>  (the gradient
 *                  of <c, backward> with respect to y; with respect to dy it is mode 1 with b = c).
 * pk_row_l2scale   mode 0: o0 = x / |x| * sc  (F.normalize, then q_scale / k_scale);  1: o0 = dx, o1 = per-row contributions to dsc, from dz;
 *                  2: o0 = grad_x, o1 = per-row contributions to grad_sc, o2 = grad_dz of <gx, dx> + <gsc, dsc>.
 * pk_row_ln_bwd2   the same for the gamma-only LayerNorm's backward (pk_layernorm_bwd): u = upstream of dx [M][D], w = upstream of dgamma [D].
 * The per-row contributions are summed over rows by pk_colsum. */
int pk_row_softmax(const float* a, const float* b, const float* c, float* out, long long M, int n, int mode, void* stream);
int pk_row_l2scale(const float* x, const float* sc, const float* dz, const float* gx, const float* gsc, float* o0, float* o1, float* o2,
                   long long M, int d, int mode, void* stream);
int pk_row_ln_bwd2(const float* x, const float* gamma, const float* dy, const float* u, const float* w, float eps, float* grad_x,
                   float* grad_gamma_rows, float* grad_dy, long long M, int D, void* stream);

/* ---- the perceptual network of the tokenizer's GAN objective: reference cvivit.py:349-352 (torchvision VGG16, classifier[:-2]) and :636-651
 * (F.mse_loss(vgg(frame), vgg(recon frame)), whose gradient reaches the tokenizer through the reconstructed frame).  Channels-last pixel rows
 * x[(b, y, x)][c] as above, C % 8 == 0 (the 3-channel frame padded to 8 by pk_nchw_to_rows).  csrc/vgg.hip.
 * pk_conv3x3: y[(b,y,x)][co] = act(bias[co] + sum_{ky,kx,c} x[(b, y+ky-1, x+kx-1)][c] W[co][(ky*3+kx)*C + c]), stride 1, pad 1, zero outside the image:
 *   a DIRECT convolution (implicit GEMM, the patch matrix of pk_im2col is never written).  W [Co][ldw] is the pk_gemm weight image of `dtype` over
 *   K = 9 C columns in pk_im2col's order (ldw >= K rounded up to 64 for dtype 1, 32 otherwise, zero padded: pk_pack); dtype / a_is_f32 / out_is_f32 as
 *   pk_gemm (0 exact f32, 1 bf16 MFMA with f32 or bf16 x and y, 2 split-bf16 with W in the plane format).  act: 0 none, 1 ReLU; bias optional.
 *   gate (optional; [B H W][ldg], f32 or bf16 by gate_is_f32): x[r][c] is read as 0 wherever gate[r][c] <= 0 -- with x = dy, gate = the saved post-ReLU
 *   output and W = Wb, Wb[c][((2-ky)*3 + (2-kx))*Co + co] = W[co][(ky*3+kx)*C + c], this is the input gradient of relu(conv) (no weight gradient exists).
 *   tile: 0 automatic, 1 = 64 x 64, 2 = 128 x 64, 3 = 128 x 128 (rows x output channels per workgroup; tools/vgg_time.py).  Co % 4 == 0, B H W < 2^31 - 256.
 * pk_maxpool2x2 / _bwd: nn.MaxPool2d(2, 2) on rows of f32 or bf16 (is_f32), output (H / 2) x (W / 2) (floor); the backward routes dy to the FIRST maximum
 *   of each window in scan order (0,0), (0,1), (1,0), (1,1) (torch's rule), recomputed from the saved input x; gather form, deterministic; dy / dx f32.
 * pk_adaptive_avgpool / _bwd: nn.AdaptiveAvgPool2d((7, 7)) with torch's windows [floor(i s / 7), ceil((i + 1) s / 7)), any H, W >= 1; out / dy
 *   [(b, i, j)][c] f32; the backward in gather form. */
int pk_conv3x3(int dtype, int a_is_f32, const void* x, int B, int H, int W, int C, const void* Wm, int ldw, int Co, const float* bias, int act,
               const void* gate, int ldg, int gate_is_f32, void* y, int ldy, int out_is_f32, int tile, void* stream);
int pk_maxpool2x2(int is_f32, const void* x, int B, int H, int W, int C, void* y, void* stream);
int pk_maxpool2x2_bwd(int is_f32, const void* x, const float* dy, int B, int H, int W, int C, float* dx, void* stream);
int pk_adaptive_avgpool(int is_f32, const void* x, int B, int H, int W, int C, float* out, void* stream);
int pk_adaptive_avgpool_bwd(const float* dy, int B, int H, int W, int C, float* dx, void* stream);

/* ---- validation metrics of the tokenizer (csrc/metrics.hip; the reference's trainer only dumps image grids, cvivit_trainer.py:284-323).  a, b:
 * contiguous f32 videos (B, C, F, H, W), 4-byte aligned (16-byte loads are used where the addresses allow them, the results do not depend on it);
 * results per frame, (B, F) f32, the C planes of a frame combined.  clamp_hi > 0: the FIRST operand is read as min(max(a, 0), clamp_hi) (no copy is
 * written); <= 0: as it is.  partials: planes x pk_frame_*_parts(H, W) doubles of workspace (nparts = that product), one slot per workgroup, added
 * per frame in index order: no floating-point atomics, bit-reproducible.  Always f32 arithmetic, whatever the model's compute dtype.
 *   pk_frame_sqerr: mse[b, f] = mean over C H W of (a - b)^2, any H, W >= 1; psnr (optional) = 10 log10(R^2 / max(mse, 1e-10 R^2)), R = data_range,
 *                   formed from the unrounded mean (identical frames: exactly 100).
 *   pk_frame_ssim:  SSIM of Wang et al. as pytorch-msssim / torchmetrics compute it: 11 x 11 Gaussian window (sigma 1.5, sum 1), 'valid' positions
 *                   (H - 10) x (W - 10), biased moments, C1 = (0.01 R)^2, C2 = (0.03 R)^2, the map averaged over the positions and planes of the frame.
 *                   H, W >= 11.  The moments are accumulated on a - s, b - s (s = the tile's mean of a), never as E[a^2] - E[a]^2 on raw pixels;
 *                   identical frames give exactly 1.
 *   pk_code_usage:  counts (V,) int32 as pk_vq_hist writes them -> out[0..5) doubles: total T, codes with count > 0, entropy H = -sum p ln p over p > 0
 *                   (p = count / T), perplexity exp(H), max p.  T = 0: 0, 0, 0, 1, 0.  One workgroup, fixed-order sums. */
int pk_frame_sqerr_parts(int H, int W);
int pk_frame_ssim_parts(int H, int W);
int pk_frame_sqerr(const float* a, const float* b, int B, int C, int F, int H, int W, float clamp_hi, float data_range, double* partials,
                   long long nparts, float* mse, float* psnr, void* stream);
int pk_frame_ssim(const float* a, const float* b, int B, int C, int F, int H, int W, float clamp_hi, float data_range, double* partials,
                  long long nparts, float* ssim, void* stream);
int pk_code_usage(const int* counts, int V, double* out, void* stream);

/* Cache policy of the result stores and read-once loads of the encode kernels (csrc/common.hpp).  The mask holds two bits
 * per site, site i at bits 2 i .. 2 i + 1: policy 0 = plain, 1 = write-through (sc1) stores, 2 = non-temporal stores / loads.  Sites:
 * 0 pk_gemm vector epilogue stores, 1 pk_qkv_attn O, 2 pk_peg (row kernel) outputs, 3 pk_layernorm / pk_layernorm_lfq outputs,
 * 4 pk_patch_embed_splitk partials + statistics, 5 pk_patch_embed_finish outputs; loads (0 or 2 only): 6 the video lines of
 * pk_patch_embed_splitk, 7 the partials of pk_patch_embed_finish, 8 the residual tile of pk_gemm.  Only cache bits change: results are
 * bit-identical under every mask.  The process default is the environment's PK_CACHE_POLICY (unset or invalid: 0x2000, non-temporal video loads, the measured
 * choice); the mask is read
 * on the host at every launch, so a captured graph keeps the value it was captured with.  pk_set_cache_policy: PK_EINVAL for an
 * unknown site or policy; pk_get_cache_policy returns the mask. */
int pk_set_cache_policy(unsigned mask);
int pk_get_cache_policy();

/* Compile-time epilogue forms of pk_gemm_ex (csrc/gemm.hip).  The three GEMM calls of a bf16 transformer block -- Attention
 * to_out, FeedForward first and second Linear -- run an epilogue in which every option is a compile-time constant, with one copy for
 * tiles inside the matrix (no bounds predicates) and one for edge tiles; results are bit-identical to the generic epilogue.  Forms:
 * 0 generic; 1 OUT (variant 8: f32 residual, f32 C, bf16 C2, stats_out); 2 FF2A (variant 8: f32 residual, f32 C, bf16 C2); 3 FF2B (the same
 * without C2); 4 FF1 (variant 24, LayerNorm fold with ln_stats: GEGLU, bf16 C).  All: dtype 1, vector epilogue, no bias, no scatter, no
 * dup_rows, both gemm cache policies plain.
 *   pk_gemm_epilogue_form: pure; the form of a launch from the fields it sees (variant: the resolved main loop; ln_kind 0 no fold, 1
 *                          in-loop statistics, 2 ln_stats; pol / pol_res: the policies of sites 0 and 8).
 *   pk_gemm_ex_form:       pk_gemm_ex's arguments without the stream -> the form that call would launch now (>= 0), or its error (< 0);
 *                          launches nothing, dereferences no pointer.
 *   pk_set_gemm_hot_forms: 0 forces form 0 for the launches that follow (default 1, or the environment's PK_GEMM_HOT_FORMS); read on the
 *                          host at every launch, so a captured graph keeps the form it was captured with. */
int pk_gemm_epilogue_form(int dtype, int variant, int ln_kind, int vec_ok, int act, int out_is_f32, int has_bias, int has_res, int has_c2,
                          int has_stats_out, int has_scatter, int dup_rows, int pol, int pol_res);
int pk_gemm_ex_form(int dtype, int a_is_f32, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias,
                    const float* res, int ldr, void* C, int ldc, int out_is_f32, int act, const int* a_rows, int a_nrows, int variant,
                    void* C2, int ldc2, const float* ln_s, const float* ln_t, float ln_eps, const int* row_off, const int* col_off,
                    float* stats_out, const float* ln_stats, int dup_rows);
int pk_set_gemm_hot_forms(int on);
int pk_get_gemm_hot_forms();

/* A-resident form of the FF1 call (csrc/gemm_resident.hpp): a pk_gemm_ex call that is exactly form 4 (FF1) with K = 512 and variant 0
 * (automatic, resolving to 24) runs ff1_resident_kernel -- a 128-row panel of A resident in LDS, W streamed to registers -- inside a measured window
 * of M; the bf16 output is bit-identical to the tiled kernel's.  pk_gemm_ex_form still reports 4.
 *   pk_set_ff1_resident:          0 the tiled kernel; 1 inside the window (default, or the environment's PK_FF1_RESIDENT); 2 at every M.  Read on the
 *                                 host at every launch, so a captured graph keeps the kernel it was captured with.
 *   pk_set_ff1_resident_workers:  tests only: n > 0 workgroups per panel and the resident kernel for every form-4 call at K = 512 (any M, any
 *                                 variant argument); 0 (default, or PK_FF1_RESIDENT_WORKERS) restores the rule above.
 *   pk_get_ff1_resident_launches: resident launches of this process so far. */
int pk_set_ff1_resident(int mode);
int pk_get_ff1_resident();
int pk_set_ff1_resident_workers(int n);
int pk_get_ff1_resident_launches();

/* A-resident form of the vocabulary head (csrc/sampler.hip vocab_resident_kernel): bf16, D = 512.  The same [tile][row] partials as the tiled kernel.
 *   pk_set_vocab_resident:          0 the tiled kernel; 1 / 2 force the 8- / 12-wave build at M >= 1024; 3 (default, or the environment's
 *                                   PK_VOCAB_RESIDENT) the measured rule: M >= 2048, 12 waves without the log-sum-exp state, 8 waves with it.  Read on the
 *                                   host at every launch, so a captured graph keeps the kernel it was captured with.  PK_EINVAL outside 0..3.
 *   pk_set_vocab_resident_workers:  tests only: n > 0 workgroups per XCD (grid 8 n) instead of 32; the kernel derives its work split from the grid.
 *                                   0 restores the default.  PK_EINVAL outside 0..256.
 *   pk_get_vocab_resident_launches: resident launches of this process so far. */
int pk_set_vocab_resident(int mode);
int pk_get_vocab_resident();
int pk_set_vocab_resident_workers(int n);
int pk_get_vocab_resident_launches();

#ifdef __cplusplus
}
#endif
#endif
