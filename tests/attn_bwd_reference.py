"""Float64 restatement of the attention backward (csrc/attn_train.hip: pk_attn_bwd_ws = attn_bwd_q_kernel<X3, DROP> + attn_bwd_kv_kernel<X3, DROP>), the seeded
cases that reach every branch of its dispatch, and a per-element checker whose bound is derived from the kernels' rounding points.  CPU only;
tests/test_attn_bwd_host.py shows what the checker rejects, tests/test_attn_bwd_gpu.py runs the kernels against it.  Built on tests/attn_fwd_reference.py (R).

Inputs go straight to pk_attn_bwd_ws, no prep kernel in between: Qh (S h, n, 64), Kh / Vh (S h, nkt, 64) f32, flat and exactly as long as the shape needs; dO
and O heads-merged (S n, h 64 + 8) views whose 8 slack columns are poisoned (NaN, +Inf in a second pass).  O is the reference's own P V (keep mask and scale
under dropout) rounded to its storage type (f32, bf16 in the o_bf16 cases); D = rowsum(dO o O) is DEFINED on that stored O, so its rounding is an input and not
an error.  With have_lse = 1 the lse handed in is the f64 log-sum-exp of the undropped scores rounded to f32.  For X3 = 2 (single bf16 products) Qh, Kh, Vh, dO
hold bf16-representable values (`rep`), as the forward's dtype-1 images do: only the in-kernel roundings of P and dS remain; the case general2_n65 runs X3 = 2
on general f32 operands and its bound carries the operand term.

Planted attention: the construction of R.build (targets dealt from the last key backwards, a `forbidden` component on the first key beyond the diagonal and on
a masked key, the -GAMMA shift that keeps the normaliser O(1)).  In the shapes the packed layout takes, all (sequence, head) pairs share one key set up to
noise, so a query that attended the next group's keys would find its own targets there.  planted_property() states what must hold: every planted (row, key)
holds >= MASS of the row's f64 softmax; a pair with at least as many rows as visible keys has every visible key planted, another pair every visible key of its
last 64-key tile, and every visible key is planted in the union over the pairs (a pair whose rows cannot hold even the last tile's keys, n = 1 against 70 keys,
plants what its rows hold); among the planted entries of rows with two or more visible keys at least PLANTED_DS_SHARE have |dS| >= PLANTED_DS_FACTOR x the
bf16-form bound of that entry (dS = P (dP - D) vanishes where the row has one key, and dP - D can be small by chance on single entries: the share, not
every entry; not asked beyond a drop rate of 1 / 2, where most rows keep nothing and dS = -P D vanishes with O).

Reference (closed form, f64): sim = Q K^T + bias over the real keys, ALiBi d slope with d = j - (nkt - n + i) over all keys and the causal mask, key mask over
the real keys only, masked scores = -finfo(float32).max as in the model; P = softmax, Pm = P o keep scale, dP = dO V^T, dS = P o (dP o keep scale - D), dS
zeroed at masked positions (masked_fill's gradient: it matters on a fully masked row only, where P = 1 / nkt is not 0), dQ = dS K, dK = dS^T Q, dV = Pm^T dO.
The keep mask is phenaki_pytorch_amd.dropout.keep_mask.  autograd_reference() differentiates a plain masked_fill / softmax attention instead; the host test
holds the closed form to it.

Host mirror of the dispatch: branch_of(c, X3, have_lse) -> packed / pack_g, (G, chunk) of kv_split_of, X3, DROP, have_lse, the dS store form.

Bound.  Per element, 2 x (sum of the first-order terms) + 2^-126; the factor 2 covers the second-order terms and the lower binade ends, as in R.  Every term is
a sum of ABSOLUTE contributions (dP - D cancels; dQ, dK, dV are signed sums).  u = 2^-24.  With mag_i = max_j (sum_d |q_id k_jd| + |bias| + |ALiBi|),
Adp_ij = sum_d |dO_id v_jd| keep scale, AD_i = sum_d |dO_id O_id|, T_ij = |dP_ij keep scale - D_i|, the error of one dS entry is P_ij times
  operand    op2 (mag_i T_ij + Adp_ij): the operand form of the Q K^T and dO V^T products (to_operand in mma_regA): 0 for f32, 3 * 2^-16 for split-bf16 (R's
             reasoning: two operand splits and the dropped lo.lo), 0 for X3 = 2 on bf16-representable operands, 2 * 2^-9 on general ones
  score      (64 + 3) u mag_i T_ij: the 64-term f32 accumulation of a score and the bias / ALiBi additions in score()
  exp        (3 + 2 * 24 ln 2) u T_ij: __expf(sc - lse): R's `exp` term with |x| <= 24 ln 2, once more for the rounding of the subtraction
  lse        el_i T_ij: the absolute error of the row's lse.  Handed over: 2^-23 |lse| (the f32 rounding of the input).  Computed (pass 1 of kernel Q):
             operand + score + (3 + 24 ln 2) u + (nkt + 3 tiles + 15) u (the online sums and the four cross-lane merges) + 2^-21 (v_log_f32 and the ln 2
             product, the constant R uses) + 2^-23 |lse|.  A fully masked row has P = 1 / nkt whatever its lse: operand, score, exp, lse are replaced by u there.
  dP         (64 + 1) u Adp_ij: the 64-term accumulation of dP and the product with the survivor scale
  D          10 u AD_i: 64 products, the pairwise adds of a lane's 16 and of the two chunks, two shuffles
  round      2 u T_ij: the subtraction and the product of `ds = P * (dp - D)`
dS itself is held to that; at masked positions the bound is 0 (+ 2^-126): the gradient is exactly 0.  dQ_id sums these over the keys against |k_jd| and adds
  lds_operand  opA sum_j |dS_ij k_jd|: mma_ldsA calls to_operand on the P / dS tile read back from LDS and on the B tile: 0, 3 * 2^-16, 2^-9 (B exact), 2 * 2^-9
  accumulate   (terms + 3) u sum_j |dS_ij k_jd|: the f32 accumulation over the keys (dQ) or the query rows plus the in-order slab sum (dK, dV: n + G + 3)
dK_jd the same over the query rows against |q_id|; dV_jd = sum_i Pm_ij dO_id takes operand + score + exp + lse (+ u for the scale) of Pm_ij |dO_id|.
lse (have_lse = 0) is held to the ABSOLUTE bound 2 el_i, as R.check_lse does; Drow to 2 * 10 u AD_i.

Checker.  One NaN-filled buffer holds dQh, dKh, dVh, dS, lse, Drow with GUARD floats before, between and after (layout()); check() asserts every element
inside the extents finite and within its bound, every guard element still NaN, nothing skipped or sampled; with have_lse = 1 the lse extent must still hold the
input bit for bit.

Not covered: the forms reachable only through the environment switches PK_ATTN_BWD_PACK=0 (short self-attention unpacked) and PK_ATTN_BWD_SPLIT=0 (split-bf16
asked for, f32 products run), read once per process; the prep kernels (tests/test_train_glue_gpu.py); head widths other than 64."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests import attn_fwd_reference as R

NEG_MAX, MASS = R.NEG_MAX, R.MASS
U_F32, U_BF16, U_SPLIT = R.U_F32, R.U_BF16, R.U_SPLIT
FORMS = (0, 1, 2)
FORM_NAME = {0: 'f32', 1: 'x3', 2: 'bf16'}
SLACK, GUARD = 8, 64
TINY = 2.0 ** -126
SEED, OFFSET = 0x5eed0123456789, 12
XR = 24 * math.log(2)
PLANTED_DS_FACTOR, PLANTED_DS_SHARE = 4.0, 0.75


# ------------------------------------------------------------------------------------------------ cases

def _case(name, S, h, n, n_kv=None, *, nnull=0, bias=None, mask=None, causal=False, drop=None, o_bf16=False, work=True, general2=False):
    """bias: None | 'dS' (the gradient is wanted) | 'nodS'; mask: None | 'mask' | 'full' (the last sequence fully masked) | 'first2' (the first two real keys);
    drop: None | the keep threshold (1 .. 255, p_eff = thr / 256); work=False: the C entry point with work = NULL; general2: X3 = 2 on f32 operands"""
    n_kv = n if n_kv is None else n_kv
    assert bias in (None, 'dS', 'nodS') and mask in (None, 'mask', 'full', 'first2') and (not causal or n == n_kv)
    return SimpleNamespace(name=name, S=S, h=h, n=n, nq=n, n_kv=n_kv, nnull=nnull, bias=bias, mask=mask, causal=causal, drop=drop, o_bf16=o_bf16, work=work,
                           general2=general2, dS=bias == 'dS')


def kv_split_of(S, h, n, nkt):
    """(G, chunk) of kv_split_of in attn_train.hip: the 32-row query tiles of a key tile dealt to G workgroups, `chunk` tiles each"""
    ntl, nqt = -(-nkt // 64), -(-n // 32)
    G = 768 // max(S * h * ntl, 1)
    if G < 2 or nqt < 2:
        return 1, nqt
    G = min(G, nqt)
    chunk = -(-nqt // G)
    return -(-nqt // chunk), chunk


def work_floats(c):
    """pk_attn_bwd_work"""
    G, _ = kv_split_of(c.S, c.h, c.n, c.nnull + c.n_kv)
    return 2 * G * c.S * c.h * (c.nnull + c.n_kv) * 64 if G > 1 else 0


def ds_store_form(c):
    """the store forms kernel Q takes for the 4-key groups of a dS row: 'vector' (16 bytes), 'scalar', or both where a leading group lies on the null keys"""
    if not c.dS:
        return None
    nkt, nreal = c.nnull + c.n_kv, c.n_kv
    forms = set()
    for j in range(0, nkt, 4):
        jr = j - c.nnull                                    # a group of null keys only (jr + 3 < 0) takes the scalar form and stores nothing
        forms.add('vector' if (jr >= 0 and j + 3 < nkt and nreal % 4 == 0 and jr % 4 == 0) else 'scalar')
    return '+'.join(sorted(forms))


def branch_of(c, X3, have_lse):
    """host mirror of pk_attn_bwd_ws's dispatch (no environment switch set)"""
    packed = c.drop is None and c.nnull == 0 and c.n == c.n_kv and c.n <= 32 and not c.dS
    G, chunk = (1, -(-c.n // 32))
    if c.work and not packed:
        G, chunk = kv_split_of(c.S, c.h, c.n, c.nnull + c.n_kv)
    drop = int(c.drop is not None)
    return dict(packed=packed, pack_g=64 // c.n if packed else 0, G=G, chunk=chunk, X3=X3, DROP=drop, have_lse=have_lse, dS_store=ds_store_form(c),
                kernels=f'attn_bwd_q_kernel<{X3},{drop}> + attn_bwd_kv_kernel<{X3},{drop}>')


def _cases():
    out = []
    add = lambda *a, **k: out.append(_case(*a, **k))
    # kernel tiles: 64 query rows x 64 keys (kernel Q), 64 keys x 32 query rows (kernel KV)
    for n in (33, 63, 64, 65, 130):
        add(f'plain_n{n}', 2, 3, n)
    add('bias_dS_n64', 2, 3, 64, bias='dS')                               # exact tile, 16-byte dS stores
    add('bias_dS_n65', 2, 3, 65, bias='dS')                               # ragged, scalar stores
    add('bias_nodS_n64', 2, 3, 64, bias='nodS')
    add('bias_nodS_n63', 2, 3, 63, bias='nodS')
    add('mask_n64', 2, 3, 64, mask='mask')
    add('mask_n130', 2, 2, 130, mask='mask')
    add('null2_n62', 2, 3, 62, nnull=2)                                   # nkt = 64
    add('null2_n63', 2, 3, 63, nnull=2)
    add('null2_mask_bias_n62', 2, 3, 62, nnull=2, mask='mask', bias='dS')  # dS stores with jr & 3 != 0
    add('null2_mask_bias_n33', 2, 3, 33, nnull=2, mask='mask', bias='dS')
    add('causal_n64', 2, 3, 64, causal=True)
    add('causal_n65', 2, 3, 65, causal=True)
    add('causal_null2_n62', 2, 3, 62, causal=True, nnull=2)
    add('causal_null2_n130', 2, 2, 130, causal=True, nnull=2)
    add('dS_null4_n36', 2, 3, 36, nnull=4, bias='dS')                     # a leading dS group with jr < 0, then 16-byte stores
    # cross-attention
    add('cross_q65_k14_null2_mask', 2, 3, 65, 14, nnull=2, mask='mask')
    add('cross_q65_k62_null2', 2, 3, 65, 62, nnull=2)                     # exactly one key tile
    add('cross_q65_k63_null2_mask_bias', 2, 3, 65, 63, nnull=2, mask='mask', bias='dS')        # one key into the second tile
    add('cross_q40_k129_bias_nodS', 2, 3, 40, 129, bias='nodS')
    add('cross_q1_k70_mask', 2, 3, 1, 70, mask='mask')
    add('cross_q70_k1', 2, 3, 70, 1)
    # kv_split (G is capped at nqt in every small case above: chunk = 1)
    add('split_even_q192', 128, 2, 192, 12, nnull=2, mask='mask')         # 768 // 256 = 3 workgroups x 2 tiles
    add('split_short_q160', 128, 2, 160, 12, nnull=2)                     # 5 tiles: 2 + 2 + 1
    add('split_tail_q150', 128, 2, 150, 14)                               # the short last chunk ends in a ragged tile
    add('g1_product_n40', 129, 3, 40)                                     # 768 // 387 < 2
    add('g1_nowork_n65', 2, 3, 65, work=False)
    # packed: n <= 32, nnull = 0, n = n_kv, no dS, no site; S h is no multiple of 64 // n
    for n, S, h in ((1, 23, 3), (9, 3, 3), (21, 2, 2), (31, 3, 3), (32, 3, 3)):
        add(f'packed_n{n}_plain', S, h, n)
    add('packed_n1_causal', 23, 3, 1, causal=True)
    add('packed_n9_causal', 3, 3, 9, causal=True)
    add('packed_n32_causal', 3, 3, 32, causal=True)
    add('packed_n21_mask', 2, 2, 21, mask='mask')
    add('packed_n31_mask', 3, 3, 31, mask='mask')
    add('packed_n9_bias_nodS', 3, 3, 9, bias='nodS')
    add('packed_n32_bias_nodS', 3, 3, 32, bias='nodS')
    add('unpacked_n21_dS', 2, 2, 21, bias='dS')
    add('unpacked_n21_null2', 2, 2, 21, nnull=2)
    add('unpacked_n21_site', 2, 2, 21, drop=64)
    # fully masked rows
    add('full_n65_bias_dS', 2, 3, 65, mask='full', bias='dS')
    add('full_packed_n21', 2, 2, 21, mask='full')
    add('first2_causal_n65_bias_dS', 2, 3, 65, mask='first2', causal=True, bias='dS')
    add('first2_causal_packed_n9', 3, 3, 9, mask='first2', causal=True)
    add('first2_causal_null2_n63_bias_dS', 2, 3, 63, mask='first2', causal=True, nnull=2, bias='dS')    # the control: no row is fully masked
    # dropout site (DROP = true): p = 0.25 and the two ends of the legal threshold range
    add('drop_plain_n65', 2, 3, 65, drop=64)
    add('drop_cross_q65_k14_null2_mask', 2, 3, 65, 14, nnull=2, mask='mask', drop=64)
    add('drop_causal_n64', 2, 3, 64, causal=True, drop=64)
    add('drop_bias_dS_n33', 2, 3, 33, bias='dS', drop=64)
    add('drop_split_n130', 2, 2, 130, drop=64)
    add('drop_thr1_n65', 2, 3, 65, drop=1)
    add('drop_thr255_n65', 2, 3, 65, drop=255)
    # bf16 O
    add('obf16_plain_n65', 2, 3, 65, o_bf16=True)
    add('obf16_packed_n9', 3, 3, 9, o_bf16=True)
    add('obf16_site_n65', 2, 3, 65, o_bf16=True, drop=64)
    add('general2_n65', 2, 3, 65, general2=True)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
DETERMINISM = ('plain_n130', 'packed_n9_plain')          # kv_split > 1 with slab summation, and the packed layout


def runs_of(c):
    """(X3, have_lse) of every launch of a case: a dropout forward always hands its lse over"""
    return [(X3, hl) for X3 in FORMS for hl in ((1,) if c.drop is not None else (0, 1))]


def rep_of(c, X3):
    """bf16-representable operands: X3 = 2, except in the one case that keeps general ones"""
    return X3 == 2 and not c.general2


# ------------------------------------------------------------------------------------------------ inputs

def fully_masked_rows(masked):
    return masked.all(-1)


def _packable(c):
    return c.nnull == 0 and c.n == c.n_kv and c.n <= 32


def build(c, rep=False):
    """the seeded inputs of a case: Q (P, n, 64), K, V (P, nkt, 64), dO (P, n, 64) as f32 values, bias (h, n, n_kv), kmask (S, n_kv) bool, slopes (h,), the
    keep mask (P, n, nkt) and survivor scale, O (P, n, 64): the f64 value of the stored forward output, lse32: the lse handed over, and the planting record"""
    g = R._gen(c.name + ('/rep' if rep else ''))
    rt = (lambda t: t.to(torch.bfloat16).to(torch.float32)) if rep else (lambda t: t.to(torch.float32))
    P, nk, n = c.S * c.h, c.nnull + c.n_kv, c.n
    x = SimpleNamespace(bias=None, kmask=None, slopes=None, rep=rep)
    if c.bias is not None:
        x.bias = (torch.randn(c.h, n, c.n_kv, generator=g) * 0.5).contiguous()
    if c.mask is not None:
        km = torch.rand(c.S, c.n_kv, generator=g) < 0.75
        km[:, -1] = True
        km[:, 0] = False
        if c.mask == 'full':
            assert c.S >= 2
            km[-1] = False
        if c.mask == 'first2':
            km[:] = True
            km[:, :2] = False
        x.kmask = km
    if c.causal:
        x.slopes = (2.0 ** -(6 + torch.arange(c.h))).float()
    D = 64 - R.NOFF
    K = torch.zeros(P, nk, 64)
    Kr = torch.randn(P, nk, D, generator=g) * 0.35
    if _packable(c):                                        # one key set for all pairs, up to noise: a leak into the next group finds this row's targets
        Kr = Kr[:1] + 0.02 * torch.randn(P, nk, D, generator=g)
    K[:, :, :D] = rt(Kr)
    K[:, :, D:] = 0.5
    V = rt(torch.randn(P, nk, 64, generator=g))
    dO = rt(torch.randn(P, n, 64, generator=g))
    noise = torch.randn(P, n, D, generator=g) * 0.1
    add, masked = R.structure(c, x)
    vis = ~masked
    targets = R._assign(vis, R.MAX_TARGETS)
    planted = targets | R._forbidden(c, x, masked)
    Kd = K[:, :, :D].double()
    U = Kd / (Kd * Kd).sum(-1, keepdim=True)
    zero = torch.zeros((), dtype=torch.float64)
    coef = torch.where(planted, R.G0 - add, zero)
    Q = torch.zeros(P, n, 64)
    Q[:, :, D:] = -R.GAMMA / (R.NOFF * 0.5)
    want = 0.9 / targets.sum(-1, keepdim=True).clamp_min(1)
    for _ in range(16):
        Q[:, :, :D] = rt((noise.double() + coef @ U).float())
        sim = Q.double() @ K.double().transpose(1, 2) + add
        prob = torch.where(masked, torch.full_like(sim, NEG_MAX), sim).softmax(-1)
        if not (targets & (prob < MASS + 0.02)).any():
            break
        coef = coef + torch.where(targets, 0.8 * (want / prob.clamp_min(1e-30)).log().clamp(-2, 2), zero)
        coef = coef - torch.where(vis & ~targets & (prob > 0.03), 0.8 * (prob / 0.01).log().clamp(0, 2), zero)
    x.Q, x.K, x.V, x.dO, x.targets, x.vis = Q, K, V, dO, targets, vis
    x.keep, x.scale = torch.ones(P, n, nk, dtype=torch.float64), 1.0
    if c.drop is not None:
        from phenaki_pytorch_amd import dropout as DR
        p = c.drop / 256.0
        thr, _, x.scale = DR.quantize(p)
        assert thr == c.drop
        wide = torch.from_numpy(DR.keep_mask(SEED, OFFSET, P * n, nk + 4, p)).double().view(P, n, nk + 4)
        x.keep = wide[:, :, :nk].contiguous()                # the keep function does not depend on the column count
        assert torch.equal(x.keep, torch.from_numpy(DR.keep_mask(SEED, OFFSET, P * n, nk, p)).double().view(P, n, nk))
        x.keep_shift = wide[:, :, 4:].contiguous()
        m = min(n, nk)
        x.keep_T = x.keep.clone()
        x.keep_T[:, :m, :m] = x.keep[:, :m, :m].transpose(1, 2)
    f = forward(c, x)
    x.O_exact = f.O
    x.O = f.O.to(torch.bfloat16 if c.o_bf16 else torch.float32).double()
    x.lse32 = f.lse.float()
    return x


def forward(c, x):
    add, masked = R.structure(c, x)
    sim = x.Q.double() @ x.K.double().transpose(1, 2) + add
    sim = torch.where(masked, torch.full_like(sim, NEG_MAX), sim)
    return SimpleNamespace(O=(sim.softmax(-1) * x.keep * x.scale) @ x.V.double(), lse=torch.logsumexp(sim, dim=-1))


def merged(c, t, poison, dtype=torch.float32):
    """(P, n, 64) -> (buffer (S n, h 64 + SLACK) with poisoned slack columns, its (S n, h 64) view)"""
    buf = torch.full((c.S * c.n, c.h * 64 + SLACK), poison, dtype=dtype)
    buf[:, :c.h * 64] = R.to_rows(c, t.contiguous()).to(dtype)
    return buf, buf[:, :c.h * 64]


# ------------------------------------------------------------------------------------------------ reference

MUTANTS = ('admit_pad_key', 'drop_last_key', 'causal_off_by_one_late', 'causal_off_by_one_early', 'mask_ignored_one_key', 'mask_applied_to_null_key',
           'bias_on_null_key', 'alibi_skips_null_keys', 'no_D_term', 'D_from_undropped_O', 'drop_mask_transposed', 'drop_group_shifted',
           'drop_scale_missing_in_dV', 'kv_split_last_chunk_lost', 'kv_split_slab_twice', 'query_tail_lost', 'packed_leak', 'packed_tail_group',
           'packed_bias_head', 'full_mask_P_is_one', 'full_mask_dS_flows')
_STRUCT_MUTANT = {'causal_off_by_one_late': 'causal_diag_late', 'causal_off_by_one_early': 'causal_diag_early', 'mask_applied_to_null_key': 'mask_no_null_shift',
                  'bias_on_null_key': 'bias_col_null_shift', 'alibi_skips_null_keys': 'alibi_skips_null'}


def has_full_rows(c):
    return c.nnull == 0 and (c.mask == 'full' or (c.mask == 'first2' and c.causal))


def applies(m, c):
    nk = c.nnull + c.n_kv
    br = branch_of(c, 0, 1)
    drop = c.drop is not None
    sparse = drop and c.drop > 192                         # so few survivors that a lost tail row may have kept nothing: O = 0, D = 0, dS = 0 on it
    return {'admit_pad_key': nk % 64 != 0,
            'drop_last_key': True,
            'causal_off_by_one_late': c.causal and c.n >= 2, 'causal_off_by_one_early': c.causal and nk >= 2,
            'mask_ignored_one_key': c.mask is not None and nk >= 2,
            'mask_applied_to_null_key': c.mask is not None and c.nnull > 0,
            'bias_on_null_key': c.bias is not None and c.nnull > 0,
            'alibi_skips_null_keys': c.causal and c.nnull > 0,
            'no_D_term': nk >= 2,
            'D_from_undropped_O': drop, 'drop_mask_transposed': drop, 'drop_group_shifted': drop,
            'drop_scale_missing_in_dV': drop and c.drop >= 64,          # thr = 1: the scale 256 / 255 is within the bf16 form's bound
            'kv_split_last_chunk_lost': br['G'] > 1 and not sparse, 'kv_split_slab_twice': br['G'] > 1,
            'query_tail_lost': c.n % 32 != 0 and not sparse,
            'packed_leak': br['packed'] and c.S * c.h >= 2, 'packed_tail_group': br['packed'] and (c.S * c.h) % br['pack_g'] != 0,
            'packed_bias_head': br['packed'] and c.bias is not None,
            'full_mask_P_is_one': has_full_rows(c) and nk >= 2, 'full_mask_dS_flows': has_full_rows(c) and nk >= 2}[m]


def reference(c, x, mutant=None, exact_O=False):
    """-> dQ (P, n, 64), dK, dV (P, nkt, 64), dS (P, n, n_kv), lse, D (P, n) and what the bound needs; `mutant`: as a kernel with that bug would compute"""
    P, n, nk, h = c.S * c.h, c.n, c.nnull + c.n_kv, c.h
    Q, K, V, dO = x.Q.double(), x.K.double(), x.V.double(), x.dO.double()
    xs = x
    if mutant == 'mask_ignored_one_key':
        km = x.kmask.clone()
        for s in range(c.S):
            dead = (~km[s]).nonzero().flatten()
            km[s, dead[0]] = True
        xs = SimpleNamespace(**{**vars(x), 'kmask': km})
    add, masked = R.structure(c, xs, _STRUCT_MUTANT.get(mutant))
    br = branch_of(c, 0, 1)
    pp = torch.arange(P)
    if mutant == 'packed_bias_head':
        b = x.bias.double()
        add = add + b[(pp // h) % h] - b[pp % h]
    sim = Q @ K.transpose(1, 2) + add
    sim = torch.where(masked, torch.full_like(sim, NEG_MAX), sim)
    if mutant == 'drop_last_key':
        sim[:, :, -1] = -math.inf
    ext = 0
    if mutant == 'admit_pad_key':
        sim, ext = torch.cat((sim, torch.zeros_like(sim[:, :, :1])), dim=2), 1
    if mutant == 'packed_leak':                             # the next group of the same tile, scored without bias or mask
        nxt = torch.roll(K, -1, dims=0)
        leak = Q @ nxt.transpose(1, 2)
        alone = ((pp % br['pack_g']) == br['pack_g'] - 1) | (pp == P - 1)
        leak[alone] = -math.inf
        sim, ext = torch.cat((sim, leak), dim=2), nk
    lse = torch.logsumexp(sim, dim=-1)
    prob = sim.softmax(-1)
    if ext:
        prob = prob[:, :, :nk]
    full = fully_masked_rows(masked)
    if mutant == 'full_mask_P_is_one':
        prob = torch.where(full[:, :, None], torch.ones_like(prob), prob)
    keep = {'drop_mask_transposed': getattr(x, 'keep_T', None), 'drop_group_shifted': getattr(x, 'keep_shift', None)}.get(mutant, x.keep)
    Pm = prob * keep * x.scale
    dPk = (dO @ V.transpose(1, 2)) * keep * x.scale
    O = x.O_exact if exact_O else x.O
    if mutant == 'D_from_undropped_O':
        O = prob @ V
    D = (dO * O).sum(-1)
    dS = prob * dPk if mutant == 'no_D_term' else prob * (dPk - D[:, :, None])
    if mutant != 'full_mask_dS_flows':
        dS = torch.where(masked, torch.zeros_like(dS), dS)
    dQ = dS @ K
    rows = torch.ones(n, dtype=torch.bool)
    if mutant == 'kv_split_last_chunk_lost':
        rows[32 * br['chunk'] * (br['G'] - 1):] = False
    if mutant == 'query_tail_lost':
        rows[32 * (-(-n // 32) - 1):] = False
    dSr, Pmr = dS * rows[None, :, None], (Pm if mutant != 'drop_scale_missing_in_dV' else prob * keep) * rows[None, :, None]
    dK, dV = dSr.transpose(1, 2) @ Q, Pmr.transpose(1, 2) @ dO
    if mutant == 'kv_split_slab_twice':
        r = 32 * br['chunk']
        dK = dK + dS[:, :r].transpose(1, 2) @ Q[:, :r]
        dV = dV + Pm[:, :r].transpose(1, 2) @ dO[:, :r]
    if mutant == 'packed_tail_group':
        lost = pp >= (P // br['pack_g']) * br['pack_g']
        dQ, dK, dV = dQ.clone(), dK.clone(), dV.clone()
        dQ[lost], dK[lost], dV[lost] = 0, 0, 0
    return SimpleNamespace(dQ=dQ, dK=dK, dV=dV, dS=dS[:, :, c.nnull:].contiguous(), dS_all=dS, lse=lse, D=D, prob=prob, Pm=Pm, dPk=dPk, masked=masked, add=add,
                           full=full)


def autograd_reference(c, x):
    """the same gradients by torch autograd of a plain float64 attention: masked_fill, dense softmax, the keep mask and scale on the softmax.  D is implicit
    here, i.e. taken from the exact O: compare with reference(exact_O=True)"""
    P, n, nk = c.S * c.h, c.n, c.nnull + c.n_kv
    add, masked = R.structure(c, x)
    with torch.enable_grad():                               # other test modules switch grad mode off process-wide at import
        Q, K, V = (t.double().clone().requires_grad_() for t in (x.Q, x.K, x.V))
        pre = torch.zeros(P, n, nk, dtype=torch.float64, requires_grad=True)      # d loss / d pre = the score gradient in front of masked_fill
        sim = Q @ K.transpose(1, 2) + add + pre
        sim = sim.masked_fill(masked, NEG_MAX)
        attn = sim.softmax(dim=-1) * x.keep * x.scale
        out = attn @ V
        (out * x.dO.double()).sum().backward()
    return SimpleNamespace(dQ=Q.grad, dK=K.grad, dV=V.grad, dS=pre.grad[:, :, c.nnull:], O=out.detach())


def planted_property(c, x, ref, bnd2):
    """asserts the planted property (module docstring); bnd2: the dS bound (P, n, nkt) of the bf16 form"""
    t = x.targets
    low = (t & (ref.prob < MASS)).nonzero()
    assert low.numel() == 0, f'{c.name}: planted (pair, row, key) below {MASS} of the softmax: {low[:8].tolist()}'
    vis_any = x.vis.any(1)
    whole = c.n >= vis_any.sum(1)
    miss = (vis_any & whole[:, None] & ~t.any(1)).nonzero()
    assert miss.numel() == 0, f'{c.name}: visible keys of a pair with enough rows that no row is planted on: {miss[:8].tolist()}'
    nk = c.nnull + c.n_kv
    tail = torch.arange(nk) >= 64 * ((nk - 1) // 64)
    fits = c.n * R.MAX_TARGETS >= (vis_any & tail[None]).sum(1)
    miss = (vis_any & tail[None] & fits[:, None] & ~t.any(1)).nonzero()
    assert miss.numel() == 0, f'{c.name}: visible keys of the last key tile that no row is planted on: {miss[:8].tolist()}'
    union = vis_any.any(0) & ~t.any(1).any(0) & bool(c.n * R.MAX_TARGETS > (vis_any & tail[None]).sum(1).max())
    assert not union.any(), f'{c.name}: keys planted in no pair: {union.nonzero().flatten()[:8].tolist()}'
    many = t & (x.vis.sum(-1, keepdim=True) >= 2)
    if many.any() and (c.drop or 0) <= 128:                # beyond a drop rate of 1 / 2 most rows keep nothing: O = 0 and dS = -P D vanishes with it
        strong = (ref.dS_all.abs() >= PLANTED_DS_FACTOR * bnd2)[many].double().mean().item()
        assert strong >= PLANTED_DS_SHARE, f'{c.name}: only {strong:.2f} of the planted dS entries stand {PLANTED_DS_FACTOR} x above their bound'


# ------------------------------------------------------------------------------------------------ bound

def operand_terms(X3, rep):
    """(op2, opA): the relative error of a product of two tiles in the operand form, for the register / global tiles and for the LDS round trip of P / dS"""
    if X3 == 0:
        return 0.0, 0.0
    if X3 == 1:
        return 3 * U_SPLIT, 3 * U_SPLIT
    return (0.0, U_BF16) if rep else (2 * U_BF16, 2 * U_BF16)


def bound(c, x, ref, X3, have_lse):
    """-> namespace dQ, dK, dV, dS (P, n, n_kv), dS_all, lse, D: the per-element bounds, and terms: {output: {name: largest contribution}}"""
    n, nk = c.n, c.nnull + c.n_kv
    op2, opA = operand_terms(X3, x.rep)
    G = branch_of(c, X3, have_lse)['G']
    Q, K, V, dO = x.Q.double(), x.K.double(), x.V.double(), x.dO.double()
    u = U_F32
    mag = (Q.abs() @ K.abs().transpose(1, 2) + ref.add.abs()).amax(-1, keepdim=True)          # (P, n, 1)
    Adp = (dO.abs() @ V.abs().transpose(1, 2)) * x.keep * x.scale
    AD = (dO.abs() * x.O.abs()).sum(-1, keepdim=True)
    T = (ref.dPk - ref.D[:, :, None]).abs()
    full = ref.full[:, :, None]
    live = lambda v: torch.where(full, torch.full_like(mag, u / 4), v + torch.zeros_like(mag))      # a fully masked row: P = 1 / nkt, one rounding in all
    lse_abs = ref.lse.abs()[:, :, None]
    ntl = -(-nk // 64)
    el0 = (op2 + 67 * u) * mag + (3 + XR) * u + (nk + 3 * ntl + 15) * u + 2.0 ** -21 + 2.0 ** -23 * lse_abs
    el = 2.0 ** -23 * lse_abs if have_lse else el0
    rho = dict(operand=live(op2 * mag), score=live(67 * u * mag), exp=live(torch.full_like(mag, (3 + 2 * XR) * u)), lse=live(el))
    Pa = ref.prob
    ds = {k: Pa * v * T for k, v in rho.items()}
    ds['operand'] = ds['operand'] + Pa * op2 * Adp
    ds['dP'] = Pa * 65 * u * Adp
    ds['D'] = Pa * 10 * u * AD
    ds['round'] = Pa * 2 * u * T
    ds = {k: torch.where(ref.masked, torch.zeros_like(v), v) for k, v in ds.items()}                  # the gradient of a masked score is exactly 0
    dS_abs = ref.dS_all.abs()
    tq = {k: v @ K.abs() for k, v in ds.items()}
    tq['lds_operand'] = opA * (dS_abs @ K.abs())
    tq['accumulate'] = (nk + 3) * u * (dS_abs @ K.abs())
    tk = {k: v.transpose(1, 2) @ Q.abs() for k, v in ds.items()}
    tk['lds_operand'] = opA * (dS_abs.transpose(1, 2) @ Q.abs())
    tk['accumulate'] = (n + G + 3) * u * (dS_abs.transpose(1, 2) @ Q.abs())
    PmT = ref.Pm.transpose(1, 2)
    tv = {k: (ref.Pm * v).transpose(1, 2) @ dO.abs() for k, v in rho.items()}
    tv['lds_operand'] = opA * (PmT @ dO.abs())
    tv['accumulate'] = (n + G + 4) * u * (PmT @ dO.abs())
    tot = lambda d: 2 * sum(d.values()) + TINY
    big = lambda d: {k: v.max().item() for k, v in d.items()}
    dS_all = tot(ds)
    return SimpleNamespace(dQ=tot(tq), dK=tot(tk), dV=tot(tv), dS_all=dS_all, dS=dS_all[:, :, c.nnull:].contiguous(), lse=2 * el0.squeeze(-1),
                           D=2 * 10 * u * AD.squeeze(-1) + TINY, terms=dict(dQ=big(tq), dK=big(tk), dV=big(tv), dS=big(ds)))


def largest_term(bnd):
    return {out: max(t, key=t.get) for out, t in bnd.terms.items()}


# ------------------------------------------------------------------------------------------------ checker

def layout(c):
    """{name: (offset, shape)} of the outputs inside one buffer, GUARD floats before, between and after; -> (layout, total floats).  Offsets are multiples of 4
    floats (16 bytes)"""
    P, n, nk = c.S * c.h, c.n, c.nnull + c.n_kv
    shapes = dict(dQ=(P, n, 64), dK=(P, nk, 64), dV=(P, nk, 64), dS=(P, n, c.n_kv) if c.dS else (0,), lse=(P, n), D=(P, n))
    lay, off = {}, GUARD
    for k, s in shapes.items():
        lay[k] = (off, s)
        off += -(-math.prod(s) // 4) * 4 + GUARD
    return lay, off


def as_output(c, ref, lse32=None):
    """what kernels with exactly the reference's values would leave: the buffer of layout(), NaN everywhere else"""
    lay, total = layout(c)
    buf = torch.full((total,), float('nan'), dtype=torch.float32)
    for k, (off, s) in lay.items():
        if k == 'dS' and not c.dS:
            continue
        v = lse32 if (k == 'lse' and lse32 is not None) else getattr(ref, k)
        buf[off:off + v.numel()] = v.reshape(-1).float()
    return buf


def check(what, buf, c, ref, bnd, lse_in=None):
    """buf: the WHOLE buffer of layout(c) as the launch left it (NaN-filled before; with have_lse = 1 the lse extent holds lse_in).  Every element inside an
    extent finite and within its bound, every other element still NaN; lse_in must be untouched.  Returns {output: largest error / bound}"""
    buf = buf.detach().cpu()
    lay, total = layout(c)
    assert buf.dtype == torch.float32 and buf.numel() == total, f'{what}: a buffer of {buf.numel()} floats for a layout of {total}'
    inside = torch.zeros(total, dtype=torch.bool)
    worst = {}
    for k, (off, s) in lay.items():
        cnt = math.prod(s)
        inside[off:off + cnt] = True
        if cnt == 0:
            continue
        got = buf[off:off + cnt].view(s)
        if k == 'lse' and lse_in is not None:
            assert torch.equal(got.view(torch.int32), lse_in.view(s).view(torch.int32)), f'{what}: the lse handed over was written to'
            continue
        bad = ~torch.isfinite(got)
        assert not bad.any(), f'{what}: {int(bad.sum())} non-finite / unwritten elements of {k}, first at {bad.nonzero()[0].tolist()}'
        r, b = getattr(ref, k), getattr(bnd, k)
        ratio = (got.double() - r).abs() / b
        worst[k] = ratio.max().item()
        if worst[k] > 1:
            at = tuple(np.unravel_index(int(ratio.argmax()), s))
            raise AssertionError(f'{what}: {k}{list(at)} is {got[at].item():.6g}, reference {r[at].item():.6g}: error {abs(got[at].item() - r[at].item()):.3e} = '
                                 f'{worst[k]:.2f} x bound {b[at].item():.3e}; {int((ratio > 1).sum())} elements of {k} beyond their bound')
    guard = buf[~inside]
    assert torch.isnan(guard).all(), f'{what}: {int((~torch.isnan(guard)).sum())} writes into the guard bands around the outputs'
    return worst
