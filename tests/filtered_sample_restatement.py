"""Float64 restatement of top-k filtered sampling (csrc/filter_sample.hip: pk_logits_topk_sample; _lib.vocab_sample_filtered; Phenaki.sample(filter_thres=,
top_k=)).  CPU only, own text.  tests/test_filtered_sample_host.py shows what it accepts and rejects, tests/test_filtered_sample_gpu.py runs the kernels
against it.  The noise expressions, their bounds B, the logit bound E, the LOG_C constants and uniform24x4_np are those of tests/vocab_reference.py.

Semantics per row, l[v] the logit, k in [1, V]:
  cut   the k-th largest of l, counting multiplicity;  kept = {v : l[v] >= cut} as floats (-0.0 == +0.0): exact ties at the cut are ALL kept
  pred  argmax over kept v of noisy(l[v]); the first maximum wins
  score 1 - exp(l[pred] - logsumexp_v l[v]) over ALL V columns

With logits known only to within E (the GEMM of the slabbed head, or a trunk in another summation order) the device's cut is the k-th largest of values
within E of l64.  With lo = l64 - E and hi = l64 + E a column v is
  possibly kept  hi[v] >= the k-th largest of lo (fewer than k columns are surely above it: l64 + E >= cut64 - E_cut, made rigorous)
  surely kept    fewer than k OTHER columns w can be above it: #{w != v : hi[w] > lo[v]} <= k - 1
accept(): pred is possibly kept; its noisy value can reach the best surely-kept column's, noisy[pred] + B[pred] >= max over surely-kept s of
(noisy[s] - B[s]); and no surely-kept column of a LOWER index ties with it exactly in float64.  With exact inputs (E = 0, B from the noise alone) possibly
and surely kept coincide, and check_select() holds cut and the kept count to equality.
accept_counts(): per row the number of columns accept() would take; singleton_share() is the share of rows where that is one column.
score_ref(): the score and its bound: one rounded __expf per column against the row's exact maximum (no rescale), the any-order sum bound over V terms,
one division, one subtraction; E of the chosen and of the largest logit enter relatively."""
import math
from types import SimpleNamespace as NS

import torch

from tests import vocab_reference as VR
from tests.gemm_reference import U1, U24
from tests.train_glue_reference import sum_bound

PARITY, FAST, NONE = VR.PARITY, VR.FAST, VR.NONE


def k_of(thres, V):
    """the k of a filter threshold, as the reference's helper evaluates it (in Python floats)"""
    return max(int((1 - thres) * V), 1)


def kth_largest(l, k):
    return l.sort(-1, descending=True).values[..., k - 1]


def select64(l, k):
    """(cut (...,), kept mask (..., V)) of float64 logits; == on floats: -0.0 and +0.0 are one value"""
    cut = kth_largest(l, k)
    return cut, l >= cut[..., None]


def noisy_ref(l64, E, mode, T, *, U=None, seed=0, seed_dev=None, rows=None):
    """vocab_reference.reference on given logits: NS(l64, E, noisy, B), each (M, V).  rows: the logical row of each of the M rows (FAST: noise index)"""
    M, V = l64.shape
    c = NS(noise=mode, T=T, seed=seed, seed_dev=seed_dev, V=V, M=M)
    x = NS(l64=l64, E=E, U=U, rows=None if rows is None else torch.as_tensor(rows))
    return VR.reference(c, x)


def bands(ref, k):
    """(possibly kept, surely kept) masks (M, V)"""
    lo, hi = ref.l64 - ref.E, ref.l64 + ref.E
    poss = hi >= kth_largest(lo, k)[:, None]                                    # fewer than k columns are surely above it
    hs = hi.sort(-1).values
    above = hi.shape[-1] - torch.searchsorted(hs, lo.contiguous(), right=True)  # columns w with hi[w] > lo[v], v itself among them where E[v] > 0
    return poss, above - (hi > lo).long() <= k - 1


def _floor(ref, sure):
    """per row: what the winner's noisy value plus its bound must reach: the best surely-kept column's lower end.  Where the bound leaves no column
    surely kept (k = 1 with the two largest logits within 2 E), the device still keeps ITS largest logit, one of the columns whose hi reaches the
    largest lo: the least lower end among those"""
    nb = ref.noisy - ref.B
    lo, hi = ref.l64 - ref.E, ref.l64 + ref.E
    top = hi >= lo.max(-1, keepdim=True).values
    weakest_top = torch.where(top, nb, torch.full_like(nb, math.inf)).min(-1).values
    best_sure = torch.where(sure, nb, torch.full_like(nb, -math.inf)).max(-1).values
    return torch.maximum(best_sure, weakest_top)


def accept_mask(ref, k):
    poss, sure = bands(ref, k)
    return poss & (ref.noisy + ref.B >= _floor(ref, sure)[:, None])


def accept_counts(ref, k):
    return accept_mask(ref, k).sum(-1)


def singleton_share(ref, k, rows=None):
    cnt = accept_counts(ref, k)
    if rows is not None:
        cnt = cnt[rows]
    return float((cnt == 1).double().mean()) if cnt.numel() else 1.0


def accept(ref, k, pred, what='pred', rows=None):
    """every pred[m] (rows: bool (M,) of the rows that are checked) is acceptable; returns the number of checked rows whose accept set is not one column"""
    pred = torch.as_tensor(pred).detach().cpu().long().reshape(-1)
    M, V = ref.l64.shape
    assert pred.shape == (M,), f'{what}: {tuple(pred.shape)} predictions for {M} rows'
    sel = torch.ones(M, dtype=torch.bool) if rows is None else torch.as_tensor(rows).cpu().bool().reshape(-1)
    bad = sel & ((pred < 0) | (pred >= V))
    assert not bad.any(), f'{what}: row {int(bad.nonzero()[0])} chose column {int(pred[bad][0])} outside [0, {V})'
    p = pred.clamp(0, V - 1)[:, None]
    poss, sure = bands(ref, k)
    bad = sel & ~poss.gather(-1, p)[:, 0]
    if bad.any():
        m = int(bad.nonzero()[0])
        raise AssertionError(f'{what}: row {m} chose column {int(pred[m])} with logit {ref.l64[m, pred[m]].item()!r}, which the top-{k} filter drops '
                             f'(cut {kth_largest(ref.l64[m], k).item()!r}, bound {ref.E[m, pred[m]].item():.3e}; {int(bad.sum())} rows)')
    n_at, B_at = ref.noisy.gather(-1, p)[:, 0], ref.B.gather(-1, p)[:, 0]
    floor = _floor(ref, sure)
    bad = sel & ~(n_at + B_at >= floor)
    if bad.any():
        m = int(bad.nonzero()[0])
        raise AssertionError(f'{what}: row {m} chose column {int(pred[m])} with reference value {n_at[m].item()!r} (+ {B_at[m].item():.3e}); a kept column '
                             f'reaches {floor[m].item()!r} ({int(bad.sum())} rows)')
    tie = sure & (ref.noisy == n_at[:, None])
    first = torch.where(tie.any(-1), tie.int().argmax(-1), pred)
    bad = sel & (first < pred)
    assert not bad.any(), f'{what}: row {int(bad.nonzero()[0])} chose a later one of exactly equal maxima ({int(bad.sum())} rows)'
    amb = sel & (accept_mask(ref, k).sum(-1) != 1)
    return int(amb.sum())


def check_select(l, k, cut_out, kept_out, what='select'):
    """exact logits: the device's cut is the k-th largest AS A FLOAT and its count is the count of columns >= cut"""
    l = l.detach().cpu()
    cut, kept = select64(l.double(), k)
    got = cut_out.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == cut.shape
    if k == l.shape[-1]:
        assert (got == -math.inf).all(), f'{what}: k = V must report cut = -inf'
        want_n = torch.full_like(kept.sum(-1), l.shape[-1])
    else:
        bad = got.double() != cut                                          # ==: a cut of -0.0 and one of +0.0 are the same value
        assert not bad.any(), f'{what}: cut of row {int(bad.nonzero()[0])} is {got[bad][0].item()!r}, the {k}-th largest is {cut[bad][0].item()!r}'
        want_n = kept.sum(-1)
    assert torch.equal(kept_out.detach().cpu().long(), want_n), (f'{what}: kept counts {kept_out.detach().cpu().tolist()[:6]} .. against '
                                                                  f'{want_n.tolist()[:6]} ..')
    return want_n


def score_ref(ref, pred):
    """(1 - p (M,), bound (M,)) of the unfiltered softmax at pred"""
    l, E = ref.l64, ref.E
    M, V = l.shape
    lmax = l.max(-1, keepdim=True).values
    Em = E.max(-1, keepdim=True).values
    xarg = l - lmax
    ex = torch.exp(xarg)
    s = ex.sum(-1)
    rel = E + Em + (VR.EXP_C + 3 * xarg.abs() + 2) * U24
    dsum = (ex * rel).sum(-1) + sum_bound(s, V)
    p = torch.as_tensor(pred).detach().cpu().long().reshape(-1, 1)
    xx = xarg.gather(-1, p)[:, 0]
    P = torch.exp(xx) / s
    relP = E.gather(-1, p)[:, 0] + Em[:, 0] + (VR.EXP_C + 3 * xx.abs() + 2) * U24 + dsum / s + 2 * U1
    sc = 1 - P
    return sc, P * relP + U1 * sc.abs()


# ------------------------------------------------------------------------------------------------ data of the exact-select tests

SELECT_SHAPES = ((1, 8), (3, 1000), (130, 1024), (5, 4100), (2, 65536))
SELECT_DATA = ('normal', 'negative', 'mixed', 'dyadic', 'zeros')


def select_ks(V):
    return sorted({1, 2, max(V // 10, 1), V - 1, V})


def select_data(kind, M, V):
    """(M, V) f32 rows.  normal; all negative; mixed sign with magnitudes 1e-30 .. 1e30 (the keys cross the sign boundary); a dyadic grid with
    heavy duplication (the cut falls inside a run of equal values: kept > k); rows holding +0.0 and -0.0 where the cut falls"""
    g = VR._gen(f'filtered/select/{kind}/{M}/{V}')
    if kind == 'normal':
        return torch.randn(M, V, generator=g) * 3
    if kind == 'negative':
        return -torch.rand(M, V, generator=g) * 50 - 1e-3
    if kind == 'mixed':
        mag = 10.0 ** (torch.rand(M, V, generator=g) * 60 - 30)
        return (mag * torch.where(torch.rand(M, V, generator=g) < 0.5, -1.0, 1.0)).float()
    if kind == 'dyadic':
        return torch.randint(-6, 7, (M, V), generator=g).float() / 4
    # zeros: a third of the row positive, a third negative, the rest +0.0 / -0.0 alternating: every k in the middle third cuts at zero
    x = torch.randn(M, V, generator=g)
    third = torch.rand(M, V, generator=g)
    z = torch.where(torch.arange(V)[None, :] % 2 == 0, torch.tensor(0.0), torch.tensor(-0.0)).expand(M, V)
    return torch.where(third < 1 / 3, x.abs() + 0.5, torch.where(third < 2 / 3, -x.abs() - 0.5, z)).contiguous()


# ------------------------------------------------------------------------------------------------ the loop on the oracle (end-to-end margins)

E2E_REL = 1e-4                      # the decision-margin tolerance of the f32-grade modes (tests/test_modules_gpu.py MODES): E = 1e-4 max|logits| per step
E2E_SEEDS = (500, 700)              # noise bases vetted by tests/test_filtered_sample_host.py
E2E_AMBIGUOUS_CAP = 0.02            # share of checked (step, position) pairs whose accept set is not one column: vocab_reference's 98 % singleton figure


def e2e_ref(logits, temperature, U, k):
    """a step's reference from the oracle's (B, n, V) logits and the injected uniforms: PARITY noise, E = E2E_REL max|logits|"""
    V = logits.shape[-1]
    l64 = logits.reshape(-1, V).double()
    E = torch.full_like(l64, E2E_REL * float(l64.abs().max()))
    return noisy_ref(l64, E, PARITY, temperature, U=U.reshape(-1, V))


def oracle_filtered_sample(O, mg_sd, mgc, cr_sd, crc, *, batch, n, patch_shape, context, steps, k, noise_fn, cond_scale=5., starting_temperature=0.9,
                           noise_K=1.):
    """the mask-predict loop on the oracle with the top-k filter in front of the gumbel arg-max; per step dict(masked_ids, mask, logits, temperature,
    pred, ids).  Scores: the critic's, or 1 - p of the UNFILTERED softmax."""
    V, mask_id = mgc['num_tokens'], mgc['num_tokens']
    tm = None if context is None else (context != 0).any(-1)
    ids = torch.full((batch, n), mask_id)
    mask = torch.ones((batch, n), dtype=torch.bool)
    scores, out = None, []
    ks = O.mask_schedule(n, steps)
    for step in range(steps):
        if step > 0:
            mask = torch.zeros((batch, n)).scatter(1, scores.topk(ks[step], dim=-1).indices, 1).bool()
        ids = torch.where(mask, mask_id, ids)
        rec = dict(masked_ids=ids.clone(), mask=mask.clone())
        logits = O.maskgit_cfg(mg_sd, mgc, ids, cond_scale=cond_scale, video_patch_shape=patch_shape, context=context, text_mask=tm)
        til = steps - (step + 1)
        T = starting_temperature * (til / steps)
        U = noise_fn('gumbel', step, (batch, n, V))
        ref = e2e_ref(logits, T, U, k)
        _, kept = select64(ref.l64, k)
        pred = torch.where(kept, ref.noisy, torch.full_like(ref.noisy, -math.inf)).argmax(-1).reshape(batch, n)
        ids = torch.where(mask, pred, ids)
        rec.update(logits=logits, temperature=T, pred=pred, ids=ids.clone(), ref=ref)
        if step != steps - 1:
            if cr_sd is not None:
                sc = O.critic_cfg(cr_sd, crc, ids, cond_scale=cond_scale, video_patch_shape=patch_shape, context=context, text_mask=tm)
                scores = sc + noise_K * (noise_fn('critic', step, (batch, n)) - 0.5) * (til / steps)
            else:
                p = logits.softmax(-1).gather(2, pred[..., None]).squeeze(-1)
                scores = torch.where(mask, 1 - p, torch.full_like(p, -1e4))
        out.append(rec)
    return out
