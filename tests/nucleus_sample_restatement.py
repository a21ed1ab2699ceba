"""Float64 restatement of nucleus / min-p filtered sampling (csrc/filter_sample.hip: pk_logits_nucleus_sample; _lib.vocab_sample_nucleus;
Phenaki.sample(top_p=, min_p=)).  CPU only, own text; it builds on tests/filtered_sample_restatement.py (R) and tests/vocab_reference.py.
tests/test_nucleus_sample_host.py shows what it accepts and rejects, tests/test_nucleus_sample_gpu.py runs the kernel against it.

Semantics per row, l[v] the logit, T = max(temperature, 1e-10f), lmax the row maximum, w[v] = exp((l[v] - lmax) / T):
  top-k  S = {v : l[v] >= the k-th largest}; k == V: all columns
  top-p  cut_p = the largest row value c with w{v in S : l[v] >= c} >= top_p w(S): the smallest descending prefix of S that reaches the share
         top_p of S's own mass, exact ties at the cut all kept; top_p == 1: none
  min-p  v passes iff (l[v] - lmax) / T >= ln(min_p); min_p == 0: none
  kept   the intersection = {v : l[v] >= cut}, cut the smallest kept logit (-inf when no filter is active)
The draw is R's at k' = the kept count (the kept set is upward-closed and holds every tie at its cut: a nucleus draw is a top-k' draw); the score is
R.score_ref's, unchanged.

The device forms w in f32 (arg = (l - lmax) * (1.0f / T), __expf) and sums it as 2^40 fixed point, so its cut is held to a band, not to equality.
DELTA = 2^-15, derived and not tuned: the f32 arg carries at most four roundings (the subtraction, the reciprocal, the product, the exp's argument
scaling): relative error <= 2^-22; a share moves by that times the mass-weighted |arg|, which is H(p) - ln(Z / w_max) <= ln V <= 11.1; with one ulp
of v_exp_f32 and the truncation V 2^-40 a share moves by at most ~ 6e-6; DELTA leaves 5x headroom.  A CPU emulation of the arithmetic (numpy f32 exp,
2^40 fixed point; V in {8, 256, 1156, 65 536}, four data kinds, five temperatures down to 1e-10, four values of p) violated the exact conditions by
at most 8e-10.  With logits known only to within E the device's weights lie within e^{+-2E/T} of the float64 ones (E enters once on the logit and
once on the maximum): RHO = exp(4E/T) on a share.  The min-p band: surely kept at (l - lmax)/T >= ln(min_p) + eps, surely dropped at <= ln(min_p) -
eps, eps = 2^-20 (1 + |ln min_p|) + 2E/T: 4x the four f32 roundings.

check_nucleus(): c the reported cut, n the reported count.  c is the largest of the three filters' cuts, so for EVERY active filter c is not below
that filter's cut, and for at LEAST ONE c is not above it (that filter binds):
  c is a row value (within E of one);   #{l >= c + E} <= n <= #{l >= c - E}
  not below:  top-k  #{l > c + E} <= k - 1          top-p  share{l > c + E} / RHO < top_p + DELTA          min-p  (c - lmax)/T >= ln(min_p) - eps
  binds:      top-k  #{l >= c - E} >= k             top-p  share{l >= c - E} RHO >= top_p - DELTA          min-p  no column under c - E surely passes
share(A) = w(A) / w(S); with E > 0 and k < V the top-k set itself is known to within 2E and the two sides take w(S) at its two ends."""
import math

import numpy as np
import torch

from tests import filtered_sample_restatement as R
from tests import vocab_reference as VR

DELTA = 2.0 ** -15
T_MIN = VR.EPS32                   # the clamp, 1e-10f


def f32(x):
    """the value the kernel's float argument holds"""
    return float(np.float32(x))


def _weights(l64, T):
    T = max(f32(T), T_MIN)
    arg = (l64 - l64.max(-1, keepdim=True).values) / T
    return arg, torch.exp(arg)


def nucleus64(l64, T, k, top_p, min_p):
    """(cut (M,), kept count (M,)) of float64 logits (M, V), by sort and cumulative sum"""
    M, V = l64.shape
    top_p, min_p = f32(top_p), f32(min_p)                                                       # what the kernel's float arguments hold
    arg, w = _weights(l64, T)
    keep = torch.ones_like(l64, dtype=torch.bool)
    if k < V:
        keep &= R.select64(l64, k)[1]
    if top_p < 1:
        ls, order = l64.sort(-1, descending=True)
        ws = torch.where(keep.gather(-1, order), w.gather(-1, order), torch.zeros_like(w))       # S is a prefix of the descending order
        cs = ws.cumsum(-1)
        first = (cs >= top_p * cs[:, -1:]).int().argmax(-1)                                     # the first sorted position that reaches the target
        keep &= l64 >= ls.gather(-1, first[:, None])                                            # its value and every tie of it
    if min_p > 0:
        keep &= arg >= math.log(min_p)
    cut = torch.where(keep, l64, torch.full_like(l64, math.inf)).min(-1).values
    if k == V and top_p == 1 and min_p == 0:
        cut = torch.full_like(cut, -math.inf)
    return cut, keep.sum(-1)


def prefix_count64(l64, T, top_p):
    """the count a tie-breaking top-p would keep (k = V): the length of the shortest descending prefix that reaches top_p; the kept count exceeds it
    exactly where the cut falls inside a run of equal values"""
    _, w = _weights(l64, T)
    cs = w.gather(-1, l64.sort(-1, descending=True).indices).cumsum(-1)
    return (cs >= f32(top_p) * cs[:, -1:]).int().argmax(-1) + 1


def _eps(min_p, E, T):
    return 2.0 ** -20 * (1 + abs(math.log(min_p))) + 2 * E / T


def check_nucleus(l64, E, T, k, top_p, min_p, cut_out, kept_out, what='nucleus'):
    """the band check, every row; E >= 0 a float: the logit bound (0 for given logits).  Returns the float64 kept counts."""
    l64 = l64.detach().cpu().double()
    M, V = l64.shape
    c = cut_out.detach().cpu()
    n = kept_out.detach().cpu().long()
    assert c.dtype == torch.float32 and c.shape == (M,) and n.shape == (M,), f'{what}: outputs of the wrong shape or type'
    cut64, n64 = nucleus64(l64, T, k, top_p, min_p)
    if k == V and top_p == 1 and min_p == 0:
        assert (c == -math.inf).all() and (n == V).all(), f'{what}: no filter is active: cut = -inf and all V columns kept'
        return n64
    T, top_p, min_p = max(f32(T), T_MIN), f32(top_p), f32(min_p)
    c = c.double()[:, None]
    rho = math.exp(min(4 * E / T, 700.))
    arg, w = _weights(l64, T)
    near = (l64 - c).abs().min(-1).values
    bad = ~(near <= E)
    assert not bad.any(), f'{what}: the cut {c[bad][0].item()!r} of row {int(bad.nonzero()[0])} is no row value (nearest at {near[bad][0].item():.3e})'
    hi_set, lo_set = l64 > c + E, l64 >= c - E                                                  # surely above the cut; possibly kept
    n_hi, n_lo = (l64 >= c + E).sum(-1), lo_set.sum(-1)
    bad = ~((n_hi <= n) & (n <= n_lo))
    assert not bad.any(), (f'{what}: kept count {int(n[bad][0])} of row {int(bad.nonzero()[0])} outside [{int(n_hi[bad][0])}, {int(n_lo[bad][0])}] '
                           f'(float64: {int(n64[bad][0])}; {int(bad.sum())} rows)')
    # the mass of S at its two ends (E = 0 or k = V: one value)
    if k < V:
        ck = R.kth_largest(l64, k)[:, None]
        z_hi = torch.where(l64 >= ck - 2 * E, w, torch.zeros_like(w)).sum(-1)
        z_lo = torch.where(l64 >= ck + 2 * E, w, torch.zeros_like(w)).sum(-1).clamp_min(1.0)      # the maximum (w = 1) is always in S
    else:
        z_hi = z_lo = w.sum(-1)
    share_above = torch.where(hi_set, w, torch.zeros_like(w)).sum(-1) / z_hi / rho
    share_kept = torch.where(lo_set, w, torch.zeros_like(w)).sum(-1) / z_lo * rho
    ok = torch.ones(M, dtype=torch.bool)                                                       # c is not below any active filter's cut
    binds = torch.zeros(M, dtype=torch.bool)                                                   # c is not above some active filter's cut
    low = []
    if k < V:
        f = hi_set.sum(-1) <= k - 1
        ok &= f
        low.append(('top-k', f))
    binds |= n_lo >= k                                                                         # k = V: every column is kept
    if top_p < 1:
        f = share_above < top_p + DELTA
        ok &= f
        low.append(('top-p', f))
        binds |= share_kept >= top_p - DELTA
    if min_p > 0:
        eps, lp = _eps(min_p, E, T), math.log(min_p)
        f = (c[:, 0] - l64.max(-1).values) / T >= lp - eps
        ok &= f
        low.append(('min-p', f))
        under = l64 < c - E
        binds |= ~(under & (arg >= lp + eps)).any(-1)
    if not ok.all():
        m = int((~ok).nonzero()[0])
        which = [name for name, f in low if not f[m]]
        raise AssertionError(f'{what}: the cut {c[m, 0].item()!r} of row {m} is too low for {which}: it keeps {int(n[m])} columns, float64 keeps '
                             f'{int(n64[m])} at cut {cut64[m].item()!r} (share above the cut {share_above[m].item():.9f}; {int((~ok).sum())} rows)')
    if not binds.all():
        m = int((~binds).nonzero()[0])
        raise AssertionError(f'{what}: the cut {c[m, 0].item()!r} of row {m} is too high: no filter drops the columns under it; it keeps {int(n[m])} '
                             f'columns, float64 keeps {int(n64[m])} at cut {cut64[m].item()!r} (share kept {share_kept[m].item():.9f}; '
                             f'{int((~binds).sum())} rows)')
    return n64


def accept_draw(ref, kept_out, pred, what='pred', rows=None):
    """the draw of row m lies in R's accept set at k' = kept_out[m]; returns the number of checked rows whose accept set is not one column"""
    n = kept_out.detach().cpu().long().reshape(-1)
    sel = torch.ones_like(n, dtype=torch.bool) if rows is None else torch.as_tensor(rows).cpu().bool().reshape(-1)
    amb = 0
    for kk in n[sel].unique().tolist():
        amb += R.accept(ref, kk, pred, f'{what} (k\' = {kk})', rows=sel & (n == kk))
    return amb


# ------------------------------------------------------------------------------------------------ data

def designed_row(masses, V, T, tail=-1e30):
    """a row whose first columns carry the given masses at temperature T (logits T ln m) and whose other columns weigh nothing"""
    l = torch.full((V,), tail, dtype=torch.float64)
    l[:len(masses)] = T * torch.log(torch.tensor(masses, dtype=torch.float64))
    return l


DESIGNED = ((0.5, 0.3, 0.15, 0.05), ((0.45, 1), (0.6, 2), (0.9, 3), (0.97, 4)))       # the masses; (top_p, kept count)
DESIGNED_TIE = ((0.4, 0.2, 0.2, 0.2), 0.5, 4)                                          # the cut falls inside the run of ties: all four are kept

TOP_PS = (1e-6, 0.1, 0.5, 0.9, 0.999)
MIN_PS = (0., 0.05, 0.5)
TEMPERATURES = (1.0, 0.225, 0.)


def data_kinds():
    return R.SELECT_DATA + ('designed', 'constant')


def nucleus_data(kind, M, V, T):
    """(M, V) f32 rows: R.select_data's kinds, the designed rows (shuffled into the row, one set of masses per row) and a constant row"""
    if kind in R.SELECT_DATA:
        return R.select_data(kind, M, V)
    if kind == 'constant':
        return torch.full((M, V), 1.5)
    g = VR._gen(f'nucleus/designed/{M}/{V}')
    Td = f32(T) if T > 0 else 1.0                                                        # at T = 0 the row is its maximum alone, whatever the masses
    rows = []
    for m in range(M):
        masses = DESIGNED[0] if m % 2 == 0 else DESIGNED_TIE[0]
        rows.append(designed_row(masses, V, Td)[torch.randperm(V, generator=g)])
    return torch.stack(rows).float()


# ------------------------------------------------------------------------------------------------ the loop on the oracle (end-to-end margins)

E2E_TOP_P = 0.5
E2E_SEEDS = (500, 700)              # noise bases vetted by tests/test_nucleus_sample_host.py


def e2e_accept(l64, E, T, top_p, pred):
    """(rows,) bool: the drawn column v is not surely outside the nucleus: share64{l > l[v] + 2E} exp(-4E/T) < top_p + DELTA.  (The device's cut is
    within E of a logit it holds to within E.)  Vacuous as T -> 0: the greedy check covers that end."""
    T = max(f32(T), T_MIN)
    _, w = _weights(l64, T)
    lv = l64.gather(-1, pred.reshape(-1, 1).long())
    share = torch.where(l64 > lv + 2 * E, w, torch.zeros_like(w)).sum(-1) / w.sum(-1)
    return share * math.exp(-min(4 * E / T, 700.)) < top_p + DELTA


def oracle_nucleus_sample(O, mg_sd, mgc, cr_sd, crc, *, batch, n, patch_shape, context, steps, top_p, noise_fn, cond_scale=5., starting_temperature=0.9,
                          noise_K=1.):
    """R.oracle_filtered_sample with the nucleus (top_p None: no filter) in front of the gumbel arg-max; per step dict(masked_ids, mask, logits,
    temperature, pred, ids, ref, E)"""
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
        ref = R.e2e_ref(logits, T, U, V)
        kept = torch.ones_like(ref.l64, dtype=torch.bool)
        if top_p is not None:
            cut, _ = nucleus64(ref.l64, T, V, top_p, 0.)
            kept = ref.l64 >= cut[:, None]
        pred = torch.where(kept, ref.noisy, torch.full_like(ref.noisy, -math.inf)).argmax(-1).reshape(batch, n)
        ids = torch.where(mask, pred, ids)
        rec.update(logits=logits, temperature=T, pred=pred, ids=ids.clone(), ref=ref, E=float(ref.E.max()))
        if step != steps - 1:
            if cr_sd is not None:
                sc = O.critic_cfg(cr_sd, crc, ids, cond_scale=cond_scale, video_patch_shape=patch_shape, context=context, text_mask=tm)
                scores = sc + noise_K * (noise_fn('critic', step, (batch, n)) - 0.5) * (til / steps)
            else:
                p = logits.softmax(-1).gather(2, pred[..., None]).squeeze(-1)
                scores = torch.where(mask, 1 - p, torch.full_like(p, -1e4))
        out.append(rec)
    return out
