"""Guided sampling (`Phenaki.sample(cond_scale=[..], guidance_schedule=, negative_texts=, blend=)`, pk_guidance_mix, pk_critic_head_guided)
restated on the CPU.  The reference has one scalar scale and a null branch (phenaki_pytorch.py:149-161, :251-263); the formula below, from
the issue's "The math" section, is the specification of everything beyond that and this file is its executable form.

    cbar  = e_0                              if P == 1   (no multiply)
    cbar  = sum_k a[k,b] * e_k , k ascending if P > 1    (a[0,b] = 1 - sum_{k>=1} a[k,b])
    mixed = e_base + (cbar - e_base) * g[s,b]
    g[s,b] = cond_scale[b]                     without a schedule (the value itself)
    g[s,b] = 1 + (cond_scale[b] - 1) * m[s]    with a schedule m (float64, rounded once to f32)

  table            the (steps, P + 1, B) table in float64 and its f32 rounding;
  mix              the formula on tensors of any floating dtype (the kernels' references call it in float64);
  guidance_mix_ref / critic_head_guided_ref   pk_guidance_mix / pk_critic_head_guided in float64 on the same f32 inputs, with their bounds;
  guided_sample    the mask-predict loop with one oracle forward per branch (O.maskgit_forward / O.critic_forward on contexts padded as the
                   product pads them), the LOGITS mixed (the oracle's head is linear, so that is the mix of the trunk outputs), the rest of
                   the loop as O.sample_step; it fills a trace like O.sample's, plus the noisy logits.
"""
import contextlib
import math

import numpy as np
import torch

from oracle import phenaki_oracle as O
from oracle import weights
from tests.infill_restatement import double_oracle, oracle_noise, to_double

U24 = 2.0 ** -24


# --------------------------------------------------------------------------- the table and the mix

def multipliers(schedule, steps):
    if schedule is None:
        return None
    if isinstance(schedule, str):
        assert schedule == 'linear'
        return [(s + 1) / steps for s in range(steps)]
    assert len(schedule) == steps
    return [float(v) for v in schedule]


def table(cond_scale, steps, schedule=None, blend_weights=()):
    """(float64 table, its float32 rounding), both numpy (steps, P + 1, B): rows 0..P-1 = a[k, b], row P = g[s, b]"""
    cs = np.asarray(cond_scale, dtype=np.float64)
    B, P = cs.shape[0], len(blend_weights) + 1
    t = np.empty((steps, P + 1, B), dtype=np.float64)
    rest = np.zeros((B,), dtype=np.float64)
    for k, w in enumerate(blend_weights, start=1):
        t[:, k] = np.broadcast_to(np.asarray(w, dtype=np.float64), (B,))
        rest = rest + t[0, k]
    t[:, 0] = 1.0 - rest
    m = multipliers(schedule, steps)
    for s in range(steps):
        t[s, P] = cs if m is None else 1.0 + (cs - 1.0) * m[s]
    return t, t.astype(np.float32)


def mix(branches, base, a, g):
    """branches: P tensors (B, ...); base: tensor or None; a: (P, B) tensor; g: (B,) tensor or None -- the formula above, in the tensors' dtype"""
    shape = (-1,) + (1,) * (branches[0].ndim - 1)
    if len(branches) == 1:
        cbar = branches[0]
    else:
        cbar = branches[0] * a[0].reshape(shape)
        for k in range(1, len(branches)):
            cbar = cbar + branches[k] * a[k].reshape(shape)
    if base is None:
        return cbar
    return base + (cbar - base) * g.reshape(shape)


# --------------------------------------------------------------------------- the two kernels in float64

def _gather(x, nb, n_tot, n_prime, rows, nrows, branch):
    """the rows of branch `branch` that output rows 0..nrows-1 read: logical row lr = rows ? rows[r] : r -> (b, i) = (lr / n, lr % n + n_prime)"""
    n = n_tot - n_prime
    lr = torch.arange(nrows) if rows is None else torch.as_tensor(rows, dtype=torch.int64)
    b, i = lr // n, lr % n + n_prime
    return x[(branch * nb + b) * n_tot + i], b


def guidance_mix_ref(x, nb, n_tot, n_prime, rows, nrows, coef, P, has_base):
    """x ((P + has_base) nb n_tot, D) f32, coef ((P + 1) nb,) f32 -> (ref (nrows, D) float64, bound (nrows, D) float64).
    bound = (P + 2) 2^-23 (1 + |g|) (sum_k |a_k e_k| + |e_base|): at most 2 P + 2 roundings of relative 2^-24 each, every one on a quantity of
    magnitude <= (1 + |g|) (sum_k |a_k e_k| + |e_base|).  P == 1 does not multiply: a_0 = 1 whatever the table holds."""
    x = x.double()
    coef = coef.double().reshape(P + 1, nb)
    es, b = zip(*[_gather(x, nb, n_tot, n_prime, rows, nrows, k) for k in range(P)])
    b = b[0]
    a = coef[:P, b] if P > 1 else torch.ones((1, nrows), dtype=torch.float64)
    base = _gather(x, nb, n_tot, n_prime, rows, nrows, P)[0] if has_base else None
    g = coef[P, b] if has_base else torch.zeros((nrows,), dtype=torch.float64)
    ref = mix(list(es), base, a, g)
    mag = sum((a[k][:, None] * es[k]).abs() for k in range(P)) + (base.abs() if has_base else 0.)
    bound = (P + 2) * 2.0 ** -23 * (1 + g.abs())[:, None] * mag
    return ref, bound


def critic_head_guided_ref(x, w, bias, D, nb, n_tot, n_prime, coef, P, has_base, u=None, noise_mult=0.):
    """pk_critic_head_guided in float64: s_k = x_k . w + b per branch, mixed by `mix`, plus noise_mult (u - 0.5).  Returns (ref (nb, n), bound).

    The bound follows the kernel's summation tree.  A product x_i w_i is rounded once, then passes through: the pair add and the add of the two
    pairs (2), the lane's running sum (ceil(D / 256) adds), the 6 levels of the wave sum, the bias add (1): 10 + ceil(D / 256) roundings in
    all (fused multiply-adds only remove some).  The mix adds at most P roundings to a conditional term (its a_k multiply and the adds of the
    blend) and 2 more to every term (the difference and the final multiply-add), all on quantities of magnitude <= (1 + |g|) M, where
    M = sum_k |a_k| (sum_i |x_ki w_i| + |b|) + (sum_i |x_base,i w_i| + |b|).  With R = 12 + ceil(D / 256) + P:
        bound = R u / (1 - R u) (1 + |g|) M + 2^-23 |noise_mult (u - 0.5)|,    u = 2^-24,
    which for |a_k| <= 1 is below D 2^-24 (1 + |g|) sum_branches (sum_i |x_i w_i| + |b|) as soon as D >= 17 (R <= 17 for D <= 512)."""
    n = n_tot - n_prime
    nrows = nb * n
    x, w = x.double()[:, :D], w.double().reshape(-1)
    bv = 0. if bias is None else float(bias.double().reshape(-1)[0])
    coef = coef.double().reshape(P + 1, nb)
    xs, b = zip(*[_gather(x, nb, n_tot, n_prime, None, nrows, k) for k in range(P)])
    b = b[0]
    a = coef[:P, b] if P > 1 else torch.ones((1, nrows), dtype=torch.float64)
    s = [xk @ w + bv for xk in xs]
    mag = sum(a[k].abs() * ((xs[k] * w).abs().sum(-1) + abs(bv)) for k in range(P))
    base = None
    g = torch.zeros((nrows,), dtype=torch.float64)
    if has_base:
        xb = _gather(x, nb, n_tot, n_prime, None, nrows, P)[0]
        base = xb @ w + bv
        mag = mag + (xb * w).abs().sum(-1) + abs(bv)
        g = coef[P, b]
    ref = mix(s, base, a, g)
    R = 12 + math.ceil(D / 256) + P
    bound = R * U24 / (1 - R * U24) * (1 + g.abs()) * mag
    if u is not None:
        noise = noise_mult * (u.double().reshape(-1) - 0.5)
        ref = ref + noise
        bound = bound + 2.0 ** -23 * (noise.abs() + ref.abs())
    return ref.reshape(nb, n), bound.reshape(nb, n)


# --------------------------------------------------------------------------- the sampler

def pad_contexts(conds, negative):
    """conds: P contexts (B, L_k, d); negative: (B, L_n, d) or None.  Every context zero-padded to the longest length, text mask =
    any(ctx != 0) (padded rows: False); the null base is the first conditional context under an all-False mask (what O.maskgit_forward's
    null_cond=True does).  Returns [(ctx, mask)] of the P conditional branches and the (ctx, mask) of the base."""
    every = list(conds) + ([negative] if negative is not None else [])
    Lmax = max(c.shape[1] for c in every)

    def pad(c):
        out = torch.zeros((c.shape[0], Lmax, c.shape[2]), dtype=c.dtype)
        out[:, :c.shape[1]] = c
        return out, (out != 0).any(dim=-1)

    padded = [pad(c) for c in every]
    cond = padded[:len(conds)]
    base = padded[-1] if negative is not None else (cond[0][0], torch.zeros_like(cond[0][1]))
    return cond, base


def guided_sample(cv, cv_cfg, mg, mg_cfg, cr, cr_cfg, *, num_frames, contexts, blend_weights=(), negative=None, cond_scale, schedule=None,
                  steps, starting_temperature=0.9, noise_K=1., anneal='decay', noise_fn=None, trace=None, decode=True):
    """contexts: the P conditional contexts [texts, blend_1, ..] each (B, L_k, d); blend_weights: P - 1 entries (float or B floats);
    cond_scale: B floats.  Runs in the dtype of the state dicts (f32, or float64 after to_double + double_oracle); the table enters as its f32
    rounding, like the product's.  No priming.  Returns (video or None, final ids)."""
    fdt = mg['to_logits.weight'].dtype
    B = contexts[0].shape[0]
    P = len(contexts)
    assert len(blend_weights) == P - 1 and len(cond_scale) == B
    tab = torch.from_numpy(table(cond_scale, steps, schedule, blend_weights)[1]).to(fdt)
    cond, base = pad_contexts([c.to(fdt) for c in contexts], None if negative is None else negative.to(fdt))
    H, W = cv_cfg['image_size']
    ph, pw = cv_cfg['patch_size']
    pt = cv_cfg['temporal_patch_size']
    assert (num_frames - 1) % pt == 0
    patch_shape = (1 + (num_frames - 1) // pt, H // ph, W // pw)
    n = patch_shape[0] * patch_shape[1] * patch_shape[2]
    V = mask_id = mg_cfg['num_tokens']
    critic_text = cr is not None and (cr_cfg.get('self_critic') is not None or cr_cfg.get('has_cross_attn', False))
    ids = torch.full((B, n), mask_id)
    mask = torch.ones((B, n), dtype=torch.bool)
    scores = None
    ks = O.mask_schedule(n, steps)
    for step in range(steps):
        if step > 0 and scores is not None:
            idx = scores.topk(ks[step], dim=-1).indices
            mask = torch.zeros((B, n)).scatter(1, idx, 1).bool()
        ids = torch.where(mask, mask_id, ids)
        rec = dict(step=step, masked_ids=ids.clone(), mask=mask.clone())
        a, g = tab[step, :P], tab[step, P]
        fwd = lambda cm: O.maskgit_forward(mg, mg_cfg, ids, video_patch_shape=patch_shape, context=cm[0], text_mask=cm[1])
        logits = mix([fwd(cm) for cm in cond], fwd(base), a, g)
        til = steps - (step + 1)
        temperature = starting_temperature * (til / steps)
        u = noise_fn('gumbel', step, (B, n, V)).to(fdt)
        noisy = logits / max(temperature, 1e-10) + (-torch.log(-torch.log(u + 1e-10) + 1e-10))      # tests/util.gumbel_noisy
        pred = noisy.argmax(dim=-1)
        ids = torch.where(mask, pred, ids)
        rec.update(pred=pred, ids=ids.clone(), noisy=noisy, temperature=temperature)
        new_scores = None
        if step != steps - 1:
            if cr is not None:
                cfwd = lambda cm: O.critic_forward(cr, cr_cfg, ids, video_patch_shape=patch_shape, context=cm[0], text_mask=cm[1])
                sc = mix([cfwd(cm) for cm in cond], cfwd(base), a, g) if critic_text else cfwd(cond[0])
                mult = {'fixed': 1., 'decay': til / steps, 'increase': (step + 1) / steps}[anneal]
                new_scores = sc + noise_K * (noise_fn('critic', step, (B, n)).to(fdt) - 0.5) * mult
            else:
                p = logits.softmax(dim=-1).gather(2, pred[..., None]).squeeze(-1)
                new_scores = torch.where(mask, 1 - p, -1e4)
        rec['scores'] = scores = new_scores
        if trace is not None:
            trace.append(rec)
    video = O.cvivit_decode_ids(cv, cv_cfg, ids) if decode else None
    return video, ids


# --------------------------------------------------------------------------- the parity configurations of the issue (TINY, B = 2, 5 frames, 6 steps)

def _ctx(L, seed):
    from oracle.configs import TINY
    return weights.synthetic_context(2, L, TINY['maskgit']['dim_context'], seed=seed)


def config(name):
    """A: blend + negative + linear schedule, noise base 700.  B: negative only, per-sample scales, base 710."""
    texts, negative = _ctx(6, 2), _ctx(9, 4)
    if name == 'A':
        return dict(contexts=[texts, _ctx(4, 3)], blend_weights=[[0.25, 0.75]], negative=negative, cond_scale=[5., 2.5], schedule='linear', base=700)
    assert name == 'B'
    return dict(contexts=[texts], blend_weights=[], negative=negative, cond_scale=[5., 2.5], schedule=None, base=710)


def run_config(name, double=False, decode=False, base=None):
    from oracle.configs import TINY, oracle_cfgs, state_dicts
    c = config(name)
    cv_sd, mg_sd, cr_sd = state_dicts('tiny')
    cvc, mgc, crc = oracle_cfgs(TINY)
    conv = to_double if double else (lambda sd: sd)
    cast = (lambda t: t.double()) if double else (lambda t: t)
    trace = []
    with double_oracle() if double else contextlib.nullcontext():
        video, ids = guided_sample(conv(cv_sd), cvc, conv(mg_sd), mgc, conv(cr_sd), crc, num_frames=5, contexts=[cast(t) for t in c['contexts']],
                                   blend_weights=c['blend_weights'], negative=cast(c['negative']), cond_scale=c['cond_scale'], schedule=c['schedule'],
                                   steps=TINY['steps'], starting_temperature=0.9, noise_K=1., anneal='decay',
                                   noise_fn=oracle_noise(c['base'] if base is None else base), trace=trace, decode=decode)
    return trace, video, ids


def gaps(trace, steps):
    """(smallest top-2 gap of the noisy logits over masked positions / max |noisy|, smallest gap across a step's top-k boundary of the scores /
    max |scores|) of a trace: how far the run is from a tie that rounding could decide"""
    pred_gap, score_gap = math.inf, math.inf
    n = trace[0]['mask'].shape[1]
    ks = O.mask_schedule(n, steps)
    for rec in trace:
        noisy = rec['noisy']
        top2 = noisy.topk(2, dim=-1).values
        gap = (top2[..., 0] - top2[..., 1])[rec['mask']]
        pred_gap = min(pred_gap, (gap.min() / noisy.abs().max()).item())
        if rec['scores'] is not None:
            k = ks[rec['step'] + 1]                                 # these scores choose the k positions the NEXT step re-masks
            if k < n:
                s = rec['scores'].sort(dim=-1, descending=True).values
                score_gap = min(score_gap, ((s[:, k - 1] - s[:, k]).min() / rec['scores'].abs().max()).item())
    return pred_gap, score_gap
