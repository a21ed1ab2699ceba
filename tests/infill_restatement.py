"""Infilling (`Phenaki.sample(known_ids=, known_mask=)`, `Phenaki.infill`) restated on the CPU.  There is no reference for this feature: the
issue's "Semantics" section is the specification and this file is its executable form.

  topk_mask_keep   pk_topk_mask_keep in numpy float64: ranking among the FREE positions only (known ones excluded by index), ties to the lower
                   index, ragged offsets into the compact row list, -1e4 at every position of scores_next;
  infill_sample    the whole mask-predict loop with known tokens, assembled from oracle.phenaki_oracle's maskgit_cfg / critic_cfg /
                   gumbel_argmax / cvivit_decode_ids (the oracle itself is untouched); it runs in the dtype of the state dicts it is given
                   (f32, or float64 after `to_double`) and records per step masked_ids, mask, pred, ids, scores and the noisy logits;
  pixel_to_token_brute   the pixel -> token reduction of `infill`, one python loop per token.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import phenaki_oracle as O

SENTINEL = -77


def topk_mask_keep(scores, k, row_off, known, mask_id, ids, rows_out=None):
    """scores (B, n) or None (all equal); k, row_off (B,) ints; known (B, n) bool or None; ids (B, n) int64; rows_out 1-d int array or None.
    Returns dict(mask uint8 (B, n), ids, rows_out (copies with the kernel's writes applied), scores_next f32 (B, n) = -1e4)."""
    ids = np.array(ids, dtype=np.int64, copy=True)
    B, n = ids.shape
    sc = np.zeros((B, n), dtype=np.float64) if scores is None else np.asarray(scores, dtype=np.float64).reshape(B, n)
    kn = np.zeros((B, n), dtype=bool) if known is None else np.asarray(known).astype(bool).reshape(B, n)
    mask = np.zeros((B, n), dtype=np.uint8)
    rows = None if rows_out is None else np.array(rows_out, copy=True)
    for b in range(B):
        free = np.flatnonzero(~kn[b])
        # rank of a free position = number of free positions with a larger score, or an equal score and a lower index
        order = free[np.argsort(-sc[b, free], kind='stable')]
        sel = order[:max(int(k[b]), 0)]
        mask[b, sel] = 1
        ids[b, sel] = mask_id
        if rows is not None:
            rows[int(row_off[b]):int(row_off[b]) + len(sel)] = b * n + sel
    return dict(mask=mask, ids=ids, rows_out=rows, scores_next=np.full((B, n), -1e4, dtype=np.float32))


def schedule(free_counts, steps):
    """k_b(0) = F_b, k_b(s) = oracle mask_schedule(F_b, steps)[s]; exclusive prefix sums; totals"""
    ks, offs, totals = [], [], []
    for s in range(steps):
        row = [F if s == 0 else O.mask_schedule(F, steps)[s] for F in free_counts]
        ks.append(row)
        offs.append([sum(row[:b]) for b in range(len(row))])
        totals.append(sum(row))
    return ks, offs, totals


def to_double(sd):
    return None if sd is None else {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@contextlib.contextmanager
def double_oracle():
    """the oracle follows the dtype of its state dicts everywhere but in continuous_position_bias, which casts the relative positions to f32:
    inside this context that one function is replaced by the same lines in float64 (the oracle's file is untouched)"""
    def cpb64(sd, p, dims, nlayers=2):
        pos = [torch.arange(d) for d in dims]
        grid = torch.stack(torch.meshgrid(*pos, indexing='ij')).reshape(len(dims), -1).t()
        rel = grid[:, None, :] - grid[None, :, :]
        h = torch.sign(rel).double() * torch.log(rel.abs().double() + 1)
        for l in range(nlayers):
            h = F.leaky_relu(h @ sd[f'{p}net.{l}.0.weight'].t() + sd[f'{p}net.{l}.0.bias'], 0.1)
        return (h @ sd[f'{p}net.{nlayers}.weight'].t() + sd[f'{p}net.{nlayers}.bias']).permute(2, 0, 1)
    saved = O.continuous_position_bias
    O.continuous_position_bias = cpb64
    try:
        yield
    finally:
        O.continuous_position_bias = saved


def infill_sample(cv, cv_cfg, mg, mg_cfg, cr, cr_cfg, *, ids0, known, patch_shape, steps, context=None, cond_scale=3., starting_temperature=0.9,
                  noise_K=1., anneal='decay', noise_fn=None, trace=None, decode=True, force=None):
    """the loop of the issue's Semantics section.  ids0 (B, n) int64, known (B, n) bool.  force(step) -> (masked ids, mask) replaces a step's
    input (teacher forcing).  Returns (video or None, final ids)."""
    B, n = ids0.shape
    V = mask_id = mg_cfg['num_tokens']
    known = known.bool()
    free = ~known
    ks, offs, _ = schedule(free.sum(1).tolist(), steps)
    text_mask = None if context is None else (context != 0).any(dim=-1)
    fdt = mg['to_logits.weight'].dtype
    ids = torch.where(free, mask_id, ids0)                          # start
    mask = free.clone()
    scores = None
    for step in range(steps):
        if step > 0:
            r = topk_mask_keep(scores.numpy(), ks[step], offs[step], known.numpy(), mask_id, ids.numpy())
            mask, ids = torch.from_numpy(r['mask']).bool(), torch.from_numpy(r['ids'])
        if force is not None:
            ids, mask = force(step)
        rec = dict(step=step, masked_ids=ids.clone(), mask=mask.clone(), k=ks[step])
        logits = O.maskgit_cfg(mg, mg_cfg, ids, cond_scale=cond_scale, video_patch_shape=patch_shape, context=context, text_mask=text_mask)
        til = steps - (step + 1)
        temperature = starting_temperature * (til / steps)
        u = noise_fn('gumbel', step, (B, n, V)).to(fdt)
        g = -torch.log(-torch.log(u + 1e-10) + 1e-10)
        noisy = logits / max(temperature, 1e-10) + g
        pred = O.gumbel_argmax(logits, temperature, u)
        assert torch.equal(pred, noisy.argmax(-1))
        ids = torch.where(mask, pred, ids)
        rec.update(pred=pred, ids=ids.clone(), noisy=noisy, temperature=temperature)
        scores = None
        if step != steps - 1:
            if cr is not None:
                sc = O.critic_cfg(cr, cr_cfg, ids, cond_scale=cond_scale, video_patch_shape=patch_shape, context=context, text_mask=text_mask)
                mult = {'fixed': 1., 'decay': til / steps, 'increase': (step + 1) / steps}[anneal]
                scores = sc + noise_K * (noise_fn('critic', step, (B, n)).to(fdt) - 0.5) * mult
            else:
                p = logits.softmax(dim=-1).gather(2, pred[..., None]).squeeze(-1)
                scores = torch.where(mask, 1 - p, -1e4)
        rec['scores'] = scores
        if trace is not None:
            trace.append(rec)
    video = O.cvivit_decode_ids(cv, cv_cfg, ids) if decode else None
    return video, ids


def pixel_to_token_brute(pixel_mask, pt, ph, pw):
    """(b, F, H, W) bool -> (b, f, h, w) bool, token by token: frame 0 -> token frame 0; frames 1 + (t-1) pt .. t pt -> token frame t"""
    pm = np.asarray(pixel_mask).astype(bool)
    b, F, H, W = pm.shape
    f, h, w = 1 + (F - 1) // pt, H // ph, W // pw
    out = np.zeros((b, f, h, w), dtype=bool)
    for s in range(b):
        for t in range(f):
            frames = [0] if t == 0 else list(range(1 + (t - 1) * pt, t * pt + 1))
            for y in range(h):
                for x in range(w):
                    out[s, t, y, x] = any(pm[s, fr, y * ph:(y + 1) * ph, x * pw:(x + 1) * pw].any() for fr in frames)
    return torch.from_numpy(out)


# --------------------------------------------------------------------------- the TINY case of tests/test_infill_gpu.py

# Noise seed of the teacher-forced parity test.  Admissible because the f32 restatement and a float64 run of itself (teacher-forced with the f32
# run's inputs) pick the same token at every masked position of every step, with and without critic: f32_vs_f64_flips == 0, asserted on the CPU
# by tests/test_infill_host.py.
PARITY_SEED = 700
PARITY_STEPS = 4
PARITY_GRID = (3, 4, 4)


def oracle_noise(base):
    """the CPU twin of tests.util.noise_fn_cuda(base)"""
    from oracle import weights

    def fn(kind, step, shape):
        return weights.uniform_noise(tuple(shape), base + 2 * step + (1 if kind == 'critic' else 0))
    return fn


def parity_known():
    """B = 2, n = 48: sample 0 keeps token frame 0 (F = 32), sample 1 keeps a 2 x 2 block in every frame (F = 36)"""
    known = torch.zeros((2, *PARITY_GRID), dtype=torch.bool)
    known[0, 0] = True
    known[1, :, 1:3, 1:3] = True
    ids0 = (torch.arange(2 * 48) * 37 + 11) % 256
    return ids0.reshape(2, 48), known.reshape(2, 48)


def parity_case(with_critic):
    from oracle import weights
    from oracle.configs import TINY, oracle_cfgs, state_dicts
    cv_sd, mg_sd, cr_sd = state_dicts('tiny')
    cvc, mgc, crc = oracle_cfgs(TINY)
    ids0, known = parity_known()
    ctx = weights.synthetic_context(2, 6, TINY['maskgit']['dim_context'], seed=2)
    return dict(cv=cv_sd, cvc=cvc, mg=mg_sd, mgc=mgc, cr=cr_sd if with_critic else None, crc=crc, ids0=ids0, known=known, ctx=ctx)


def run_parity_case(c, seed, double=False, force=None, decode=False):
    conv = to_double if double else (lambda sd: sd)
    trace = []
    with double_oracle() if double else contextlib.nullcontext():
        video, ids = infill_sample(conv(c['cv']), c['cvc'], conv(c['mg']), c['mgc'], conv(c['cr']), c['crc'], ids0=c['ids0'], known=c['known'],
                                   patch_shape=PARITY_GRID, steps=PARITY_STEPS, context=c['ctx'].double() if double else c['ctx'], cond_scale=5.,
                                   noise_fn=oracle_noise(seed), trace=trace, decode=decode, force=force)
    return trace, video, ids


def f32_vs_f64_flips(c, seed):
    """masked positions at which the f32 restatement and its float64 twin, fed the f32 run's inputs step by step, predict another token"""
    t32, _, _ = run_parity_case(c, seed)
    t64, _, _ = run_parity_case(c, seed, double=True, force=lambda step: (t32[step]['masked_ids'], t32[step]['mask']))
    return sum(int(((a['pred'] != b['pred']) & a['mask']).sum()) for a, b in zip(t32, t64))
