"""MaskGit / TokenCritic / SelfCritic / Phenaki / make_video with the reference's surfaces
(/root/reference/phenaki_pytorch/phenaki_pytorch.py:105-560, 691-714) on the MI355X kernels.

What changes relative to the reference's op sequence (results are the same up to f32 rounding):
  * cond and null passes of classifier-free guidance run as ONE batch of 2B sequences;
  * CFG is applied to the 512-d trunk output before the (linear) vocab head, so the 65 536-wide GEMM runs once;
  * the sampler never materialises logits: gumbel-argmax / softmax confidence live in the GEMM epilogue;
  * cross-attention K/V of the (step-invariant) text context and the position bias are computed once per sample();
  * the mask schedule k_s is data independent and precomputed on the host (no per-step .item() sync).
`Phenaki.forward` (phenaki_pytorch.py:562-687) returns the VALUE of the training objective (no autograd graph): masked-token
cross entropy without logits (pk_vocab_sample statistics + pk_vocab_ce) + the token-critic BCE.
"""
import math
from functools import partial
from collections import namedtuple
from typing import List

import torch
from torch import nn

from . import _lib as L
from .attention import (ContinuousPositionBias, PackedModule, Transformer, compute_dtype_of, exists, default, linear_weight,
                        param_fingerprint, set_compute_dtype)
from .cvivit import CViViT
from .t5 import t5_encode_text, get_encoded_dim, DEFAULT_T5_NAME


def cast_tuple(val, length=1):
    return val if isinstance(val, tuple) else (val,) * length


def eval_decorator(fn):
    def inner(model, *args, **kwargs):
        was_training = model.training
        model.eval()
        out = fn(model, *args, **kwargs)
        model.train(was_training)
        return out
    return inner


def uniform(shape, device):
    return torch.zeros(shape, device=device).float().uniform_(0, 1)


def prob_mask_like(shape, prob, device):
    if prob == 1:
        return torch.ones(shape, device=device, dtype=torch.bool)
    elif prob == 0:
        return torch.zeros(shape, device=device, dtype=torch.bool)
    return torch.zeros(shape, device=device).float().uniform_(0, 1) < prob


def default_text_mask(context, text_mask, device):
    """no text mask with a context means all True"""
    if exists(context) and not exists(text_mask):
        return torch.ones(context.shape[:2], device=device, dtype=torch.bool)
    return text_mask


def cond_drop_text_mask(context, text_mask, cond_drop_prob, b, device, *, needs_context):
    """the text mask of a forward call: the default one, then classifier-free-guidance dropout -- a prob_mask_like((b,), 1 - p) keep draw ANDed
    into it, drawn only when the guard below holds and p > 0."""
    # needs_context: False = MaskGit, which drops whenever a text mask exists (phenaki_pytorch.py:188-189); True = TokenCritic, only with a context (:286-287)
    text_mask = default_text_mask(context, text_mask, device)
    guard = exists(context) if needs_context else exists(text_mask)
    if guard and exists(cond_drop_prob) and cond_drop_prob > 0:
        text_mask = prob_mask_like((b,), 1 - cond_drop_prob, device=device)[:, None] & text_mask
    return text_mask


def critic_noise_multiplier(schedule, step, steps):
    """the critic's noise scale at `step` as a fraction of noise_K (phenaki_pytorch.py:533-540)"""
    multipliers = dict(fixed=1., decay=(steps - (step + 1)) / steps, increase=(step + 1) / steps)
    if schedule not in multipliers:
        raise ValueError('invalid critic noise anneal schedule name')
    return multipliers[schedule]


def mask_schedule(num_tokens, steps):
    """k_s = round(n * cos(pi/2 * s/steps)).clamp(1) in f32, s = 1..steps-1 (phenaki_pytorch.py:484-486), on the host."""
    ks = [None]
    for s in range(1, steps):
        time = torch.full((1,), s / steps)
        ks.append(int((num_tokens * torch.cos(time * math.pi * 0.5)).round().long().clamp(min=1).item()))
    return ks


def infill_schedule(free_counts, steps):
    """the per-sample schedule of an infilling sample(): with F_b free (regenerated) tokens in sample b, k_b(0) = F_b and
    k_b(s) = mask_schedule(F_b, steps)[s] for s >= 1 (<= F_b always: cos <= 1 and F_b >= 1).  Returns host lists (ks, offs, totals):
    ks[s][b], the exclusive prefix sums offs[s][b] = sum_{b' < b} ks[s][b'] (where sample b's rows start in the compact row list) and
    totals[s] = sum_b ks[s][b] (the rows the vocabulary head visits at step s)."""
    per_count = {F: mask_schedule(F, steps) for F in set(free_counts)}
    ks, offs, totals = [], [], []
    for s in range(steps):
        row = [F if s == 0 else per_count[F][s] for F in free_counts]
        off, acc = [], 0
        for k in row:
            off.append(acc)
            acc += k
        ks.append(row)
        offs.append(off)
        totals.append(acc)
    return ks, offs, totals


def pixel_to_token_mask(pixel_mask, temporal_patch_size, patch_size):
    """(b, F, H, W) bool pixel mask -> (b, f, h, w) bool token mask: a token is marked iff ANY pixel of its footprint is.  Token frame 0 is
    video frame 0; token frame t >= 1 covers video frames 1 + (t-1) pt .. t pt; spatially the footprint is the ph x pw patch."""
    ph, pw = patch_size
    pt = temporal_patch_size
    b, F, H, W = pixel_mask.shape
    sp = pixel_mask.reshape(b, F, H // ph, ph, W // pw, pw).any(dim=5).any(dim=3)
    rest = sp[:, 1:].reshape(b, (F - 1) // pt, pt, H // ph, W // pw).any(dim=2)
    return torch.cat((sp[:, :1], rest), dim=1)


def token_to_pixel_mask(token_mask, temporal_patch_size, patch_size):
    """(b, f, h, w) bool token mask -> (b, F, H, W) bool: every token's footprint (the inverse layout of pixel_to_token_mask)"""
    ph, pw = patch_size
    sp = token_mask.repeat_interleave(ph, dim=2).repeat_interleave(pw, dim=3)
    return torch.cat((sp[:, :1], sp[:, 1:].repeat_interleave(temporal_patch_size, dim=1)), dim=1)


def _check_known(known_ids, known_mask, B, patch_shape, V, device):
    """validate sample()'s known_ids / known_mask (ValueError) and lay them out: ids (B, n) int64 and known (B, n) uint8, contiguous on
    `device`, plus the host list of free counts F_b -- read with the ONE host synchronisation of an infilling call (the range check of the
    known ids rides on the same transfer)."""
    n = patch_shape[0] * patch_shape[1] * patch_shape[2]
    if not (torch.is_tensor(known_ids) and torch.is_tensor(known_mask)):
        raise ValueError('sample: known_ids and known_mask must be tensors')
    if known_ids.dtype != torch.int64:
        raise ValueError(f'sample: known_ids must be int64 token ids, got {known_ids.dtype}')
    if known_mask.dtype != torch.bool:
        raise ValueError(f'sample: known_mask must be bool (True = keep the token), got {known_mask.dtype}')
    grid = tuple(patch_shape)
    if tuple(known_ids.shape) not in ((B, *grid), (B, n)):
        raise ValueError(f'sample: known_ids must be {(B, *grid)} or {(B, n)}, got {tuple(known_ids.shape)}')
    if tuple(known_mask.shape) not in ((B, *grid), (B, n), grid, (n,)):
        raise ValueError(f'sample: known_mask must be {(B, *grid)}, {(B, n)}, {grid} or {(n,)}, got {tuple(known_mask.shape)}')
    ids = known_ids.to(device).reshape(B, n).contiguous()
    known = known_mask.to(device)
    known = known.reshape(1, n).expand(B, n) if known.ndim in (1, 3) else known.reshape(B, n)
    bad = (known & ((ids < 0) | (ids >= V))).sum().reshape(1)
    *free, nbad = torch.cat(((~known).sum(dim=1), bad)).tolist()
    if nbad:
        raise ValueError(f'sample: {nbad} known token ids lie outside [0, {V})')
    if min(free) < 1:
        raise ValueError(f'sample: every sample needs at least one token to generate, free counts {free}')
    return ids, known.to(torch.uint8).contiguous(), free


def _u8(mask):
    if mask is None or (mask.dtype == torch.uint8 and mask.is_contiguous()):
        return mask
    return mask.to(torch.uint8).contiguous()


def _cfg_masks(text_mask, nb, with_null):
    """(nb, n_ctx) bool text mask -> uint8 mask for the S = 2 nb sequences of a CFG batch: [cond rows | all-False null rows]
    (cond_drop_prob = 1, phenaki_pytorch.py:188-190); prepared ONCE per sample() call, not per step."""
    if text_mask is None:
        return None
    tm = text_mask.to(torch.uint8)
    if not with_null:
        return tm.contiguous()
    return torch.cat((tm, torch.zeros_like(tm)), dim=0).contiguous()


# ---------------------------------------------------------------------------------------------- guided sampling: the table path
# For sample b, step s and P conditional branches (1 <= P <= 3) with trunk outputs e_0 .. e_{P-1} and a base branch e_base (the null branch,
# or the trunk on the negative prompt's context):
#     cbar  = e_0 (P == 1)  |  sum_k a[k, b] e_k, k ascending, a[0, b] = 1 - sum_{k >= 1} a[k, b]
#     mixed = e_base + (cbar - e_base) * g[s, b]
#     g[s, b] = cond_scale[b]  |  1 + (cond_scale[b] - 1) * m[s] with a schedule m (float64 on the host, rounded once to f32)
# (pk_guidance_mix on the trunk outputs, pk_critic_head_guided on the critic's scalar head outputs; DESIGN.md "Guided sampling").

GUIDANCE_MAX_BRANCHES = 3


def _is_scalar_scale(cond_scale):
    """a Python number (or 0-d tensor): today's scalar path; a sequence / 1-D tensor / array: the table path"""
    if torch.is_tensor(cond_scale):
        return cond_scale.ndim == 0
    return not (isinstance(cond_scale, (list, tuple)) or getattr(cond_scale, 'ndim', 0) > 0)


def _floats(x, length, what):
    """a number, or a sequence / 1-D tensor of `length` numbers -> list of `length` finite Python floats (ValueError otherwise)"""
    if _is_scalar_scale(x):
        vals = [float(x)] * length
    else:
        if getattr(x, 'ndim', 1) != 1:
            raise ValueError(f'{what} must be a number or a 1-D sequence of {length} numbers')
        vals = [float(v) for v in (x.tolist() if hasattr(x, 'tolist') else x)]
        if len(vals) != length:
            raise ValueError(f'{what} must hold {length} values, got {len(vals)}')
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f'{what} must be finite, got {vals}')
    return vals


def guidance_multipliers(guidance_schedule, steps):
    """None | 'linear' (m[s] = (s + 1) / steps) | a sequence of `steps` finite floats -> None or the list m"""
    if guidance_schedule is None:
        return None
    if isinstance(guidance_schedule, str):
        if guidance_schedule != 'linear':
            raise ValueError(f"guidance_schedule must be None, 'linear' or a sequence of {steps} floats, got {guidance_schedule!r}")
        return [(s + 1) / steps for s in range(steps)]
    if _is_scalar_scale(guidance_schedule):
        raise ValueError(f"guidance_schedule must be None, 'linear' or a sequence of {steps} floats, got {guidance_schedule!r}")
    return _floats(guidance_schedule, steps, f'guidance_schedule (one multiplier per step, steps = {steps})')


def guidance_table(cond_scale, steps, multipliers=None, weights=()):
    """the (steps, P + 1, B) float32 table of the table path, built in float64 and rounded once: rows 0..P-1 of a step hold the blend weights
    a[k, b] (a[0, b] = 1 - sum_{k >= 1} a[k, b]; 1 when P == 1), row P the guidance scale g[s, b].  cond_scale: B floats; multipliers: None or
    `steps` floats m[s]; weights: P - 1 lists of B floats (the blend branches, k = 1..P-1)."""
    B, P = len(cond_scale), len(weights) + 1
    t = torch.empty((steps, P + 1, B), dtype=torch.float64)
    a0 = torch.ones((B,), dtype=torch.float64)
    if P > 1:
        w = torch.tensor(weights, dtype=torch.float64).reshape(P - 1, B)
        t[:, 1:P] = w
        a0 = 1. - w.sum(dim=0)
    t[:, 0] = a0
    cs = torch.tensor(cond_scale, dtype=torch.float64)
    if multipliers is None:
        t[:, P] = cs                                                      # the value itself, no arithmetic
    else:
        t[:, P] = 1. + (cs[None, :] - 1.) * torch.tensor(multipliers, dtype=torch.float64)[:, None]
    return t.to(torch.float32)


def guidance_contexts(conds, base=None):
    """the contexts of the P conditional branches and the base branch as ONE batch: conds = [(context (B, L_k, d) f32, text mask (B, L_k) bool or
    None = all True)], base = the same pair for a negative prompt, or None = the null branch (the first conditional context under an all-False
    mask, as pk_cfg_mix's null half).  Every context is padded with zero rows to the longest length L; padded rows are masked out.
    Returns (ctx (J * B, L, d) f32, mask (J * B, L) uint8), J = P + 1, laid out [cond_0 | .. | cond_{P-1} | base]."""
    B, _, d = conds[0][0].shape
    device = conds[0][0].device
    branches = list(conds) + ([base] if base is not None else [])
    for j, (c, m) in enumerate(branches):
        if c.ndim != 3 or tuple(c.shape[::2]) != (B, d) or (m is not None and tuple(m.shape) != tuple(c.shape[:2])):
            raise ValueError(f'guidance: branch {j} context is {tuple(c.shape)}, expected ({B}, L, {d}) with a (B, L) text mask')
    Lmax = max(c.shape[1] for c, _ in branches)
    J = len(conds) + 1
    ctx = torch.zeros((J * B, Lmax, d), device=device, dtype=torch.float32)
    tm = torch.zeros((J * B, Lmax), device=device, dtype=torch.uint8)
    for j, (c, m) in enumerate(branches):
        ctx[j * B:(j + 1) * B, :c.shape[1]] = c
        tm[j * B:(j + 1) * B, :c.shape[1]] = 1 if m is None else m.to(torch.uint8)
    if base is None:
        ctx[(J - 1) * B:] = ctx[:B]
    return ctx, tm


class _TokenTrunk(PackedModule):
    """shared plumbing of MaskGit / TokenCritic: ids -> embeddings -> Transformer -> norm_out rows."""

    def _embed(self, ids2d, replicas=1, ids_prime=None):
        """ids2d (nb, n) [after ids_prime (nb, n_prime)] -> (replicas * nb * n_tot, D) f32: token + position embedding; the
        replicas (cond | null halves of a CFG batch) read the same id rows inside the kernel (no torch.cat)."""
        nb, n = ids2d.shape
        n_tot = n + (ids_prime.shape[-1] if ids_prime is not None else 0)
        S = replicas * nb
        D = self.token_emb.weight.shape[1]
        x = torch.empty((S * n_tot, D), device=ids2d.device, dtype=torch.float32)
        L.embed(ids2d, self.token_emb.weight, self.pos_emb.weight, x, S, n, D, nb=nb, ids_prime=ids_prime)
        return x

    def _trunk(self, ids2d, video_patch_shape, *, context=None, text_mask=None, video_mask=None, attn_bias=None,
               use_cross=True, kv_cache=None, replicas=1, ids_prime=None):
        """ids2d (nb, n) int64 -> norm_out(transformer(emb)) as (S*n_tot, D) f32 for S = replicas * nb sequences.
        context (S, n_ctx, d) f32 and the masks cover all S sequences; masks may be bool or (already prepared) uint8."""
        L.require_device(ids2d, 'token ids')
        if ids2d.dtype != torch.int64 or not ids2d.is_contiguous():
            ids2d = ids2d.long().contiguous()
        nb, n = ids2d.shape
        S = replicas * nb
        n_tot = n + (ids_prime.shape[-1] if ids_prime is not None else 0)
        ctx2, n_ctx = None, None
        if use_cross and exists(context):
            n_ctx = context.shape[1]
            ctx2 = context.reshape(S * n_ctx, context.shape[-1])
            if ctx2.dtype != torch.float32 or not ctx2.is_contiguous():
                ctx2 = ctx2.float().contiguous()
        dt = compute_dtype_of(self)
        # the cond | null copies of a CFG batch see the same ids: until the first cross-attention they are the same rows, so layer 0's
        # PEG + self-attention run on nb sequences and write both copies (Transformer.run replicas)
        shared = replicas == 2 and self.transformer.shares_cfg_prefix(dt, ctx2, video_mask)
        x = self._embed(ids2d, 1 if shared else replicas, ids_prime)
        return self.transformer.run(x, S, n_tot, dt, video_shape=(S, *video_patch_shape),
                                    attn_bias=attn_bias, context2d=ctx2, n_ctx=n_ctx, self_attn_mask=_u8(video_mask),
                                    cross_attn_context_mask=_u8(text_mask) if ctx2 is not None else None,
                                    kv_cache=kv_cache, replicas=2 if shared else 1)

    def _cfg_embeds(self, x, video_patch_shape, context, text_mask, video_mask, with_null=True):
        """the scalar CFG layout: `embeds` of the 2b sequences [cond | null] -- context and masks doubled, the null half under an all-False text
        mask -- for pk_cfg_mix / pk_critic_head with has_null; with_null False: the plain b sequences"""
        if not with_null:
            return self.embeds(x, video_patch_shape=video_patch_shape, context=context, text_mask=text_mask, video_mask=video_mask)
        rep = lambda t: None if t is None else torch.cat((t, t), dim=0)
        return self.embeds(x, replicas=2, video_patch_shape=video_patch_shape, context=rep(context), text_mask=rep(text_mask),
                           video_mask=rep(video_mask), null_rows=x.shape[0])

    def _guided_embeds(self, x, video_patch_shape, context, text_mask, video_mask, cond_scale, negative_context, negative_text_mask):
        """the table layout with one conditional branch: `embeds` of the 2b sequences [cond | base] (base: the negative context, else the null
        branch) and the (2, b) device table row [1 | cond_scale[b]] for pk_guidance_mix / pk_critic_head_guided"""
        b = x.shape[0]
        table = guidance_table(_floats(cond_scale, b, 'cond_scale'), 1)[0]
        ctx_r, tm_r = guidance_contexts([(context.float(), text_mask)],
                                        (negative_context.float(), negative_text_mask) if exists(negative_context) else None)
        e = self.embeds(x, replicas=2, video_patch_shape=video_patch_shape, context=ctx_r, text_mask=tm_r,
                        video_mask=None if video_mask is None else torch.cat((video_mask, video_mask), dim=0))
        return e, table.to(x.device)

    def set_compute_dtype(self, name):
        return set_compute_dtype(self, name)


def _critic_scores(critic, e, b, n, with_null=False, cond_scale=1.):
    """(b, n) f32 scores of a critic's head on its trunk rows `e` (pk_critic_head: no noise; with_null mixes the [cond | null] halves)"""
    w, bias = critic.head()
    out = torch.empty((b, n), device=e.device, dtype=torch.float32)
    L.critic_head(e, w, bias, e.shape[1], b, n, 0, with_null, float(cond_scale), None, 0., out)
    return out


class MaskGit(_TokenTrunk):
    def __init__(self, *, dim, num_tokens, max_seq_len, gradient_shrink_alpha=0.1, heads=8, dim_head=64,
                 unconditional=False, attn_dropout=0., ff_dropout=0., **kwargs):
        super().__init__()
        self.dim = dim
        self.mask_id = num_tokens
        self.unconditional = unconditional
        self.token_emb = nn.Embedding(num_tokens + 1, dim)      # last token is used as mask_id
        self.max_seq_len = max_seq_len
        self.pos_emb = nn.Embedding(max_seq_len, dim)
        self.gradient_shrink_alpha = gradient_shrink_alpha      # identity in value (forward only)
        self.continuous_pos_bias = ContinuousPositionBias(dim=dim_head, heads=heads, num_dims=3)
        self.transformer = Transformer(dim=dim, attn_num_null_kv=2, has_cross_attn=not self.unconditional,
                                       dim_head=dim_head, heads=heads, attn_dropout=attn_dropout,
                                       ff_dropout=ff_dropout, peg=True, **kwargs)
        self.to_logits = nn.Linear(dim, num_tokens)

    def _prepare(self, x, text_mask, video_patch_shape):
        assert x.ndim in {2, 4}, 'video token ids must be of shape (batch, seq) or (batch, frame, height, width)'
        if x.ndim == 4:
            video_patch_shape = x.shape[1:]
            x = x.reshape(x.shape[0], -1)
        b, n = x.shape
        assert exists(video_patch_shape), 'video patch shape must be given'
        assert n <= self.max_seq_len, f'the video token sequence length you are passing in ({n}) is greater than the `max_seq_len` ({self.max_seq_len}) set on your `MaskGit`'
        return x, tuple(video_patch_shape)

    def embeds(self, x, *, video_patch_shape, context=None, text_mask=None, video_mask=None, null_rows=0, kv_cache=None,
               replicas=1, ids_prime=None):
        """norm_out rows (S*n_tot, D) f32 for S = replicas * x.shape[0] sequences (the replicas share the id rows); context /
        masks cover all S sequences; the LAST `null_rows` sequences get an all-False text mask (cond_drop_prob = 1,
        phenaki_pytorch.py:188-190) unless the caller already prepared a uint8 mask (sample())."""
        S = replicas * x.shape[0]
        text_mask = default_text_mask(context, text_mask, x.device)
        if exists(text_mask) and null_rows and text_mask.dtype != torch.uint8:
            text_mask = text_mask.clone()
            text_mask[S - null_rows:] = False
        bias =self.continuous_pos_bias.spec(*video_patch_shape)       # matrix or relative-position table, as each attention launch can use
        return self._trunk(x, video_patch_shape, context=context, text_mask=text_mask, video_mask=video_mask,
                           attn_bias=bias, use_cross=not self.unconditional, kv_cache=kv_cache, replicas=replicas,
                           ids_prime=ids_prime)

    def _logits(self, e2d, rows, S, n):
        dt = compute_dtype_of(self)
        V = self.to_logits.weight.shape[0]
        out = torch.empty((rows, V), device=e2d.device, dtype=torch.float32)
        L.gemm(dt, e2d, linear_weight(self.to_logits, dt), rows, V, self.dim, C=out, bias=self.to_logits.bias)
        return out.view(S, n, V)

    @torch.no_grad()
    def forward_with_cond_scale(self, *args, cond_scale=3, negative_context=None, negative_text_mask=None, **kwargs):
        """phenaki_pytorch.py:149-161.  A (B,) cond_scale, or negative_context (B, L, d) [negative_text_mask (B, L) bool] in place of the null
        branch, takes the table path: logits of base + (cond - base) * cond_scale[b] (pk_guidance_mix on the trunk outputs)."""
        guided = exists(negative_context) or not _is_scalar_scale(cond_scale)
        if not guided and cond_scale == 1:
            return self.forward(*args, cond_drop_prob=0., **kwargs)
        kwargs = dict(kwargs)
        x, vps = self._prepare(args[0], kwargs.get('text_mask'), kwargs.pop('video_patch_shape', None))
        b, n = x.shape
        context, text_mask, video_mask = kwargs.get('context'), kwargs.get('text_mask'), kwargs.get('video_mask')
        mixed = torch.empty((b * n, self.dim), device=x.device, dtype=L.tdtype(compute_dtype_of(self)))
        if guided:
            if self.unconditional or not exists(context):
                raise ValueError('forward_with_cond_scale: a per-sample cond_scale / negative_context needs a conditional MaskGit and a context')
            e, coef = self._guided_embeds(x, vps, context, text_mask, video_mask, cond_scale, negative_context, negative_text_mask)
            L.guidance_mix(e, b, n, 0, None, b * n, coef, 1, True, mixed, self.dim)
        else:
            e = self._cfg_embeds(x, vps, context, text_mask, video_mask)
            L.cfg_mix(e, b, n, 0, None, b * n, float(cond_scale), True, mixed, self.dim)
        return self._logits(mixed, b * n, b, n)

    def forward(self, x, cond_drop_prob=0., text_mask=None, video_mask=None, video_patch_shape=None,
                return_embeds=False, **kwargs):
        """phenaki_pytorch.py:163-213.  Grad mode on + trainable parameters: the logits / embeddings carry an autograd graph over this
        library's backward kernels (train.py); otherwise the fused inference path."""
        from .train import maskgit_forward_train, wants_grad
        if wants_grad(self):
            context = kwargs.pop('context', None)
            assert not kwargs, f'unexpected arguments {sorted(kwargs)}'
            return maskgit_forward_train(self, x, cond_drop_prob=cond_drop_prob, text_mask=text_mask, video_mask=video_mask,
                                         video_patch_shape=video_patch_shape, return_embeds=return_embeds, context=context)
        with torch.no_grad():
            return self._forward_value(x, cond_drop_prob, text_mask, video_mask, video_patch_shape, return_embeds, **kwargs)

    def _forward_value(self, x, cond_drop_prob=0., text_mask=None, video_mask=None, video_patch_shape=None,
                       return_embeds=False, **kwargs):
        x, vps = self._prepare(x, text_mask, video_patch_shape)
        b, n = x.shape
        context = kwargs.pop('context', None)
        assert not kwargs, f'unexpected arguments {sorted(kwargs)}'
        text_mask = cond_drop_text_mask(context, text_mask, cond_drop_prob, b, x.device, needs_context=False)
        e = self.embeds(x, video_patch_shape=vps, context=context, text_mask=text_mask, video_mask=video_mask)
        if return_embeds:
            return e.view(b, n, self.dim)
        return self._logits(e, b * n, b, n)


class TokenCritic(_TokenTrunk):
    def __init__(self, *, dim, num_tokens, max_seq_len, has_cross_attn=False, attn_dropout=0., ff_dropout=0., **kwargs):
        super().__init__()
        self.has_cross_attn = has_cross_attn
        self.mask_id = num_tokens
        self.token_emb = nn.Embedding(num_tokens + 1, dim)
        self.pos_emb = nn.Embedding(max_seq_len, dim)
        self.transformer = Transformer(dim=dim, peg=True, attn_dropout=attn_dropout, ff_dropout=ff_dropout,
                                       has_cross_attn=has_cross_attn, **kwargs)
        self.to_logits = nn.Sequential(nn.Linear(dim, 1), nn.Identity())

    def head(self):
        lin = self.to_logits[0]
        return lin.weight.reshape(-1), lin.bias

    def embeds(self, x, *, video_patch_shape, context=None, text_mask=None, video_mask=None, null_rows=0, kv_cache=None,
               replicas=1, ids_prime=None):
        S = replicas * x.shape[0]
        text_mask = default_text_mask(context, text_mask, x.device)
        if exists(text_mask) and exists(context) and null_rows and text_mask.dtype != torch.uint8:
            text_mask = text_mask.clone()
            text_mask[S - null_rows:] = False
        return self._trunk(x, video_patch_shape, context=context, text_mask=text_mask, video_mask=video_mask,
                           use_cross=self.has_cross_attn, kv_cache=kv_cache, replicas=replicas, ids_prime=ids_prime)

    def _scores(self, x, video_patch_shape, context, text_mask, video_mask, cond_scale, with_null):
        e = self._cfg_embeds(x, video_patch_shape, context, text_mask, video_mask, with_null)
        return _critic_scores(self, e, *x.shape, with_null, cond_scale)

    @staticmethod
    def _flatten(x, video_patch_shape):
        if exists(video_patch_shape):
            vps = tuple(video_patch_shape)
        else:
            vps = tuple(x.shape[1:])
        return x.reshape(x.shape[0], -1), vps

    @torch.no_grad()
    def forward_with_cond_scale(self, *args, cond_scale=3, negative_context=None, negative_text_mask=None, **kwargs):
        """phenaki_pytorch.py:251-263; a (B,) cond_scale or a negative_context mixes the head's scores as MaskGit.forward_with_cond_scale
        mixes the trunk outputs (pk_critic_head_guided).  A critic without cross-attention never sees the text: plain scores."""
        kwargs = dict(kwargs)
        x, vps = self._flatten(args[0], kwargs.pop('video_patch_shape', None))
        context, text_mask, video_mask = kwargs.get('context'), kwargs.get('text_mask'), kwargs.get('video_mask')
        if exists(negative_context) or not _is_scalar_scale(cond_scale):
            b, n = x.shape
            if not (self.has_cross_attn and exists(context)):
                _floats(cond_scale, b, 'cond_scale')                            # the argument is still checked
                return self._scores(x, vps, context, text_mask, video_mask, 1., False)
            e, coef = self._guided_embeds(x, vps, context, text_mask, video_mask, cond_scale, negative_context, negative_text_mask)
            w, bias = self.head()
            out = torch.empty((b, n), device=x.device, dtype=torch.float32)
            L.critic_head_guided(e, w, bias, e.shape[1], b, n, 0, coef, 1, True, None, 0., out)
            return out
        with_null = cond_scale != 1 and exists(context)      # without context both passes are identical
        return self._scores(x, vps, context, text_mask, video_mask, cond_scale, with_null)

    def forward(self, x, text_mask=None, cond_drop_prob=None, context=None, video_mask=None, video_patch_shape=None, **kwargs):
        """phenaki_pytorch.py:265-302; under grad mode with trainable parameters: with an autograd graph (train.py)"""
        from .train import critic_forward_train, wants_grad
        if wants_grad(self):
            return critic_forward_train(self, x, text_mask=text_mask, cond_drop_prob=cond_drop_prob, context=context, video_mask=video_mask,
                                        video_patch_shape=video_patch_shape)
        with torch.no_grad():
            return self._forward_value(x, text_mask, cond_drop_prob, context, video_mask, video_patch_shape)

    def _forward_value(self, x, text_mask=None, cond_drop_prob=None, context=None, video_mask=None, video_patch_shape=None):
        x, vps = self._flatten(x, video_patch_shape)
        text_mask = cond_drop_text_mask(context, text_mask, cond_drop_prob, x.shape[0], x.device, needs_context=True)
        return self._scores(x, vps, context, text_mask, video_mask, 1., False)


class SelfCritic(PackedModule):
    """phenaki_pytorch.py:306-336 : MaskGit embeddings -> Linear(dim, 1)."""

    def __init__(self, maskgit: MaskGit):
        super().__init__()
        self.maskgit = maskgit
        self.to_pred = nn.Sequential(nn.Linear(maskgit.dim, 1), nn.Identity())
        self.has_cross_attn = not maskgit.unconditional

    def head(self):
        lin = self.to_pred[0]
        return lin.weight.reshape(-1), lin.bias

    def embeds(self, x, **kw):
        return self.maskgit.embeds(x, **kw)

    @torch.no_grad()
    def forward_with_cond_scale(self, *args, cond_scale=3, **kwargs):
        kwargs = dict(kwargs)
        x, vps = self.maskgit._prepare(args[0], kwargs.get('text_mask'), kwargs.pop('video_patch_shape', None))
        with_null = cond_scale != 1
        e = self.maskgit._cfg_embeds(x, vps, kwargs.get('context'), kwargs.get('text_mask'), kwargs.get('video_mask'), with_null)
        return _critic_scores(self, e, *x.shape, with_null, cond_scale)

    def forward(self, x, *args, **kwargs):
        """phenaki_pytorch.py:334-336; under grad mode with trainable parameters: with an autograd graph (train.py)"""
        from .train import critic_forward_train, wants_grad
        if wants_grad(self):
            names = ('cond_drop_prob', 'text_mask', 'video_mask', 'video_patch_shape')
            kw = dict(zip(names, args))
            kw.update(kwargs)
            return critic_forward_train(self, x, text_mask=kw.get('text_mask'), cond_drop_prob=kw.get('cond_drop_prob'), context=kw.get('context'),
                                        video_mask=kw.get('video_mask'), video_patch_shape=kw.get('video_patch_shape'))
        with torch.no_grad():
            return self._forward_value(x, *args, **kwargs)

    def _forward_value(self, x, *args, **kwargs):
        embeds = self.maskgit(x, *args, return_embeds=True, **kwargs)
        b, n, d = embeds.shape
        return _critic_scores(self, embeds.reshape(b * n, d), b, n)


# what `Phenaki._masked_batch` / `Phenaki._sample_contexts` return; the fields are described there
MaskedBatch = namedtuple('MaskedBatch', 'ids patch_shape text_embeds text_mask video_mask mask masked_ids rows')
_SampleContexts = namedtuple('_SampleContexts', 'text_shape cond_scale with_null c_null ctx tm c_ctx c_tm P has_negative critic_guided')


class _SampleState:
    """everything `Phenaki._sample_loop` reads; a field that a call does not use is None.  The tensors are a captured graph's static inputs."""
    __slots__ = (
        'B', 'n', 'n_prime', 'patch_shape', 'prime_ids', 'prime_num_frames',        # n tokens to generate after n_prime prime tokens (B, n_prime)
        'ks', 'compact', 'starting_temperature', 'critic_noise',                    # ks[s] tokens re-masked at step s; critic noise scale per step
        'ids', 'mask', 'pred', 'scores', 'rows', 'partials', 'mixed',               # the loop's buffers (`Phenaki._sample_state`)
        'contexts', 'table',                                                        # _SampleContexts; table path: (steps, P + 1, B) f32 on the device
        'known', 'ks_dev', 'offs_dev', 'totals',                                    # infilling: known bytes (B, n) uint8, ks / offsets / row totals
        'noise_fn', 'trace', 'force_fn',                                            # parity hooks (eager only)
        'filter_k', 'slab',                                                         # top-k filter: k < V and the (R, V) f32 logits slab, else None
        'nucleus',                                                                  # an active nucleus filter: (top_p, min_p) floats, else None
        'seed_base', 'seed_dev')                                                    # graph mode: the base seed lives in *seed_dev, else seed_dev is None

    def __init__(self, **fields):
        for name in self.__slots__:
            setattr(self, name, fields.pop(name, None))
        assert not fields, f'unknown fields {sorted(fields)}'


_M64 = 0xFFFFFFFFFFFFFFFF
_head_seed = lambda seed_base, step: (seed_base + step * 0x9E3779B97F4A7C15) & _M64                 # pk_vocab_sample's stream at `step`
_critic_seed = lambda seed_base, step: (seed_base + (2 * step + 1) * 0xD6E8FEB86659FD93) & _M64     # pk_critic_head's


class Phenaki(PackedModule):
    def __init__(self, *, maskgit: MaskGit, cvivit: CViViT, critic=None, steps=18, t5_name=DEFAULT_T5_NAME,
                 sample_temperature=0., text_embed_dim=None, cond_drop_prob=0.25, max_text_len=128,
                 self_token_critic=False, critic_loss_weight=1., critic_noise_anneal_schedule='decay',
                 critic_train_sample_temperature=1., label_smoothing=0., z_loss_weight=0., train_cond_drop=False):
        """label_smoothing (eps in [0, 1)) and z_loss_weight (zeta >= 0) regularise the masked-token cross entropy of the training objective:
        mean_m [lse_m - (1 - eps) z_m[t_m] - eps mean_v z_m[v] + zeta lse_m^2] (train.py::vocab_cross_entropy); `evaluate` keeps the plain nll.
        train_cond_drop=True makes classifier-free-guidance dropout fire in the training step with probability `cond_drop_prob` (the reference
        shadows it with 0 at phenaki_pytorch.py:594, see train.py::phenaki_loss).  All three are off by default: the reference's objective."""
        super().__init__()
        self.label_smoothing, self.z_loss_weight = L.check_ce_regularisers(label_smoothing, z_loss_weight, 'Phenaki')
        if not isinstance(train_cond_drop, bool):
            raise ValueError(f'Phenaki: train_cond_drop must be a bool, got {train_cond_drop!r}')
        self.train_cond_drop = train_cond_drop
        assert isinstance(maskgit, MaskGit) and isinstance(cvivit, CViViT)
        assert critic is None or isinstance(critic, (TokenCritic, SelfCritic))
        self.cvivit = cvivit.copy_for_eval()
        self.maskgit = maskgit
        self.unconditional = maskgit.unconditional
        self.mask_id = maskgit.mask_id
        assert not (self_token_critic and exists(critic))
        if self_token_critic:
            critic = SelfCritic(maskgit)
        if exists(critic):
            critic = critic.eval()
        assert not exists(critic) or self_token_critic or (not maskgit.unconditional) == critic.has_cross_attn
        self.critic = critic
        self.critic_noise_anneal_schedule = critic_noise_anneal_schedule
        self.critic_loss_weight = critic_loss_weight
        self.critic_train_sample_temperature = critic_train_sample_temperature
        self.steps = steps
        self.sample_temperature = sample_temperature
        text_embed_dim = default(text_embed_dim, get_encoded_dim(t5_name) if text_embed_dim is None else None)
        self.encode_texts = partial(t5_encode_text, name=t5_name)
        self.text_embed_dim = text_embed_dim
        self.max_text_len = max_text_len
        assert cond_drop_prob > 0.
        self.cond_drop_prob = cond_drop_prob

    def set_compute_dtype(self, name):
        return set_compute_dtype(self, name)

    def sample_images(self, *, texts=None, batch_size=1, cond_scale=3., starting_temperature=0.9, noise_K=1., **guidance_kwargs):
        """guidance_kwargs: sample's guidance_schedule / negative_texts / blend"""
        video = self.sample(texts=texts, num_frames=1, cond_scale=cond_scale, starting_temperature=starting_temperature,
                            noise_K=noise_K, **guidance_kwargs)
        return video.squeeze(2)

    def forward(self, *args, **kwargs):
        """phenaki_pytorch.py:562-687.  With grad mode on and trainable MaskGit / critic parameters this is the training step: the loss
        carries an autograd graph whose nodes are the MI355X forward / backward kernels (train.py::phenaki_loss), `loss.backward()` fills
        the .grad of the MaskGit and critic parameters (the C-ViViT and the text encoder are frozen here as in the reference, :580-598).
        Otherwise (no_grad / eval without trainable parameters): the value only, through the fused inference kernels."""
        if torch.is_grad_enabled() and any(p.requires_grad for m in (self.maskgit, self.critic) if exists(m) for p in m.parameters()):
            from .train import phenaki_loss
            return phenaki_loss(self, *args, **kwargs)
        return self.objective_value(*args, **kwargs)

    def _cond_drop_masks(self, text_mask, cond_drop_prob, draws, b, need_critic):
        """(MaskGit's text mask, the critic's text mask) of one training call.  train_cond_drop off, or an unconditional model: both are
        `text_mask` itself and no random number is drawn.  On: cond_drop_prob = default(argument, self.cond_drop_prob), and MaskGit and the
        critic each AND their own prob_mask_like((b,), 1 - p) into it (phenaki_pytorch.py:188-189 through SelfCritic or MaskGit, :286-287 in a
        TokenCritic that attends to the text); draws['cond_keep'] / draws['critic_cond_keep'] ((b,) bool) replace the two draws."""
        if not self.train_cond_drop or self.unconditional or not exists(text_mask):
            return text_mask, text_mask
        p = float(default(cond_drop_prob, self.cond_drop_prob))
        if not 0. <= p <= 1.:
            raise ValueError(f'cond_drop_prob must be in [0, 1], got {cond_drop_prob!r}')
        device = text_mask.device

        def dropped(key):
            if key in draws:
                keep = draws[key].to(device).bool().reshape(b)
            elif p > 0:
                keep = prob_mask_like((b,), 1 - p, device=device)
            else:
                return text_mask
            return keep[:, None] & text_mask

        mg_mask = dropped('cond_keep')
        critic = self.critic
        critic_uses_text = need_critic and exists(critic) and (isinstance(critic, SelfCritic) or critic.has_cross_attn)
        return mg_mask, (dropped('critic_cond_keep') if critic_uses_text else text_mask)

    def _masked_batch(self, videos, texts, video_codebook_ids, video_frame_mask, text_embeds, draws, mask_prob=None, generator=None,
                      host_counts=False):
        """the inputs of the training call -> MaskedBatch(ids (b, n) int64, patch shape, text_embeds, text_mask, video_mask, mask (b, n) bool, masked
        ids, rows): the tokenizer / text-encoder front end and the masking of phenaki_pytorch.py:580-628, shared by objective_value, evaluate
        and the training step (train.py::phenaki_loss).  The two draws (schedule step, permutation noise) come from `draws` where it has
        them, else from `generator` (None: the default generator); mask_prob replaces the cosine schedule by a fixed fraction.
        host_counts=False: both draws on the ids' device, as the reference (:620); `rows` is None.
        host_counts=True (the training step): the schedule step is drawn on the HOST, so the number of masked tokens per sample -- hence the
        row count of the vocabulary head -- is known without reading anything back and the host can run a whole step ahead of the GPU; `rows`
        (M,) int32 lists the masked positions (flat b * n + i, ascending).  Under a video mask the counts live on the device: one read-back."""
        assert exists(videos) ^ exists(video_codebook_ids), 'either raw video or video codebook ids must be given'
        assert not (exists(videos) and not exists(self.cvivit)), 'cvivit must be provided if one wants to encode the videos live during training'
        assert (exists(text_embeds) ^ exists(texts)) ^ self.unconditional, \
            'either raw text of text embeds must be given, and if unconditional, none should be given'
        assert not (exists(text_embeds) and text_embeds.shape[-1] != self.text_embed_dim), 'text embedding dimension is not correct'
        if not exists(video_codebook_ids):
            assert videos.ndim in {4, 5}
            if videos.ndim == 4:
                videos = videos.unsqueeze(2)
            video_codebook_ids = self.cvivit(videos, return_only_codebook_ids=True)
        L.require_device(video_codebook_ids, 'video_codebook_ids')
        assert video_codebook_ids.ndim == 4, 'video codebook ids must be (batch, frames, height, width): MaskGit takes the patch shape from it'
        device = video_codebook_ids.device
        patch_shape = tuple(video_codebook_ids.shape[1:])

        text_mask = None
        if not self.unconditional:
            if not exists(text_embeds):
                text_embeds = self.encode_texts(texts, output_device=device)
            text_embeds = text_embeds.to(device).float()
            text_mask = torch.any(text_embeds != 0, dim=-1)

        video_mask = None
        if exists(video_frame_mask):
            video_mask = self.cvivit.calculate_video_token_mask(videos, video_frame_mask=video_frame_mask)

        ids = video_codebook_ids.reshape(video_codebook_ids.shape[0], -1).long().contiguous()
        b, n = ids.shape
        step_device = 'cpu' if host_counts else device
        if exists(mask_prob):
            mask_token_prob = torch.full((b,), float(mask_prob), device=step_device)
        else:
            rand_step = (draws['rand_step'].to(step_device) if 'rand_step' in draws
                         else torch.randint(0, self.steps, (b,), device=step_device, generator=generator))
            mask_token_prob = torch.cos(rand_step * math.pi * 0.5 / self.steps)
        perm_noise = draws['perm_noise'].to(device) if 'perm_noise' in draws else torch.rand((b, n), device=device, generator=generator)
        # get_mask_subset_with_prob (phenaki_pytorch.py:43-55)
        rows = None
        if host_counts and not exists(video_mask):
            num_masked = (mask_token_prob * n).round().clamp(min=1)
            M = int(num_masked.sum())
            # (pinned + non_blocking: a pageable host-to-device copy would wait for the stream, i.e. for the previous step)
            mask_token_mask = perm_noise.argsort(dim=-1) < num_masked.pin_memory().to(device, non_blocking=True)[:, None]
            # a stable sort lists the masked positions in ascending order, with a size the host already knows
            rows = torch.argsort((~mask_token_mask).reshape(-1).to(torch.uint8), stable=True)[:M].int()
        else:
            vm = video_mask if exists(video_mask) else torch.ones((b, n), device=device, dtype=torch.bool)
            num_tokens = vm.sum(dim=-1)
            num_masked = (mask_token_prob.to(device) * num_tokens).round().clamp(min=1)
            perm = perm_noise.argsort(dim=-1) - (n - num_tokens)[:, None]
            perm = perm.masked_fill(perm < 0, n)
            mask_token_mask = perm < num_masked[:, None]
            if host_counts:
                rows = mask_token_mask.reshape(-1).nonzero().reshape(-1).int()
        masked_input = torch.where(mask_token_mask, self.mask_id, ids)
        return MaskedBatch(ids, patch_shape, text_embeds, text_mask, video_mask, mask_token_mask, masked_input, rows)

    @torch.no_grad()
    def objective_value(self, videos=None, *, texts=None, video_codebook_ids=None, video_frame_mask=None, text_embeds=None,
                        cond_drop_prob=None, only_train_generator=False, only_train_critic=False, _draws=None):
        """phenaki_pytorch.py:562-687 -- the VALUE of the training objective (masked-token cross entropy + weighted
        token-critic BCE).  Forward only: the result carries no autograd graph (the backward kernels are SURVEY.md 8f
        "next").  The 65 536-way logits are never written: pk_vocab_sample draws the critic's input ids and leaves the
        softmax statistics, pk_vocab_ce turns them into per-row losses.  As in the reference, `cond_drop_prob` has no
        effect on this path (it is shadowed by `cond_drop_prob = 0` at :594) unless the model was built with train_cond_drop=True
        (`_cond_drop_masks`); label_smoothing / z_loss_weight apply as in the training step, so the two return the same number.
        _draws (tests): dict(rand_step (b,), perm_noise (b,n) U[0,1), gumbel_u (b,n,V) U[0,1)) replaces the three
        random draws of the reference (:620, :626 -> :43-55, :653); cond_keep / critic_cond_keep (b,) bool the two of train_cond_drop."""
        assert not (only_train_generator and only_train_critic)
        assert not (only_train_critic and not exists(self.critic)), 'only_train_critic needs a critic (Phenaki(critic=...) or self_token_critic=True)'
        mg, critic = self.maskgit, self.critic
        draws = _draws or {}
        mb = self._masked_batch(videos, texts, video_codebook_ids, video_frame_mask, text_embeds, draws)
        ids, mask_token_mask = mb.ids, mb.mask
        b, n = ids.shape
        device = ids.device

        dt = compute_dtype_of(mg)
        D, V = mg.dim, mg.to_logits.weight.shape[0]
        need_critic = exists(critic) and not only_train_generator
        mg_text_mask, critic_text_mask = self._cond_drop_masks(mb.text_mask, cond_drop_prob, draws, b, need_critic)
        e = mg.embeds(mb.masked_ids, video_patch_shape=mb.patch_shape, context=mb.text_embeds, text_mask=mg_text_mask, video_mask=mb.video_mask)
        # rows of the vocab head: the critic's labels compare the ids with the gumbel-sampled prediction at EVERY position
        # (phenaki_pytorch.py:653,671), so with a critic the head runs on all b*n rows; the generator-only objective needs
        # the masked rows only (>= 1 per sample, clamp(min=1) above)
        flat_mask = mask_token_mask.reshape(-1)
        rows = None if need_critic else flat_mask.nonzero().reshape(-1).int()
        M = b * n if need_critic else rows.numel()
        mixed = torch.empty((M, D), device=device, dtype=L.tdtype(dt))
        L.cfg_mix(e, b, n, 0, rows, M, 1.0, False, mixed, D)                    # (gather the rows,) cast to T
        w_logits = linear_weight(mg.to_logits, dt)
        partials = torch.empty((5 * L.vocab_ntiles(V) * M,), device=device, dtype=torch.float32)
        U = draws['gumbel_u'].to(device).float().contiguous() if 'gumbel_u' in draws else None
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if U is None else 0
        L.vocab_sample(dt, mixed, w_logits, mg.to_logits.bias, M, V, D, float(self.critic_train_sample_temperature), U, rows,
                       seed, True, partials)
        loss = None
        if not only_train_critic:
            loss_rows = torch.empty((M,), device=device, dtype=torch.float32)
            eps, zeta = self.label_smoothing, self.z_loss_weight
            wbar, bbar = L.vocab_weight_mean(dt, w_logits, mg.to_logits.bias, V, D) if eps > 0. else (None, None)
            L.vocab_ce(dt, partials, M, V, mixed, w_logits, mg.to_logits.bias, D, ids.reshape(-1), rows, loss_rows,
                       label_smoothing=eps, z_loss_weight=zeta, wbar=wbar, bbar=bbar)
            loss = (loss_rows[flat_mask] if need_critic else loss_rows).mean()
        if not need_critic:
            return loss
        pred = torch.empty((b * n,), device=device, dtype=torch.long)
        L.vocab_reduce(partials, M, V, None, None, None, pred, None, False)
        pred = pred.view(b, n)
        critic_input = torch.where(mask_token_mask, pred, ids)
        crit = critic(critic_input.view(b, *mb.patch_shape), video_mask=mb.video_mask, cond_drop_prob=0., text_mask=critic_text_mask,
                      context=mb.text_embeds)
        labels = (ids != pred).float()
        critic_loss = torch.nn.functional.binary_cross_entropy_with_logits(crit.reshape(b, n), labels)
        if only_train_critic:
            return critic_loss
        return loss + critic_loss * self.critic_loss_weight

    @torch.no_grad()
    def evaluate(self, videos=None, *, texts=None, video_codebook_ids=None, video_frame_mask=None, text_embeds=None, mask_prob=None,
                 generator=None, _draws=None):
        """held-out evaluation of the masked-token model: the per-token numbers a MaskGIT-style model is judged by, on the masked positions of
        one batch, without the (rows, V) logits (pk_vocab_eval).  Masking is that of the training objective (`objective_value`: the cosine
        schedule over `steps`, then get_mask_subset_with_prob, phenaki_pytorch.py:620-628).
        generator: a torch.Generator on the ids' device; the two draws (schedule step, permutation noise) come from it, so a validation set is
            masked identically every time.
        mask_prob: a number in (0, 1] replaces the schedule by that fixed fraction of every sample's tokens (1.0 masks them all).
        _draws (tests): dict(rand_step (b,), perm_noise (b, n)) as in objective_value.
        Returns a dict of device tensors; the host waits for nothing but the NUMBER of masked positions (the nonzero() that lists them, as in
        objective_value).  With M masked positions in all:
            rows (M,) int32 flat b * n + i of the masked positions, nll / entropy / lse (M,) f32 in nats, rank (M,) int32 = number of other
            tokens the model scores above the true one (top-k accuracy is rank < k), pred (M,) int64 arg-max, mask (b, n) bool.
        With a critic two more: critic_logits (b, n) = the critic's scores of the ids with the ARG-MAX pred filled in at the masked positions,
        and critic_labels (b, n) bool = ids != filled.  The fill is deterministic: unlike the training objective (:653), which draws a gumbel
        sample at critic_train_sample_temperature, a validation number must not move with a noise draw.
        Runs in eval mode and under no_grad; every module's train / eval flag is left as found (eval_decorator's pattern, per module: a
        Phenaki in train mode keeps its critic and tokenizer in eval mode)."""
        flags = [(m, m.training) for m in self.modules()]
        self.eval()
        try:
            return self._evaluate(videos, texts, video_codebook_ids, video_frame_mask, text_embeds, mask_prob, generator, _draws)
        finally:
            for m, was_training in flags:
                m.training = was_training

    def _evaluate(self, videos, texts, video_codebook_ids, video_frame_mask, text_embeds, mask_prob, generator, _draws):
        if exists(mask_prob) and not 0. < float(mask_prob) <= 1.:
            raise ValueError(f'evaluate: mask_prob must be in (0, 1], got {mask_prob}')
        mg, critic = self.maskgit, self.critic
        mb = self._masked_batch(videos, texts, video_codebook_ids, video_frame_mask, text_embeds, _draws or {}, mask_prob, generator)
        ids, mask_token_mask = mb.ids, mb.mask
        b, n = ids.shape
        device = ids.device

        dt = compute_dtype_of(mg)
        D, V = mg.dim, mg.to_logits.weight.shape[0]
        e = mg.embeds(mb.masked_ids, video_patch_shape=mb.patch_shape, context=mb.text_embeds, text_mask=mb.text_mask, video_mask=mb.video_mask)
        rows = mask_token_mask.reshape(-1).nonzero().reshape(-1).int()      # >= 1 per sample (clamp(min=1) above)
        M = rows.numel()
        mixed = torch.empty((M, D), device=device, dtype=L.tdtype(dt))
        L.cfg_mix(e, b, n, 0, rows, M, 1.0, False, mixed, D)                 # gather the masked rows, cast to T
        f32 = lambda: torch.empty((M,), device=device, dtype=torch.float32)
        out = dict(rows=rows, nll=f32(), entropy=f32(), lse=f32(), rank=torch.empty((M,), device=device, dtype=torch.int32),
                   pred=torch.empty((M,), device=device, dtype=torch.long), mask=mask_token_mask)
        L.vocab_eval(dt, mixed, linear_weight(mg.to_logits, dt), mg.to_logits.bias, M, V, D, ids.reshape(-1), rows,
                     pred=out['pred'], lse=out['lse'], nll=out['nll'], rank=out['rank'], entropy=out['entropy'])
        if exists(critic):
            filled = ids.reshape(-1).clone()
            filled[rows.long()] = out['pred']
            filled = filled.view(b, n)
            crit = critic(filled.view(b, *mb.patch_shape), video_mask=mb.video_mask, cond_drop_prob=0., text_mask=mb.text_mask, context=mb.text_embeds)
            out['critic_logits'] = crit.reshape(b, n)
            out['critic_labels'] = ids != filled
        return out

    # ------------------------------------------------------------------------------------------ sampling (phenaki_pytorch.py:418-560)

    def enable_sample_graph(self, on=True, static_output=False):
        """replay the whole 18-step sampling loop + final decode as ONE captured hipGraph per (batch, frames, prime, context
        length, guidance, temperature) configuration: ~3 000 kernel launches become one graph launch.  Noise stays fresh per
        call (the kernels add a device-resident seed word to their captured seeds).  Eager launches remain the default and the
        only mode for the parity hooks (_noise_fn / _trace).
        static_output=True: `sample` returns the graph's OWN output buffer (overwritten by the next call with the same configuration)
        instead of a clone of it -- saves a 13.4 MB-per-video copy per call for callers that consume the video before sampling again."""
        self.__dict__['_pk_sample_graph'] = bool(on)
        self.__dict__['_pk_sample_graph_static'] = bool(on and static_output)
        if not on:
            self.__dict__.pop('_pk_sample_graphs', None)
        return self

    def _sample_loop(self, st):
        """the mask-predict loop on prepared state `st` (_SampleState: device buffers + host scalars); kernels and allocations only, no host
        synchronisation and no torch elementwise ops: capturable as a hipGraph."""
        mg, critic = self.maskgit, self.critic
        dt = compute_dtype_of(mg)
        B, n, n_tot, npr, V, D = st.B, st.n, st.n + st.n_prime, st.n_prime, mg.to_logits.weight.shape[0], mg.dim
        ids, mask, pred, mixed, partials = st.ids, st.mask, st.pred, st.mixed, st.partials
        ks, steps, cx = st.ks, self.steps, st.contexts
        noise_fn, seed_dev = st.noise_fn, st.seed_dev
        seed_base = st.seed_base if seed_dev is None else 0             # graph mode: the base seed lives in *seed_dev
        need_lse = not exists(critic)
        trunk_kw = dict(ids_prime=st.prime_ids, video_patch_shape=st.patch_shape)
        mg_kw = dict(trunk_kw, context=cx.ctx, text_mask=cx.tm, kv_cache={})
        cr_kw = dict(trunk_kw, context=cx.c_ctx, text_mask=cx.c_tm, kv_cache={})
        # which mix and which critic head this run uses.  The table path: J = P + 1 branches [cond_0 | .. | cond_{P-1} | base] as one batch,
        # mixed with the step's table row; the scalar path: [cond | null] (or cond alone) with the scale baked into the launch
        if cx.P is not None:
            mg_kw['replicas'] = cx.P + 1
            mix = lambda e, rows, M, step: L.guidance_mix(e, B, n_tot, npr, rows, M, st.table[step], cx.P, True, mixed, D)
        else:
            mg_kw['replicas'] = 2 if cx.with_null else 1
            mix = lambda e, rows, M, step: L.cfg_mix(e, B, n_tot, npr, rows, M, float(cx.cond_scale), cx.with_null, mixed, D)
        if cx.critic_guided:
            cr_kw['replicas'] = cx.P + 1
            critic_head = lambda step, ce, w, bias, *tail, **seeds: L.critic_head_guided(
                ce, w, bias, ce.shape[1], B, n_tot, npr, st.table[step], cx.P, True, *tail, **seeds)
        else:
            cr_kw['replicas'] = 2 if cx.c_null else 1
            critic_head = lambda step, ce, w, bias, *tail, **seeds: L.critic_head(
                ce, w, bias, ce.shape[1], B, n_tot, npr, cx.c_null, float(cx.cond_scale), *tail, **seeds)
        w_logits = linear_weight(mg.to_logits, dt)
        for step in range(steps):
            is_last_step = step == (steps - 1)
            cur, nxt = st.scores[step & 1], st.scores[(step + 1) & 1]

            rows, M = None, B * n
            if st.known is not None:
                # infilling: re-mask among the FREE positions only, k_b(s) of them in sample b (known tokens are excluded by index, whatever
                # their score); step 0 has no scores and k_b = F_b: it masks every free position and lists it, so the head never visits a
                # known row.  The compact list is ragged: sample b's rows start at offs[s][b], M(s) = sum_b k_b(s) rows in all
                if st.compact:
                    rows, M = st.rows, st.totals[step]
                L.topk_mask_keep(cur if step > 0 else None, B, n, st.ks_dev[step], st.offs_dev[step], st.known, self.mask_id, mask, ids, rows,
                                 scores_next=nxt if need_lse else None, k_host=ks[step], free_host=ks[0])
            elif step > 0:
                # mask + ids = where(mask, mask_id, ids); only the k_s re-masked positions need the vocab head this step
                # (predictions elsewhere are discarded, phenaki_pytorch.py:509) -> compact row list for the head
                if st.compact:
                    rows, M = st.rows, B * ks[step]
                L.topk_mask(cur, B, n, ks[step], self.mask_id, mask, ids, rows, scores_next=nxt if need_lse else None)

            if st.force_fn is not None:
                # parity hook (eager only): the caller overwrites this step's masked ids / mask in place -- teacher forcing from a
                # reference run's recorded inputs (tests: all 18 steps audited even after a near-tie changed a free-running input)
                st.force_fn(step, ids, mask)

            rec = None
            if st.trace is not None:
                rec = dict(step=step, masked_ids=ids.clone(), mask=mask.bool().clone(), prime_ids=st.prime_ids)

            mix(mg.embeds(ids, **mg_kw), rows, M, step)
            temperature = st.starting_temperature * ((steps - (step + 1)) / steps)
            U = noise_fn('gumbel', step, (B, n, V)) if noise_fn is not None else None
            if st.nucleus is not None:
                # top-p / min-p (and a top-k, k = V without): the filtered head with the mass select in front of the draw
                L.vocab_sample_nucleus(dt, mixed, w_logits, mg.to_logits.bias, M, V, D, V if st.filter_k is None else st.filter_k, st.nucleus[0],
                                       st.nucleus[1], float(temperature), U, rows, _head_seed(seed_base, step), need_lse, mask, ids, pred,
                                       nxt if need_lse else None, st.slab, seed_dev=seed_dev)
            elif st.filter_k is not None:
                # top-k filter: the logits of a row slab exist, f32; the select, the draw and the reduce's write-out are one kernel
                L.vocab_sample_filtered(dt, mixed, w_logits, mg.to_logits.bias, M, V, D, st.filter_k, float(temperature), U, rows,
                                        _head_seed(seed_base, step), need_lse, mask, ids, pred, nxt if need_lse else None, st.slab, seed_dev=seed_dev)
            elif isinstance(U, L.TorchPhilox):
                # torch's own RNG stream: the noise torch.zeros((B, n, V)).uniform_() would hold, generated in the epilogue; then the
                # generator moves on as if that fill had happened (the reference's gumbel_noise, phenaki_pytorch.py:88-93)
                L.vocab_sample_philox(dt, mixed, w_logits, mg.to_logits.bias, M, V, D, float(temperature), rows, U, need_lse, partials)
                U.advance()
            else:
                L.vocab_sample(dt, mixed, w_logits, mg.to_logits.bias, M, V, D, float(temperature), U, rows,
                               _head_seed(seed_base, step), need_lse, partials, seed_dev=seed_dev)
            if st.filter_k is None and st.nucleus is None:
                L.vocab_reduce(partials, M, V, rows, mask, ids, pred, nxt if need_lse else None, need_lse)
            if rec is not None:
                rec.update(pred=pred.clone(), ids=ids.clone())

            if not is_last_step:
                if exists(critic):
                    ce = critic.embeds(ids, **cr_kw)
                    u = noise_fn('critic', step, (B, n)).contiguous() if noise_fn is not None else None
                    critic_head(step, ce, *critic.head(), u, st.critic_noise[step], nxt, seed=_critic_seed(seed_base, step), seed_dev=seed_dev)
                if rec is not None:
                    rec['scores'] = nxt.clone()
            if rec is not None:
                st.trace.append(rec)

        video = self.cvivit.decode_from_codebook_indices(ids, _prime_indices=st.prime_ids)
        if st.prime_ids is not None:
            video = video[:, :, st.prime_num_frames:]
        return video

    def _sample_arguments(self, texts, B, num_frames, prime_frames, cond_scale, guidance_schedule, negative_texts, blend, known_ids, known_mask,
                          noise_fn, noise_K, device, filter_thres=None, top_k=None, top_p=None, min_p=None):
        """sample()'s arguments, checked on the host: every ValueError, before anything is tokenized, encoded or launched.  Returns
        (plan: `_guidance_plan`; known: None or `_check_known`'s (ids, known bytes, free counts) -- the ONE host synchronisation of an infilling
        call; noise_fn: the callable; critic_noise: the critic's noise scale per step, None without a critic; filter_k: `_filter_k`; nucleus:
        `_filter_nucleus`)."""
        filter_k = self._filter_k(filter_thres, top_k, noise_fn)
        nucleus = self._filter_nucleus(top_p, min_p, noise_fn)
        plan = self._guidance_plan(texts, cond_scale, guidance_schedule, negative_texts, blend)
        known = None
        if exists(known_ids) or exists(known_mask):
            if not (exists(known_ids) and exists(known_mask)):
                raise ValueError('sample: give known_ids and known_mask together (or neither)')
            if exists(prime_frames):
                raise ValueError('sample: known_ids / known_mask cannot be combined with prime_frames')
            known = _check_known(known_ids, known_mask, B, self.cvivit.get_video_patch_shape(num_frames),
                                 self.maskgit.to_logits.weight.shape[0], device)
        critic_noise = None
        if exists(self.critic):
            critic_noise = [float(noise_K * critic_noise_multiplier(self.critic_noise_anneal_schedule, s, self.steps)) for s in range(self.steps - 1)]
        if isinstance(noise_fn, str):
            # _noise_fn = 'torch': the reference's own noise -- torch's device generator, consumed in the reference's order (per step one
            # uniform_ of (B, n, V) for gumbel_sample, phenaki_pytorch.py:88-93, then one of (B, n) for the critic scores, :69-70 / :541-543).
            # The (B, n, V) fill is never materialised: the vocabulary head reproduces its elements from the Philox state (pk_vocab_sample_philox)
            # and the generator is moved past it, so `torch.manual_seed(s); phenaki.sample(...)` draws what a reference run on this GPU draws.
            assert noise_fn == 'torch', "_noise_fn: a callable or 'torch'"

            def noise_fn(kind, step, shape):
                if kind == 'gumbel':
                    return L.TorchPhilox(device, shape[0] * shape[1] * shape[2])
                return torch.zeros(shape, device=device).float().uniform_(0, 1)
        return plan, known, noise_fn, critic_noise, filter_k, nucleus

    def _filter_k(self, filter_thres, top_k, noise_fn):
        """the k of the top-k filter from sample()'s filter_thres / top_k: None for the plain path (no filter given, or one that keeps all V
        columns).  filter_thres resolves as the reference's top_k helper writes it (phenaki_pytorch.py:97): k = max(int((1 - thres) * V), 1)."""
        if filter_thres is None and top_k is None:
            return None
        V = self.maskgit.to_logits.weight.shape[0]
        if filter_thres is not None and top_k is not None:
            raise ValueError('sample: give filter_thres or top_k, not both')
        if isinstance(noise_fn, str):
            raise ValueError("sample: filter_thres / top_k cannot be combined with _noise_fn='torch' (the Philox stream has no filtered path)")
        if top_k is not None:
            if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= V:
                raise ValueError(f'sample: top_k must be an int in [1, {V}], got {top_k!r}')
            k = top_k
        else:
            if isinstance(filter_thres, bool) or not isinstance(filter_thres, (int, float)) or not (0. <= filter_thres < 1.):     # NaN fails the range
                raise ValueError(f'sample: filter_thres must be a finite number in [0, 1), got {filter_thres!r}')
            k = max(int((1 - filter_thres) * V), 1)
        return None if k >= V else k

    def _filter_nucleus(self, top_p, min_p, noise_fn):
        """(top_p, min_p) as floats when sample()'s top_p / min_p make a filter active, else None: top_p None or 1 and min_p None or 0 are off"""
        if top_p is None and min_p is None:
            return None
        number = lambda x: not isinstance(x, bool) and isinstance(x, (int, float))
        if top_p is not None and not (number(top_p) and 0. < top_p <= 1.):                               # NaN fails the range
            raise ValueError(f'sample: top_p must be a finite number in (0, 1], got {top_p!r}')
        if min_p is not None and not (number(min_p) and 0. <= min_p < 1.):
            raise ValueError(f'sample: min_p must be a finite number in [0, 1), got {min_p!r}')
        top_p, min_p = 1. if top_p is None else float(top_p), 0. if min_p is None else float(min_p)
        if top_p == 1. and min_p == 0.:
            return None
        if isinstance(noise_fn, str):
            raise ValueError("sample: top_p / min_p cannot be combined with _noise_fn='torch' (the Philox stream has no filtered path)")
        # the kernel takes both as f32: what is in range as a double stays in range (and active) as a float.  A top_p below 2^-126 keeps the
        # maximum alone either way and a min_p above 1 - 2^-24 the maximum's exact ties alone; a positive min_p below 2^-126 is raised to it
        if min_p > 0.:
            min_p = min(max(min_p, 2. ** -126), 1. - 2. ** -24)
        return max(top_p, 2. ** -126), min_p

    def _prime_tokens(self, prime_frames, prime_ids, device):
        """(token ids (B, n_prime) of the prime frames, their frame count), (None, 0) without; `prime_ids` (tests) replaces the tokenizer's ids"""
        if not exists(prime_frames):
            return None, 0
        ids = self.cvivit(prime_frames, return_only_codebook_ids=True)
        ids = ids.reshape(ids.shape[0], -1).contiguous()
        if prime_ids is not None:
            assert tuple(prime_ids.shape) == tuple(ids.shape)
            ids = prime_ids.to(device=device, dtype=ids.dtype).contiguous()
        return ids, prime_frames.shape[2]

    def _sample_contexts(self, texts, B, plan, cond_scale, device):
        """encode the texts and lay out what MaskGit and the critic attend to, once per call: _SampleContexts(text_shape: the graph key's entry;
        cond_scale; with_null / c_null: MaskGit / the critic runs [cond | null]; ctx (S, L, d) f32, tm (S, L) uint8: MaskGit's context and text
        mask, c_ctx, c_tm: the critic's, None for a trunk that never sees a text; P, has_negative, critic_guided: the table path).
        Scalar path (plan None, P None): classifier-free guidance runs the cond and null passes as ONE batch of 2B sequences, the null half
        under an all-False text mask (phenaki_pytorch.py:188-190); cond_scale == 1 or no text leaves B sequences.
        Table path: all J = P + 1 branches (the texts, the blend texts, then the base: the negative texts or the null branch) as one batch of
        J B sequences on contexts zero-padded to the longest length, padded rows masked out (`guidance_contexts`); MaskGit and a critic that
        sees the text (critic_guided; a text-blind one keeps pk_critic_head) share the one layout.  cond_scale is 1. and never read."""
        mg, critic = self.maskgit, self.critic
        text_embeds = text_mask = None
        if exists(texts):
            text_embeds = self.encode_texts(texts, output_device=device).to(device).float().contiguous()
            text_mask = torch.any(text_embeds != 0, dim=-1)
        if plan is not None:
            conds = [(text_embeds, text_mask)] + [self._encode_branch(t, B, device) for t in plan['blend_texts']]
            base = self._encode_branch(plan['negative_texts'], B, device) if plan['negative_texts'] is not None else None
            ctx, tm = guidance_contexts(conds, base)
            c_text = exists(critic) and (isinstance(critic, SelfCritic) or critic.has_cross_attn)
            return _SampleContexts(tuple(ctx.shape), 1., False, False, ctx, tm, ctx if c_text else None, tm if c_text else None,
                                   plan['P'], base is not None, c_text)
        has_ctx = exists(text_embeds) and not mg.unconditional
        with_null = has_ctx and cond_scale != 1
        c_has_ctx = exists(critic) and exists(text_embeds) and critic.has_cross_attn
        c_null = (c_has_ctx and cond_scale != 1) if not isinstance(critic, SelfCritic) else cond_scale != 1

        def layout(sees_text, null):
            if not sees_text:
                return None, None
            return (torch.cat((text_embeds, text_embeds), dim=0) if null else text_embeds).contiguous(), _cfg_masks(text_mask, B, null)

        return _SampleContexts(None if text_embeds is None else tuple(text_embeds.shape), cond_scale, with_null, c_null,
                               *layout(has_ctx, with_null), *layout(c_has_ctx, c_null), None, False, False)

    def _sample_seed(self, noise_fn, seed):
        """the 62-bit base seed of the in-kernel counter hash: drawn from torch's default (CPU) generator, offset per rank, or `seed` itself;
        0 (and no draw) when the caller injects the noise.  Kept in `self._pk_last_seed`."""
        seed_base = int(torch.randint(0, 2 ** 62, (1,)).item()) if noise_fn is None else 0
        if noise_fn is None and torch.distributed.is_available() and torch.distributed.is_initialized():
            # batch-sharded sampling: every rank draws from its own noise stream even under a common torch seed
            seed_base = (seed_base + 0xD1B54A32D192ED03 * (torch.distributed.get_rank() + 1)) & 0x3FFFFFFFFFFFFFFF
        if seed is not None:
            seed_base = int(seed) & 0x3FFFFFFFFFFFFFFF
        self.__dict__['_pk_last_seed'] = seed_base
        return seed_base

    def _sample_key(self, B, n, n_prime, prime_num_frames, patch_shape, cx, starting_temperature, noise_K, compact, dt, device, known, filter_k=None,
                    nucleus=None):
        """what a captured graph of the loop depends on (`_pk_sample_graphs`' key, kept in `_pk_last_sample_key`).  On the table path the
        scales, schedule and weights live in the table, a static input refilled per call: the key names the launch structure only --
        ('guided', P, has_negative, L) in place of the scale -- so calls that differ only in those replay one graph.  Infilling: the free
        counts are part of the key; another mask with the same counts replays, other counts capture again.  The resolved k of a top-k filter
        (None on the plain path) is the last entry: another k is another kernel argument and captures another graph.  With an active nucleus
        filter the last entry is ('nucleus', k or None, top_p, min_p) instead."""
        scale = float(cx.cond_scale) if cx.P is None else ('guided', cx.P, cx.has_negative, cx.text_shape[1])
        key = (B, n, n_prime, prime_num_frames, tuple(patch_shape), cx.text_shape, scale, float(starting_temperature), float(noise_K), compact,
               dt, str(device), self.steps, self.critic_noise_anneal_schedule, None if known is None else tuple(known[2]),
               filter_k if nucleus is None else ('nucleus', filter_k, float(nucleus[0]), float(nucleus[1])))
        self.__dict__['_pk_last_sample_key'] = key
        return key

    def _sample_state(self, B, n, patch_shape, cx, plan, known, device, dt, static=False, **scalars):
        """the loop's state with its buffers allocated.  static: the state of a captured graph -- it owns its contexts (their clones, refilled
        per call by `_sample_graphed`; what was one tensor stays one) and keeps the base seed on the device."""
        V, D = self.maskgit.to_logits.weight.shape[0], self.maskgit.dim
        if static:
            own = lambda t: None if t is None else t.clone()
            ctx, tm = own(cx.ctx), own(cx.tm)
            cx = cx._replace(ctx=ctx, tm=tm, c_ctx=ctx if cx.c_ctx is cx.ctx else own(cx.c_ctx), c_tm=tm if cx.c_tm is cx.tm else own(cx.c_tm))
        st = _SampleState(B=B, n=n, patch_shape=patch_shape, ks=mask_schedule(n, self.steps), contexts=cx,
                          ids=torch.empty((B, n), device=device, dtype=torch.int64),
                          mask=torch.empty((B, n), device=device, dtype=torch.uint8),
                          pred=torch.empty((B, n), device=device, dtype=torch.int64),
                          scores=[torch.empty((B, n), device=device, dtype=torch.float32) for _ in range(2)],
                          rows=torch.empty((B * n,), device=device, dtype=torch.int32),
                          partials=(torch.empty((5 * L.vocab_ntiles(V) * B * n,), device=device, dtype=torch.float32)
                                    if scalars.get('filter_k') is None and scalars.get('nucleus') is None else None),   # a filtered head has the slab instead
                          mixed=torch.empty((B * n, D), device=device, dtype=L.tdtype(dt)), **scalars)
        if st.filter_k is not None or st.nucleus is not None:
            st.slab = torch.empty((L.filter_slab_rows(B * n, V), V), device=device, dtype=torch.float32)
        if plan is not None:
            st.table = plan['table'].to(device)
        if known is not None:
            st.ks, offs, st.totals = infill_schedule(known[2], self.steps)
            st.known = torch.empty_like(known[1])
            st.ks_dev = torch.tensor(st.ks, dtype=torch.int32, device=device)
            st.offs_dev = torch.tensor(offs, dtype=torch.int32, device=device)
        if static:
            st.seed_dev = torch.zeros((1,), device=device, dtype=torch.int64)
        return st

    def _sample_start(self, st, known):
        """the loop's starting state, in place (the buffers are a captured graph's static inputs): everything masked; or, when infilling,
        the caller's ids and known bytes -- step 0's pk_topk_mask_keep then lays the mask_id over the free positions"""
        if known is None:
            st.ids.fill_(self.mask_id)
            st.mask.fill_(1)
        else:
            st.ids.copy_(known[0])
            st.known.copy_(known[1])

    def _sample_graphed(self, key, make_state, cx, plan, prime_ids, known, seed_base, return_ids):
        """run the loop through the graph cache `_pk_sample_graphs`: {key: dict(graph, st, video, fingerprint)}"""
        device = next(self.parameters()).device
        graphs = self.__dict__.setdefault('_pk_sample_graphs', {})
        # a captured graph holds raw pointers to the live parameters AND to the packed copies derived from them: any change of a
        # parameter (optimizer step, EMA update through the autograd-visible path, load_state_dict, .to()) re-captures
        fp = param_fingerprint(self)
        entry = graphs.get(key)
        if entry is not None and entry['fingerprint'] != fp:
            graphs.pop(key)
            entry = None
        if entry is not None:
            # refill the graph's static inputs in place from this call's layout: contexts, table, prime ids
            st = entry['st']
            have = st.contexts
            pairs = {id(d): (d, s) for d, s in ((have.ctx, cx.ctx), (have.tm, cx.tm), (have.c_ctx, cx.c_ctx), (have.c_tm, cx.c_tm)) if d is not None}
            for dst, src in list(pairs.values()) + [(st.table, plan and plan['table']), (st.prime_ids, prime_ids)]:
                if dst is not None:
                    dst.copy_(src)
            self._sample_start(st, known)
            st.seed_dev.fill_(seed_base)
        else:
            # first call for this configuration: one eager pass (packs weights, fills the bias caches), then capture
            st = make_state(static=True)
            self._sample_start(st, known)
            st.seed_dev.fill_(seed_base)
            entry = dict(st=st, fingerprint=fp)
            side = torch.cuda.Stream(device=device)
            side.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.stream(side):
                self._sample_loop(st)
            torch.cuda.current_stream(device).wait_stream(side)
            self._sample_start(st, known)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                entry['video'] = self._sample_loop(st)
            entry['graph'] = graph
            graphs[key] = entry
        entry['graph'].replay()
        video = entry['video'] if self.__dict__.get('_pk_sample_graph_static') else entry['video'].clone()
        return (video, st.ids.clone()) if return_ids else video

    def _guidance_plan(self, texts, cond_scale, guidance_schedule, negative_texts, blend):
        """sample()'s guidance arguments, checked on the host (every ValueError of the table path, before anything is encoded or launched).
        None: the scalar path (a Python-number cond_scale and no other guidance argument).  Else dict(B, table (steps, P + 1, B) f32 on the
        host, P, blend_texts [str | list of B str], negative_texts None | str | list of B str)."""
        if _is_scalar_scale(cond_scale) and guidance_schedule is None and negative_texts is None and blend is None:
            return None
        if texts is None or self.unconditional:
            raise ValueError('sample: per-sample cond_scale / guidance_schedule / negative_texts / blend need texts and a conditional MaskGit')
        B = 1 if isinstance(texts, str) else len(texts)

        def branch_texts(t, what):
            if isinstance(t, str):
                return t
            if not isinstance(t, (list, tuple)) or not all(isinstance(s, str) for s in t) or len(t) != B:
                raise ValueError(f'sample: {what} must be a str or a list of {B} strings')
            return list(t)

        cs = _floats(cond_scale, B, 'sample: cond_scale')
        m = guidance_multipliers(guidance_schedule, self.steps)
        blend = [] if blend is None else list(blend)
        if len(blend) > GUIDANCE_MAX_BRANCHES - 1:
            raise ValueError(f'sample: blend takes at most {GUIDANCE_MAX_BRANCHES - 1} (texts, weight) pairs, got {len(blend)}')
        blend_texts, weights = [], []
        for k, pair in enumerate(blend):
            if not isinstance(pair, (list, tuple)) or len(pair) != 2:
                raise ValueError(f'sample: blend[{k}] must be a (texts, weight) pair')
            blend_texts.append(branch_texts(pair[0], f'blend[{k}] texts'))
            weights.append(_floats(pair[1], B, f'sample: blend[{k}] weight'))
        if negative_texts is not None:
            negative_texts = branch_texts(negative_texts, 'negative_texts')
        return dict(B=B, P=1 + len(blend_texts), table=guidance_table(cs, self.steps, m, weights), blend_texts=blend_texts,
                    negative_texts=negative_texts)

    def _encode_branch(self, branch_texts, B, device):
        """(embeddings (B, L, d) f32, text mask (B, L) bool = any(embeds != 0)) of one branch's texts; a str is encoded once and shared"""
        shared = isinstance(branch_texts, str)
        emb = self.encode_texts([branch_texts] if shared else branch_texts, output_device=device).to(device).float()
        if shared and B > 1:
            emb = emb.expand(B, -1, -1)
        return emb, torch.any(emb != 0, dim=-1)

    @eval_decorator
    @torch.no_grad()
    def sample(self, *, num_frames, texts=None, prime_frames=None, batch_size=1, cond_scale=3.,
               starting_temperature=0.9, noise_K=1., _noise_fn=None, _trace=None, _return_ids=False, _compact=None, _seed=None,
               _force_fn=None, _prime_ids=None, known_ids=None, known_mask=None, guidance_schedule=None, negative_texts=None, blend=None,
               filter_thres=None, top_k=None, top_p=None, min_p=None):
        """phenaki_pytorch.py:418-560: `num_frames` new frames for `texts` (a str or B strings; without texts `batch_size` samples), continuing
        `prime_frames` if given.  Returns the video (B, C, num_frames, H, W).

        Noise comes from an in-kernel counter hash seeded from torch's default (CPU) generator; the seed a call used is kept in
        `self._pk_last_seed`.  With `enable_sample_graph` the whole call replays one captured graph per configuration.

        Infilling: `known_ids` (int64 token ids) and `known_mask` (bool, True = keep the token), both or neither, shaped (B, f, h, w) or
        (B, n) for (f, h, w) = get_video_patch_shape(num_frames); the mask may also be (f, h, w) or (n,), shared by the batch.  The known
        tokens stay as given and are part of the decoded clip; only the free ones are sampled, k_b(s) = mask_schedule(F_b, steps)[s] of sample
        b's F_b free tokens re-masked per step.  Not combined with prime_frames.  The free counts F_b are read from the device once per call:
        ONE host synchronisation that a plain call does not have.

        Guidance.  `cond_scale`: a Python number (the scalar path: one scale for the batch and all steps), or a sequence / 1-D tensor of B
        finite floats, one per sample.  `guidance_schedule`: None, 'linear' (m[s] = (s + 1) / steps) or `steps` finite floats m[s]; the scale
        of step s is 1 + (cond_scale[b] - 1) m[s].  `negative_texts`: a str shared by the batch or B strings; the guidance then points away
        from that text's trunk output instead of the null branch's.  `blend`: up to two (texts_k, weight_k) pairs, texts_k a str (shared) or
        B strings, weight_k a float or B floats: the conditional output becomes (1 - sum_k weight_k) e(texts) + sum_k weight_k e(texts_k).
        Any of these, or a non-scalar cond_scale, selects the table path (`_sample_contexts`, `_sample_key`).

        Top-k filtering.  `filter_thres` (a finite number in [0, 1); k = max(int((1 - filter_thres) * V), 1), the reference's top_k helper,
        phenaki_pytorch.py:95-101) or `top_k` (an int in [1, V]), not both: every draw of the vocabulary head is taken from the columns whose
        logit is >= the row's k-th largest (exact ties at the cut are all kept; torch.topk keeps an arbitrary k of them).  The confidence score
        of a critic-less run stays 1 - p under the unfiltered softmax.  k = V, or neither argument, is the plain path: the logits are never
        formed.  With a filter they are, one (R, V) f32 slab at a time (`_lib.vocab_sample_filtered`).  Not combined with _noise_fn='torch'.

        Nucleus and min-p filtering (the reference has neither).  `top_p`: a finite number in (0, 1], None or 1 = off: keep the smallest set of
        most likely codes whose probability sums to top_p.  `min_p`: a finite number in [0, 1), None or 0 = off: keep the codes whose
        probability is at least min_p times the most likely one's.  Either or both may be combined with one of filter_thres / top_k; the
        filters apply in the order temperature, top-k, top-p, min-p and a column is kept iff every active one keeps it.  The probabilities are
        those of softmax(logits / T) at the step's annealed temperature T (the distribution the gumbel arg-max samples from), top-p taken on
        the top-k set's own mass; exact ties at a cut are all kept, and at the last step (T = 0) the nucleus is the row maximum and its exact
        ties.  The exact arithmetic is pk_logits_nucleus_sample's (include/phenaki_hip.h).  With either active every step's head is one
        `_lib.vocab_sample_nucleus`; both off is exactly the path above.  Not combined with _noise_fn='torch'.

        Shape, dtype, range and length errors (known ids outside [0, num_tokens), a sample with nothing to generate, non-finite values, more
        than two blend entries, a guidance argument without texts or on an unconditional MaskGit, an unknown critic_noise_anneal_schedule)
        are ValueErrors raised before anything launches (`_sample_arguments`).
        Test hooks: `_noise_fn(kind, step, shape)` injects the U[0,1) draws of a reference run ('gumbel' (B,n,V) and 'critic' (B,n), device
        f32 tensors); _noise_fn='torch': torch's device generator in the reference's order.  `_seed`: the exact 64-bit stream seed.
        `_force_fn(step, ids, mask)` may overwrite a step's masked input ids (B, n) int64 and mask (B, n) uint8 in place before the trunk
        runs (teacher forcing), `_trace` is a list that receives one record per step: both run eagerly without row compaction.  `_prime_ids`
        replaces the token ids the tokenizer would produce for the prime frames; `_return_ids`: also return the sampled ids (B, n)."""
        device = next(self.parameters()).device
        L.require_device(next(self.parameters()), 'Phenaki parameters')
        dt = compute_dtype_of(self.maskgit)
        if isinstance(texts, str):
            texts = [texts]
        B = len(texts) if exists(texts) else batch_size
        plan, known, noise_fn, critic_noise, filter_k, nucleus = self._sample_arguments(
            texts, B, num_frames, prime_frames, cond_scale, guidance_schedule, negative_texts, blend, known_ids, known_mask, _noise_fn, noise_K, device,
            filter_thres, top_k, top_p, min_p)
        prime_ids, prime_num_frames = self._prime_tokens(prime_frames, _prime_ids, device)
        n_prime = 0 if prime_ids is None else prime_ids.shape[-1]
        n = self.cvivit.num_tokens_per_frames(num_frames, include_first_frame=not exists(prime_frames))
        patch_shape = self.cvivit.get_video_patch_shape(num_frames + prime_num_frames, include_first_frame=True)
        cx = self._sample_contexts(texts, B, plan, cond_scale, device)
        seed_base = self._sample_seed(noise_fn, _seed)
        compact = (_trace is None) if _compact is None else bool(_compact)    # traces record the prediction at EVERY position
        if _force_fn is not None:
            compact = False                                                    # the forced mask need not be the top-k one
        key = self._sample_key(B, n, n_prime, prime_num_frames, patch_shape, cx, starting_temperature, noise_K, compact, dt, device, known, filter_k,
                               nucleus)
        make_state = partial(self._sample_state, B, n, patch_shape, cx, plan, known, device, dt, n_prime=n_prime, prime_ids=prime_ids,
                             prime_num_frames=prime_num_frames, compact=compact, starting_temperature=starting_temperature,
                             critic_noise=critic_noise, noise_fn=noise_fn, trace=_trace, force_fn=_force_fn, seed_base=seed_base, filter_k=filter_k,
                             nucleus=nucleus)
        if self.__dict__.get('_pk_sample_graph', False) and noise_fn is None and _trace is None and _force_fn is None:
            return self._sample_graphed(key, make_state, cx, plan, prime_ids, known, seed_base, _return_ids)
        st = make_state()
        self._sample_start(st, known)
        video = self._sample_loop(st)
        return (video, st.ids) if _return_ids else video

    @eval_decorator
    @torch.no_grad()
    def infill(self, video, edit_mask, *, texts=None, mask_level='pixel', composite=False, **sample_kwargs):
        """regenerate a region of a clip and keep the rest: inpainting / outpainting (a spatial region), frame interpolation or extension in
        either direction (whole frames), in token space.  `video` (B, C, F, H, W) float32; `edit_mask` bool, True = regenerate:
          mask_level='pixel': (B | 1, F, H, W).  A token is regenerated iff ANY pixel of its footprint is marked: token frame 0 is video
                              frame 0, token frame t >= 1 covers frames 1 + (t-1) pt .. t pt, spatially the ph x pw patch;
          mask_level='token': (B | 1, f, h, w) over get_video_patch_shape(F), taken as it is.
        The clip is tokenised, the tokens outside the edit region become sample()'s known tokens (the one host synchronisation and the
        graph key of `sample(known_ids=, known_mask=)` apply; other keyword arguments go to sample) and the decoded clip, ALL frames, is
        returned.  The known tokens were computed from the ORIGINAL clip -- the tokenizer attends spatially and causally in time, so a known
        token may carry traces of the pixels that are being replaced, and kept regions come back as the tokenizer reconstructs them (the
        usual token-space inpainting).  composite=True returns where(edit pixels, decoded, video) instead (pk_composite_mask): pixels
        outside the mask are the input's bits; the pixel mask is the caller's at mask_level='pixel', the tokens' footprint at 'token'."""
        cv = self.cvivit
        if mask_level not in ('pixel', 'token'):
            raise ValueError(f"infill: mask_level must be 'pixel' or 'token', got {mask_level!r}")
        if not torch.is_tensor(video) or video.ndim != 5 or video.dtype != torch.float32:
            raise ValueError('infill: video must be a (B, C, F, H, W) float32 tensor')
        if 'prime_frames' in sample_kwargs or 'known_ids' in sample_kwargs or 'known_mask' in sample_kwargs or 'num_frames' in sample_kwargs:
            raise ValueError('infill: prime_frames / known_ids / known_mask / num_frames are not arguments of infill')
        B, C, F, H, W = video.shape
        pt = cv.temporal_patch_size
        if (H, W) != tuple(cv.image_size) or (F - 1) % pt:
            raise ValueError(f'infill: video must be {tuple(cv.image_size)} pixels with 1 + a multiple of {pt} frames, got {(F, H, W)}')
        grid = tuple(cv.get_video_patch_shape(F))
        want = (F, H, W) if mask_level == 'pixel' else grid
        if not torch.is_tensor(edit_mask) or edit_mask.dtype != torch.bool:
            raise ValueError('infill: edit_mask must be a bool tensor (True = regenerate)')
        if edit_mask.ndim != 4 or edit_mask.shape[0] not in (1, B) or tuple(edit_mask.shape[1:]) != want:
            raise ValueError(f'infill: a {mask_level} edit_mask must be ({B} | 1, {", ".join(map(str, want))}), got {tuple(edit_mask.shape)}')
        edit_mask = edit_mask.to(video.device)
        token_edit = pixel_to_token_mask(edit_mask, pt, cv.patch_size) if mask_level == 'pixel' else edit_mask
        ids = cv(video, return_only_codebook_ids=True).reshape(B, -1)
        known_mask = ~token_edit
        out = self.sample(num_frames=F, texts=texts, batch_size=B, known_ids=ids, known_mask=known_mask[0] if known_mask.shape[0] == 1 else known_mask,
                          **sample_kwargs)
        if not composite:
            return out
        decoded = out[0] if isinstance(out, tuple) else out
        pixel_edit = edit_mask if mask_level == 'pixel' else token_to_pixel_mask(edit_mask, pt, cv.patch_size)
        mixed = torch.empty_like(video, memory_format=torch.contiguous_format)
        L.composite_mask(decoded.contiguous(), video.contiguous(), pixel_edit.to(torch.uint8).contiguous(), mixed)
        return (mixed, *out[1:]) if isinstance(out, tuple) else mixed


def make_video(phenaki: Phenaki, texts: List[str], num_frames, prime_lengths, **sample_kwargs):
    """phenaki_pytorch.py:691-714 : autoregressive scene chaining with K primed frames.  sample_kwargs (cond_scale, guidance_schedule,
    negative_texts, blend, ...) go to every scene's `sample`."""
    num_scenes = len(texts)
    num_frames = cast_tuple(num_frames, num_scenes)
    prime_lengths = cast_tuple(prime_lengths, num_scenes - 1)
    prime_lengths = (*prime_lengths, 0)       # last scene needs no priming
    video_prime = None
    scenes = []
    for text, scene_num_frames, next_scene_prime_length in zip(texts, num_frames, prime_lengths):
        video = phenaki.sample(texts=text, prime_frames=video_prime, num_frames=scene_num_frames, **sample_kwargs)
        scenes.append(video)
        video_prime = video[:, :, -next_scene_prime_length:]
    return torch.cat(scenes, dim=2), scenes
