"""Float64 restatement, in torch on the CPU, of the validation statistics of a MaskGIT vocabulary head, written from their definitions (no product
code is imported): for logits l = e W^T + b of shape (M, V) and a target column per row,

    lse     = log sum_v exp(l_v)                         nll  = lse - l_target
    entropy = lse - sum_v softmax(l)_v l_v   (nats)      pred = argmax_v l_v (first maximum)
    rank    = #{v != target : l_v > l_target}            top-k accuracy = mean(rank < k)

The operands come AS THE MODE ROUNDS THEM: bf16-cast e and W for `bf16`, unrounded for `fp32` / `bf16x3` (tests/test_kernels_gpu.py builds the
reference of test_vocab_ce_matches_cross_entropy the same way).  A kernel that sums in f32 in another order moves every logit by up to
eps = rel * max|l|, so a rank is only determined up to the columns within eps of the target's logit: `rank_lo` counts the columns above t + eps,
`rank_hi` those above t - eps; where the two agree the rank is exact.  rel: 2e-5 for fp32, and for bf16 against its own rounded operands (only the
f32 accumulation order differs: the project's f32 figure), 4e-5 for bf16x3 (the project's figure for that mode)."""
import functools
import math

import torch

REL = {'fp32': 2e-5, 'bf16': 2e-5, 'bf16x3': 4e-5}
# tests.util.close tolerances of nll / lse, those of test_vocab_ce_matches_cross_entropy; bf16 is held to the 2e-5 of REL as well
CLOSE = {'fp32': 2e-5, 'bf16x3': 4e-5, 'bf16': 2e-3}


def round_operands(mode, e, W):
    """the operand values the mode's kernels multiply"""
    if mode == 'bf16':
        return e.to(torch.bfloat16).float(), W.to(torch.bfloat16).float()
    return e, W


def logits64(e, W, b):
    return e.double() @ W.double().t() + b.double()


def head_stats(logits, targets, rel):
    """logits (M, V) float64, targets (M,) int64 -> dict of (M,) tensors + eps (float)"""
    logits = logits.double()
    M, V = logits.shape
    idx = targets.reshape(M, 1)
    t = logits.gather(1, idx)
    mx = logits.max(dim=1, keepdim=True).values
    ex = torch.exp(logits - mx)
    z = ex.sum(dim=1, keepdim=True)
    lse = (mx + torch.log(z)).squeeze(1)
    entropy = lse - (ex * logits).sum(dim=1) / z.squeeze(1)
    other = torch.ones_like(logits, dtype=torch.bool).scatter_(1, idx, False)
    eps = rel * float(logits.abs().max())
    count = lambda thr: ((logits > thr) & other).sum(dim=1)
    top2 = logits.topk(2, dim=1).values
    return dict(lse=lse, nll=lse - t.squeeze(1), entropy=entropy, pred=logits.argmax(dim=1), rank=count(t), rank_lo=count(t + eps),
                rank_hi=count(t - eps), top2_gap=top2[:, 0] - top2[:, 1], eps=eps, max_abs=float(logits.abs().max()))


def pooled(stats_list, critic=None):
    """the numbers MaskGitMetrics.compute() reports, from a list of head_stats dicts (one per batch) pooled over all their rows.
    critic: optional list of (logits (b, n) float, labels (b, n) bool) per batch"""
    cat = lambda k: torch.cat([s[k].double() for s in stats_list])
    nll, ent, rank = cat('nll'), cat('entropy'), cat('rank')
    n = nll.numel()
    loss = float(nll.sum() / n)
    out = dict(tokens=n, loss=loss, perplexity=math.exp(loss), top1=float((rank < 1).sum()) / n, top5=float((rank < 5).sum()) / n,
               top10=float((rank < 10).sum()) / n, mean_rank=float(rank.sum() / n), mrr=float((1. / (rank + 1.)).sum() / n),
               entropy=float(ent.sum() / n))
    if critic is not None:
        x = torch.cat([c[0].double().reshape(-1) for c in critic])
        y = torch.cat([c[1].reshape(-1) for c in critic]).double()
        bce = (torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).sum()
        out.update(critic_bce=float(bce / x.numel()), critic_accuracy=float(((x > 0).double() == y).sum()) / x.numel(),
                   critic_positive_share=float(y.sum()) / x.numel())
    return out


# ---- the kernel-parity cases of tests/test_maskgit_metrics_gpu.py (inputs of the existing vocabulary tests, seeds written out) -----------------------

CASES = [(130, 512, 128, False),        # two row tiles with a tail, four vocabulary tiles: four XCD slices are empty
         (77, 1000, 96, True),          # V tail, K tail, row indirection into a 2M + 5 target array
         (300, 4096, 512, True),        # 32 tiles, a full W-panel
         (140, 65536, 512, True)]       # the real vocabulary
PLANT = (0, 2, 4, 5)                    # the restatement's 1st, 3rd, 5th, 6th largest column: rank 0 and both sides of the top-5 boundary


def g(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _inputs(rounded, M, V, D, with_rows):
    """inputs, targets and float64 logits of one case; computed once per rounding and shared, never modified"""
    e = torch.randn(M, D, generator=g(50))
    W = torch.randn(V, D, generator=g(51)) / math.sqrt(D) * 3
    b = torch.randn(V, generator=g(52)) * 0.1
    total = 2 * M + 5
    rows = torch.randperm(total, generator=g(53))[:M].int() if with_rows else None
    targets_full = torch.randint(0, V, (total,), generator=g(54))
    logical = rows.long() if with_rows else torch.arange(M)
    er, Wr = round_operands('bf16' if rounded else 'fp32', e, W)
    logits = logits64(er, Wr, b)
    planted = M // 2
    order = logits[:planted].argsort(dim=1, descending=True, stable=True)
    for m in range(planted):
        targets_full[logical[m]] = order[m, PLANT[m % 4]]
    targets_full[logical[planted]] = 0                                   # a target in the first column ...
    targets_full[logical[planted + 1]] = V - 1                           # ... and one in the last (at V = 1000: partial) tile
    return dict(e=e, W=W, b=b, rows=rows, targets_full=targets_full, tg=targets_full[logical], planted=planted, logits=logits)


@functools.lru_cache(maxsize=None)
def make_case(mode, M, V, D, with_rows):
    """-> dict(e, W, b (unrounded f32), rows (int32 or None), targets_full (int64), tg (per-row targets), planted (number of planted rows), logits
    (float64, of the operands as the mode rounds them), stats = head_stats of those logits with the mode's eps)"""
    c = dict(_inputs(mode == 'bf16', M, V, D, with_rows))
    c['stats'] = head_stats(c['logits'], c['tg'], REL[mode])
    return c
