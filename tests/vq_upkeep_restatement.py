"""Plain-torch CPU restatement of the VectorQuantize upkeep (DESIGN.md "VectorQuantize upkeep"): the row choice, dead-code expiry after the EMA
update, and the spherical k-means initialisation.  Like tests/vq_train_restatement.py (whose vq_train_step does the EMA part here) the formulas
are written from memory of the published vector-quantize-pytorch module -- its randperm / randint sampling replaced by the fixed-stride choice
below -- and the tests pin the product to THESE formulas, not to upstream.

Ids are INPUTS wherever the product made them (a near-tie of an argmax never turns into a statistics mismatch); sums run in float64."""
import torch
import torch.nn.functional as F

from tests.vq_train_restatement import vq_train_step

P = 2 ** 31 - 1
EXPIRE, KMEANS = 1, 2


def pick(b, j, n):
    """((b mod n) + j P) mod n in unbounded integers: a bijection of [0, n) in j < n, wrapping evenly beyond"""
    return ((b % n) + j * P) % n


def mix(seed, call, purpose):
    """the 64-bit mix that makes b: splitmix64's finaliser chained over the three words, top 62 bits"""
    m = (1 << 64) - 1

    def fin(z):
        z = (z + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)
    return fin(fin(fin(seed & m) ^ (call & m)) ^ (purpose & m)) >> 2


def kept_rows(M, keep):
    return torch.arange(M) if keep is None else torch.nonzero(keep.bool()).flatten()


def expire(state, xn, keep, b, threshold, reset=None):
    """state: dict(cluster_size, embed_avg, embed) AFTER the EMA update; xn (M, D) f32 = the normalised rows the copies are taken from.
    -> dict(cluster_size, embed_avg, embed, expired (V,) bool, rows (n_expired,) = r(c) of the expired codes in ascending c)"""
    reset = threshold if reset is None else reset
    kept = kept_rows(xn.shape[0], keep)
    n = kept.numel()
    expired = state['cluster_size'] < threshold
    codes = torch.nonzero(expired).flatten()
    rows = torch.tensor([int(kept[pick(b, j, n)]) for j in range(codes.numel())], dtype=torch.long)
    cs, ea, e = state['cluster_size'].clone(), state['embed_avg'].clone(), state['embed'].clone()
    e[codes] = xn[rows]
    ea[codes] = xn[rows] * torch.tensor(reset, dtype=torch.float32)
    cs[codes] = reset
    return dict(cluster_size=cs, embed_avg=ea, embed=e, expired=expired, rows=rows)


def vq_upkeep_step(x, embed, embed_avg, cluster_size, keep, ids, *, threshold=0., reset=None, b=0, xn=None, stat_x=None, stat_keep=None, stat_ids=None,
                   **kw):
    """one training-mode call: vq_train_step, then expiry when threshold > 0.  stat_*: the rows the codebook statistics see when they differ from
    the call's own (every rank's rows in rank order); xn: the f32 normalised statistics rows to copy from (default F.normalize in f32)."""
    out = vq_train_step(x, embed, embed_avg, cluster_size, keep, ids, **kw)
    sx, sk, si = (x.detach(), keep, ids) if stat_x is None else (stat_x, stat_keep, stat_ids)
    if stat_x is not None:
        stat = vq_train_step(sx, embed, embed_avg, cluster_size, sk, si, **kw)
        out.update({k: stat[k] for k in ('cluster_size', 'embed_avg', 'embed', 'bins')})
    if threshold > 0:
        xn = F.normalize(sx.float(), dim=-1, eps=1e-12) if xn is None else xn
        out.update(expire(out, xn, sk, b, threshold, reset))
    return out


def kmeans(xn, keep, V, iters, b, ids=None):
    """xn (M, D) unit-norm rows, keep (M,) bool or None, ids (iters, M) int64 = the assignment of every iteration (None: the float64 argmax,
    lower index on ties) -> dict(seeds (V, D), means [iters x (V, D)], bins (V,) of the last assignment, ids (iters, M), margin [iters x (M,)] =
    the float64 top-2 margin of every row, embed, embed_avg, cluster_size = the initialised state), float64 throughout, buffers rounded to f32."""
    M = xn.shape[0]
    kept = kept_rows(M, keep)
    n = kept.numel()
    data = xn.double()
    means = data[kept[torch.tensor([pick(b, c, n) for c in range(V)])]].clone()
    seeds = means.clone()
    all_means, all_ids, margins, bins = [], [], [], None
    for it in range(iters):
        sim = data @ means.t()
        top2 = sim.topk(2, dim=-1).values
        margins.append(top2[:, 0] - top2[:, 1])
        cur = ids[it] if ids is not None else (sim == sim.max(dim=-1, keepdim=True).values).double().argmax(-1)
        kid = cur[kept]
        bins = torch.zeros(V, dtype=torch.float64).index_add_(0, kid, torch.ones(n, dtype=torch.float64))
        total = torch.zeros(V, data.shape[1], dtype=torch.float64).index_add_(0, kid, data[kept])
        new = total / total.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        means = torch.where((bins == 0)[:, None], means, new)
        all_means.append(means.clone())
        all_ids.append(cur)
    return dict(seeds=seeds.float(), means=[m.float() for m in all_means], bins=bins.long(), ids=torch.stack(all_ids), margin=margins,
                embed=means.float(), embed_avg=(means * bins[:, None]).float(), cluster_size=bins.float())
