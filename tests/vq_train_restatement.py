"""Plain-torch CPU restatement of one training-mode call of the cosine-sim VectorQuantize (DESIGN.md "VectorQuantize training"): straight-through
output, commitment loss, EMA codebook update.  The formulas are written from memory of the published vector-quantize-pytorch module
(use_cosine_sim=True, one head, no projections, decay 0.8, eps 1e-5, commitment_weight 1, no k-means init, no dead-code expiry); the package
is absent, so the tests pin the product to THESE formulas, not to upstream.

The ids are an INPUT (the product's own), so a near-tie of the argmax never turns into a statistics mismatch.  Sums run in float64."""
import torch
import torch.nn.functional as F


def vq_train_step(x, embed, embed_avg, cluster_size, keep, ids, *, decay=0.8, eps=1e-5, commitment_weight=1.0):
    """x (M, D) f32 (may require grad), embed / embed_avg (V, D), cluster_size (V,), keep (M,) bool or None, ids (M,) int64 ->
    dict(y, commit, cluster_size, embed_avg, embed, bins): y has the value embed[ids] and the gradient dx = dy; commit is differentiable in x;
    the three buffers are the state AFTER the update (inputs are left unchanged)."""
    M, D = x.shape
    V = embed.shape[0]
    keep = torch.ones(M, dtype=torch.bool) if keep is None else keep.bool()
    n_keep = int(keep.sum())
    if n_keep == 0:
        raise ValueError('the mask keeps no row')
    q = embed[ids].detach()
    y = q + (x - x.detach())                                       # value: q exactly (x - x = 0); gradient: straight through
    commit = commitment_weight * ((q.double() - x.double())[keep] ** 2).sum() / (n_keep * D)
    xn = F.normalize(x.detach().double(), dim=-1, eps=1e-12)
    kept_ids = ids[keep]
    bins = torch.zeros(V, dtype=torch.float64).index_add_(0, kept_ids, torch.ones(n_keep, dtype=torch.float64))
    total = torch.zeros(V, D, dtype=torch.float64).index_add_(0, kept_ids, xn[keep])
    cs = decay * cluster_size.double() + (1 - decay) * bins
    ea = decay * embed_avg.double() + (1 - decay) * total
    S = cs.sum()
    smoothed = (cs + eps) / (S + V * eps) * S
    e = ea / smoothed[:, None]
    e = e / e.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return dict(y=y, commit=commit.float(), cluster_size=cs.float(), embed_avg=ea.float(), embed=e.float(), bins=bins.long())
