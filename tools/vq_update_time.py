"""Time the EMA codebook update of the VectorQuantize training step at the real size: python tools/vq_update_time.py [V D M]
(default 65536 512 4608).  pk_vq_codebook_update is a pure stream -- read embed_avg, write embed_avg and embed, 3 V D 4 bytes -- so its time is
reported with the implied TB/s; the whole chain (zero counts, hist, scan, fill, update) is timed beside it.  Device events, warmed up.
Upkeep (a library that has the entry points): the same chain with dead-code expiry enabled -- cluster_size is re-drawn uniform in [0, 2) before
every launch of it, so a threshold of 1 expires about half of the codes, every time -- and one k-means iteration (lookup, hist,
scan, fill, pk_vq_kmeans_means) on the same rows."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phenaki_pytorch_amd import _lib as L  # noqa: E402

V, D, M = (int(a) for a in sys.argv[1:4]) if len(sys.argv) >= 4 else (65536, 512, 4608)
dev = 'cuda'
g = torch.Generator().manual_seed(0)
xn = torch.nn.functional.normalize(torch.randn(M, D, generator=g), dim=-1).to(dev)
ids = torch.randint(0, V, (M,), generator=g).to(dev)
embed = torch.nn.functional.normalize(torch.randn(V, D, generator=g), dim=-1).to(dev)
embed_avg, cluster_size = embed.clone(), torch.ones(V, device=dev)
lib, st, p = L.load(), L.stream(xn), L.ptr
counts = L.vq_ema_update(xn, ids, None, cluster_size, embed_avg, embed, 0.8, 1e-5)       # also leaves a sorted row list to re-run the last kernel on
offsets, cursor, rows, S = torch.empty_like(counts), torch.empty_like(counts), torch.empty(M, device=dev, dtype=torch.int32), torch.empty(1, device=dev)
assert lib.pk_vq_scan(p(counts), V, 1.0, p(cluster_size), p(offsets), p(cursor), p(S), st) == 0            # decay 1: cluster_size unchanged
assert lib.pk_vq_fill(p(ids), None, M, V, p(cursor), p(rows), st) == 0


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def update():
    assert lib.pk_vq_codebook_update(p(xn), p(counts), p(offsets), p(rows), p(cluster_size), p(S), M, V, D, 1.0, 1e-5, p(embed_avg), p(embed), st) == 0


us = timed(update)
chain = timed(lambda: L.vq_ema_update(xn, ids, None, cluster_size, embed_avg, embed, 1.0, 1e-5))
nbytes = 3 * V * D * 4 + M * D * 4                                           # the codebook stream + the M rows of xn
out = dict(kernel='pk_vq_codebook_update', V=V, D=D, M=M, codes_hit=int((counts > 0).sum()), us=round(us, 2), bytes=nbytes,
           tb_per_s=round(nbytes / us / 1e6, 3), ema_chain_us=round(chain, 2))
if hasattr(L, 'vq_ema_update_expire'):
    sizes = 2. * torch.rand(V, generator=g).to(dev)
    keep = (torch.rand(M, generator=g) > 1. / 3.).to(dev).to(torch.uint8)

    def expire(mask):
        cluster_size.copy_(sizes)                                            # (5 us of its own, timed below and subtracted)
        return L.vq_ema_update_expire(xn, ids, mask, cluster_size, embed_avg, embed, 1.0, 1e-5, 1.0, 1.0, 12345)

    refill = timed(lambda: cluster_size.copy_(sizes))
    _, jrank = expire(None)
    out.update(expired=int((jrank >= 0).sum()), ema_chain_expire_us=round(timed(lambda: expire(None)) - refill, 2),
               ema_chain_expire_masked_us=round(timed(lambda: expire(keep)) - refill, 2))
    # one k-means iteration = vq_kmeans(iters = 1) minus its seeding launch, timed alone
    from phenaki_pytorch_amd.quantize import VectorQuantize
    vq = VectorQuantize(dim=D, codebook_size=V)
    means = embed.clone()
    seed_us = timed(lambda: lib.pk_vq_pick_rows(p(xn), None, None, M, V, D, 12345, p(means), st))
    iter_us = timed(lambda: L.vq_kmeans(xn, None, means, 1, 12345, vq.ids_of_normalised), reps=20) - seed_us
    look_us = timed(lambda: vq.ids_of_normalised(xn, means), reps=20)
    out.update(kmeans_iter_us=round(iter_us, 2), kmeans_lookup_us=round(look_us, 2))
print(json.dumps(out))
