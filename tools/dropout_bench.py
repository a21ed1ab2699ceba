"""Training-step time of Phenaki.forward with and without dropout (BASELINE geometry: dim 512, depth 6 + 6, 576 tokens per video, batch 8):

    python tools/dropout_bench.py [--p 0.1] [--dtypes bf16x3,bf16] [--batch 8] [--groups 5]

One JSON line per (dtype, p): zero_grad + forward + backward + AdamW, median over `groups` timed groups of 3 steps (the train_step leg of bench.py
builds the same step; this script adds attn_dropout = ff_dropout = p).  profiles/train_dropout.txt keeps the numbers.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phenaki_pytorch_amd as P  # noqa: E402


def step_time(dtype, p, batch, groups):
    torch.manual_seed(0)
    kw = dict(dim=512, num_tokens=65536, max_seq_len=1024, depth=6, heads=8, dim_head=64, dim_context=768, attn_dropout=p, ff_dropout=p)
    cv = P.CViViT(dim=512, codebook_size=65536, image_size=256, patch_size=32, temporal_patch_size=2, spatial_depth=4, temporal_depth=4, dim_head=64,
                  heads=8, use_vgg_and_gan=False)
    mg, cr = P.MaskGit(**kw), P.TokenCritic(has_cross_attn=True, **kw)
    ph = P.Phenaki(cvivit=cv, maskgit=mg, critic=cr, text_embed_dim=768).cuda()
    P.set_compute_dtype(ph, dtype)
    mg.train()
    cr.train()
    params = list(mg.parameters()) + list(cr.parameters())
    opt = P.get_optimizer(params, lr=1e-4, wd=1e-2)
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 65536, (batch, 9, 8, 8), generator=g).cuda()
    ctx = torch.randn(batch, 12, 768, generator=g).cuda()

    def step():
        opt.zero_grad(set_to_none=True)
        loss = ph(video_codebook_ids=ids, text_embeds=ctx)
        loss.backward()
        opt.step()
        return loss

    for _ in range(3):
        loss = step()
    ts = []
    for _ in range(groups):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            loss = step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / 3)
    out = dict(dtype=dtype, p=p, batch=batch, ms_per_step=statistics.median(ts) * 1e3, ms_min=min(ts) * 1e3, ms_max=max(ts) * 1e3, loss=float(loss.detach()))
    del ph, mg, cr, cv, opt
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--p', type=float, default=0.1)
    ap.add_argument('--dtypes', default='bf16x3,bf16')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--groups', type=int, default=5)
    args = ap.parse_args()
    with torch.enable_grad():
        for dtype in args.dtypes.split(','):
            for p in (0., args.p):
                print(json.dumps(step_time(dtype, p, args.batch, args.groups)), flush=True)


if __name__ == '__main__':
    main()
