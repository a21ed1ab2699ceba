"""Nucleus (top-p) and min-p filtered sampling with `Phenaki.sample`, on the MI355X kernels.  Random weights and random text embeddings stand in for
checkpoints and the T5 encoder.

A fixed top-k is wrong for a mask-predict loop: at step 0 the distribution over the codes is nearly flat and a small k throws most of it away; in the
late, peaked steps the same k still lets hundreds of near-zero-probability codes through.  The adaptive filters follow the distribution:
  top_p  keep the smallest set of most likely codes whose probability sums to top_p;
  min_p  keep the codes whose probability is at least min_p times the most likely one's.
Both are taken on softmax(logits / T) at the step's annealed temperature, the distribution the gumbel arg-max samples from, and may be combined with
one of filter_thres / top_k (order: temperature, top-k, top-p, min-p; a column is kept iff every active filter keeps it).  Exact ties at a cut are all
kept.  The confidence scores stay those of the unfiltered softmax.

    python examples/nucleus_sample.py [--small] [--dtype bf16] [--graph]

Like a top-k filter, a nucleus filter forms the logits one f32 slab of rows at a time (PK_FILTER_SLAB_MB); a call without one never does."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phenaki_pytorch_amd as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--frames', type=int, default=17)
    ap.add_argument('--dtype', default='bf16', choices=['fp32', 'bf16x3', 'bf16'])
    ap.add_argument('--small', action='store_true', help='a small geometry (dim 128, 64 x 64 pixels) instead of the BASELINE one')
    ap.add_argument('--graph', action='store_true', help='replay the sampling loop as one captured hipGraph per configuration (and per filter)')
    args = ap.parse_args()
    torch.manual_seed(1)

    dim, size, patch, vocab, ctx_dim = (128, 64, 16, 256, 96) if args.small else (512, 256, 32, 65536, 768)
    depth = 2 if args.small else 6
    cvivit = P.CViViT(dim=dim, codebook_size=vocab, image_size=size, patch_size=patch, temporal_patch_size=2, spatial_depth=2 if args.small else 4,
                      temporal_depth=2 if args.small else 4, dim_head=64, heads=dim // 64, use_vgg_and_gan=False)
    maskgit = P.MaskGit(dim=dim, num_tokens=vocab, max_seq_len=1024, depth=depth, heads=dim // 64, dim_head=64, dim_context=ctx_dim)
    phenaki = P.Phenaki(cvivit=cvivit, maskgit=maskgit, text_embed_dim=ctx_dim).cuda().eval()       # no critic: scores = 1 - p of the head
    P.set_compute_dtype(phenaki, args.dtype)
    embed = torch.randn(1, 12, ctx_dim, device='cuda')
    phenaki.encode_texts = lambda texts, output_device=None: embed.expand(len(texts), -1, -1).contiguous()
    texts = ['a fox in the snow'] * args.batch
    phenaki.enable_sample_graph(args.graph)

    def run(what, **kw):
        t0 = time.perf_counter()
        video, ids = phenaki.sample(texts=texts, num_frames=args.frames, cond_scale=5., _return_ids=True, _seed=1234, **kw)
        torch.cuda.synchronize()
        print(f'{what}: {tuple(video.shape)} in {time.perf_counter() - t0:.2f} s, {ids.unique().numel()} distinct tokens of {ids.numel()}')
        return ids

    plain = run('plain (all columns)')
    run('top_p = 0.9 (the nucleus)', top_p=0.9)
    run('min_p = 0.05', min_p=0.05)
    run('top_k = 64 with top_p = 0.9', top_k=64, top_p=0.9)
    greedy = run('top_p = 1e-6 (the arg-max of every step)', top_p=1e-6)
    top1 = run('top_k = 1', top_k=1)
    same = run('top_p = 1, min_p = 0 (both off: the plain path)', top_p=1., min_p=0.)
    print(f'both filters off equals the plain call: {bool(torch.equal(plain, same))}; the greedy nucleus equals top_k = 1: {bool(torch.equal(greedy, top1))} '
          f'and differs from the plain call at {int((greedy != plain).sum())} of {plain.numel()} positions')
    if args.graph:
        print(f'captured graphs: {len(phenaki._pk_sample_graphs)}')


if __name__ == '__main__':
    main()
