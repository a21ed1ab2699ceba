"""Top-k filtered sampling with `Phenaki.sample`, on the MI355X kernels.  Random weights and random text embeddings stand in for checkpoints and
the T5 encoder.

With an untrained or lightly trained MaskGit the tail of a 65 536-wide softmax takes a large share of the draws at the early, hot steps.
`filter_thres` (the convention of the MaskGIT-family samplers: 0.9 keeps the top 10 % of the vocabulary) or `top_k` (a column count) cuts it: every
draw comes from the columns whose logit reaches the row's k-th largest.  The confidence scores stay those of the unfiltered softmax.

    python examples/filtered_sample.py [--small] [--dtype bf16] [--graph]

The plain call never forms the logits; a filtered one does, one f32 slab of rows at a time (PK_FILTER_SLAB_MB), so it costs a write and a read of
that slab per step on top of the head."""
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
    ap.add_argument('--graph', action='store_true', help='replay the sampling loop as one captured hipGraph per configuration (and per k)')
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
    run('filter_thres = 0.9 (top 10 %)', filter_thres=0.9)
    run(f'top_k = {max(vocab // 1024, 2)}', top_k=max(vocab // 1024, 2))
    greedy = run('top_k = 1 (the arg-max of every step)', top_k=1)
    same = run('filter_thres = 0 (keeps everything: the plain path)', filter_thres=0.)
    print(f'filter_thres = 0 equals the plain call: {bool(torch.equal(plain, same))}; top_k = 1 differs from it at '
          f'{int((greedy != plain).sum())} of {plain.numel()} positions')
    if args.graph:
        print(f'captured graphs: {len(phenaki._pk_sample_graphs)}')


if __name__ == '__main__':
    main()
