"""Editing a region of a clip with `Phenaki.infill` on the MI355X kernels: the MaskGIT mask-predict loop regenerates part of the token grid and
keeps the rest.  Synthetic video, random weights and random text embeddings stand in for a dataset, checkpoints and the T5 encoder.

  1. outpainting     the left half of every frame is kept, the right half is generated (a pixel mask; composite=True pastes the result into the
                     original pixels, so the kept half comes back bit for bit);
  2. interpolation   the first and the last token frame are kept, everything between them is generated (a token mask; the decoded clip, all
                     frames, comes back as the tokenizer reconstructs it).

    python examples/infill_video.py [--small] [--dtype bf16] [--graph]

The kept tokens are those of the ORIGINAL clip: the tokenizer attends spatially and causally in time, so they may carry traces of the replaced
pixels -- the usual token-space inpainting."""
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
    ap.add_argument('--graph', action='store_true', help='replay the sampling loop as one captured hipGraph per configuration')
    args = ap.parse_args()
    torch.manual_seed(1)

    dim, size, patch, vocab, ctx_dim = (128, 64, 16, 256, 96) if args.small else (512, 256, 32, 65536, 768)
    depth = 2 if args.small else 6
    cvivit = P.CViViT(dim=dim, codebook_size=vocab, image_size=size, patch_size=patch, temporal_patch_size=2, spatial_depth=2 if args.small else 4,
                      temporal_depth=2 if args.small else 4, dim_head=64, heads=dim // 64, use_vgg_and_gan=False)
    maskgit = P.MaskGit(dim=dim, num_tokens=vocab, max_seq_len=1024, depth=depth, heads=dim // 64, dim_head=64, dim_context=ctx_dim)
    critic = P.TokenCritic(dim=dim, num_tokens=vocab, max_seq_len=1024, depth=depth, heads=dim // 64, dim_head=64, dim_context=ctx_dim, has_cross_attn=True)
    phenaki = P.Phenaki(cvivit=cvivit, maskgit=maskgit, critic=critic, text_embed_dim=ctx_dim).cuda().eval()
    P.set_compute_dtype(phenaki, args.dtype)
    text_embeds = torch.randn(args.batch, 12, ctx_dim, device='cuda')             # phenaki.encode_texts(texts) (t5.py) would go here
    phenaki.encode_texts = lambda texts, output_device=None: text_embeds[:len(texts)]
    texts = ['a clip'] * args.batch
    video = torch.randn(args.batch, 3, args.frames, size, size, device='cuda')    # ... and a real clip here
    phenaki.enable_sample_graph(args.graph)

    # 1. outpaint the right half: one pixel mask shared by the batch
    right = torch.zeros((1, args.frames, size, size), dtype=torch.bool)
    right[..., size // 2:] = True
    t0 = time.perf_counter()
    out = phenaki.infill(video, right, texts=texts, cond_scale=5., composite=True)
    torch.cuda.synchronize()
    kept = ~right.cuda().expand(args.batch, -1, -1, -1)[:, None].expand_as(video)
    print(f'outpaint: {tuple(out.shape)} in {time.perf_counter() - t0:.2f} s; kept pixels identical to the input: {torch.equal(out[kept], video[kept])}')

    # 2. interpolate between the first and the last token frame: a token mask over get_video_patch_shape(frames)
    f, h, w = cvivit.get_video_patch_shape(args.frames)
    between = torch.zeros((1, f, h, w), dtype=torch.bool)
    between[:, 1:f - 1] = True
    t0 = time.perf_counter()
    out, ids = phenaki.infill(video, between, mask_level='token', texts=texts, cond_scale=5., _return_ids=True)
    torch.cuda.synchronize()
    tok = phenaki.cvivit(video, return_only_codebook_ids=True)           # Phenaki holds its own eval copy of the tokenizer: that one is on the GPU
    same = torch.equal(ids.reshape(args.batch, f, h, w)[:, [0, f - 1]], tok[:, [0, f - 1]])
    print(f'interpolate: {tuple(out.shape)} in {time.perf_counter() - t0:.2f} s; {h * w * (f - 2)} of {f * h * w} tokens generated per clip; '
          f'first and last token frame kept: {same}')


if __name__ == '__main__':
    main()
