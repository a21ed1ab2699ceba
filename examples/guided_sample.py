"""Steering `Phenaki.sample` beyond one guidance scale, on the MI355X kernels.  Random weights and random text embeddings stand in for
checkpoints and the T5 encoder.

  1. negative prompt    guidance points away from another text's prediction instead of away from "no text";
  2. prompt blend       the conditional prediction is a weighted mix of two prompts, 70 % / 30 % (a soft scene transition);
  3. per-sample scales  every clip of the batch has its own scale, ramped up linearly over the steps (low guidance early for diversity,
                        the full scale at the last step for fidelity).

    python examples/guided_sample.py [--small] [--dtype bf16] [--graph]

All three take the table path of `sample`: the weights and scales of every step live in one small device table, so with --graph the three
calls of a kind replay one captured hipGraph whatever the numbers are."""
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
    # phenaki.encode_texts(texts) (t5.py) would go here: one embedding per distinct prompt, prompts of different lengths
    lengths = {'a fox in the snow': 12, 'a fox in a meadow': 9, 'blurry, low quality': 7}
    embeds = {t: torch.randn(1, n, ctx_dim, device='cuda') for t, n in lengths.items()}
    phenaki.encode_texts = lambda texts, output_device=None: torch.cat([embeds[t] for t in texts], dim=0)
    texts = ['a fox in the snow'] * args.batch
    phenaki.enable_sample_graph(args.graph)

    def run(what, **kw):
        t0 = time.perf_counter()
        video = phenaki.sample(texts=texts, num_frames=args.frames, **kw)
        torch.cuda.synchronize()
        print(f'{what}: {tuple(video.shape)} in {time.perf_counter() - t0:.2f} s, finite: {bool(torch.isfinite(video).all())}')
        return video

    run('negative prompt', cond_scale=5., negative_texts='blurry, low quality')
    run('blend 70 / 30', cond_scale=5., blend=[('a fox in a meadow', 0.3)])
    scales = [3. + 4. * b / max(args.batch - 1, 1) for b in range(args.batch)]
    run(f'per-sample scales {scales}, linear schedule', cond_scale=scales, guidance_schedule='linear')
    if args.graph:
        run('per-sample scales again, other numbers (replays the same graph)', cond_scale=[2.] * args.batch, guidance_schedule='linear')
        print(f'captured graphs: {len(phenaki._pk_sample_graphs)}')


if __name__ == '__main__':
    main()
