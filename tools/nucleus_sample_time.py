"""Times the nucleus / min-p filtered vocabulary head (pk_logits_nucleus_sample, _lib.vocab_sample_nucleus) next to its yardstick, the top-k select
(pk_logits_topk_sample), in one process on one device, with device events, the arms alternating (the method of tools/filtered_sample_time.py):

  1. the kernel alone on one slab of 256 / 512 / 1024 rows x 65 536 f32 logits: top_p = 0.9; min_p = 0.05; k = 6 553 with top_p = 0.9; the yardstick
     pk_logits_topk_sample at k = 6 553 and, for the floor, at k = V (no select);
  2. a B = 8, 18-step Phenaki.sample(top_p=0.9) against the plain call and against filter_thres=0.9 at the benchmark's geometry (random weights,
     hipGraph off and on).

No time here is a pass / fail criterion: the filters are opt-in and the plain path is untouched.  Writes the table to --out.

    python tools/nucleus_sample_time.py [--iters 10] [--rounds 5] [--no-e2e]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phenaki_pytorch_amd as P  # noqa: E402
from filtered_sample_time import measure  # noqa: E402
from phenaki_pytorch_amd import _lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 65536
K = max(int((1 - 0.9) * V), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-e2e', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nucleus_sample_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    torch.set_grad_enabled(False)
    g = torch.Generator(device='cuda').manual_seed(0)
    lines = [f'Nucleus / min-p filtered vocabulary head, tools/nucleus_sample_time.py --iters {args.iters} --rounds {args.rounds}',
             f'device: {torch.cuda.get_device_name(0)}; ms per call, median of {args.rounds} rounds of {args.iters} back-to-back calls between device events, the arms',
             'alternating in one process; spread = max - min over the rounds', '']

    # 1. the kernel alone
    arms = (('topk k=6553 (yardstick)', None), ('topk k=V (no select)', None), ('top_p=0.9', (V, 0.9, 0.)), ('min_p=0.05', (V, 1., 0.05)),
            ('k=6553 top_p=0.9', (K, 0.9, 0.)), ('top_p=1 min_p=0 k=6553', (K, 1., 0.)))
    lines += ['1. pk_logits_nucleus_sample alone on one slab of f32 logits (V = 65 536, randn * 3, T = 0.7, counter-hash noise, with the log-sum-exp);',
              '   x = the time over pk_logits_topk_sample at k = 6 553 in the same run',
              f'  {"rows":>5s} {"arm":<26s} {"ms":>9s} {"spread":>8s} {"x":>6s}']
    for rows in (256, 512, 1024):
        slab = torch.randn(rows, V, device='cuda', generator=g) * 3
        pred = torch.empty(rows, device='cuda', dtype=torch.long)
        scores = torch.empty(rows, device='cuda')
        variants = {}
        for name, f in arms:
            if f is None:
                k = K if '6553' in name else V
                variants[name] = (lambda k: lambda: L.logits_topk_sample(slab, rows, V, k, 0.7, None, None, 0, 7, True, None, None, pred, scores))(k)
            else:
                variants[name] = (lambda f: lambda: L.logits_nucleus_sample(slab, rows, V, f[0], f[1], f[2], 0.7, None, None, 0, 7, True, None, None, pred,
                                                                            scores))(f)
        med, spread = measure(variants, args.iters, args.rounds)
        for name, _ in arms:
            lines.append(f'  {rows:5d} {name:<26s} {med[name]:9.4f} {spread[name]:8.4f} {med[name] / med[arms[0][0]]:6.2f}')
            print(lines[-1], flush=True)
        del slab
    lines.append('')

    # 2. end to end
    if not args.no_e2e:
        torch.manual_seed(1)
        cv = P.CViViT(dim=512, codebook_size=V, image_size=256, patch_size=32, temporal_patch_size=2, spatial_depth=4, temporal_depth=4, dim_head=64, heads=8,
                      use_vgg_and_gan=False)
        mg = P.MaskGit(dim=512, num_tokens=V, max_seq_len=1024, depth=6, heads=8, dim_head=64, dim_context=768)
        cr = P.TokenCritic(dim=512, num_tokens=V, max_seq_len=1024, depth=6, heads=8, dim_head=64, dim_context=768, has_cross_attn=True)
        ph = P.Phenaki(cvivit=cv, maskgit=mg, critic=cr, text_embed_dim=768, steps=18).cuda().eval()
        P.set_compute_dtype(ph, 'bf16')
        ctx = torch.randn(8, 12, 768, device='cuda')
        ph.encode_texts = lambda texts, output_device=None: ctx
        kw = dict(texts=['x'] * 8, num_frames=17, cond_scale=5.)
        lines += ['2. Phenaki.sample, B = 8, 17 frames (n = 576), 18 steps, bf16, TokenCritic, cond_scale 5, random weights; ms per call',
                  f'  {"mode":<8s} {"plain":>10s} {"filter_thres=0.9":>17s} {"top_p=0.9":>10s} {"top_p / plain":>14s} {"top_p / top-k":>14s}   spread (plain, top-k, top_p)']
        for graph in (False, True):
            ph.enable_sample_graph(graph)
            med, spread = measure(dict(plain=lambda: ph.sample(**kw), filt=lambda: ph.sample(filter_thres=0.9, **kw), nuc=lambda: ph.sample(top_p=0.9, **kw)),
                                  max(args.iters // 5, 2), args.rounds)
            lines.append(f'  {"hipGraph" if graph else "eager":<8s} {med["plain"]:10.2f} {med["filt"]:17.2f} {med["nuc"]:10.2f} {med["nuc"] / med["plain"]:13.3f}x '
                         f'{med["nuc"] / med["filt"]:13.3f}x   {spread["plain"]:.2f}, {spread["filt"]:.2f}, {spread["nuc"]:.2f}')
            print(lines[-1], flush=True)
        ph.enable_sample_graph(False)
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
