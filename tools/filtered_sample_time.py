"""Times the top-k filtered vocabulary head (pk_gemm into an f32 logits slab + pk_logits_topk_sample, _lib.vocab_sample_filtered) next to its yardstick,
the unfiltered head (pk_vocab_sample + pk_vocab_reduce), in one process on one device, with device events, the arms alternating:

  1. the select kernel alone on one slab of rows x 65 536 f32 logits (k = 6 553, the filter_thres = 0.9 default of the sibling samplers, and k = 1);
  2. the filtered head against the plain head at 4 608 and 9 216 rows x 65 536 x 512 in bf16, for slabs of 64, 128 and 256 MB (PK_FILTER_SLAB_MB);
  3. a B = 8, 18-step Phenaki.sample(filter_thres=0.9) against the plain call at the benchmark's geometry (random weights, hipGraph off and on).

No time here is a pass / fail criterion: the filter is opt-in and the plain path is untouched.  Writes the table to --out.

    python tools/filtered_sample_time.py [--iters 10] [--rounds 5] [--no-e2e]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phenaki_pytorch_amd as P  # noqa: E402
from phenaki_pytorch_amd import _lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, D = 65536, 512
ROWS = (4608, 9216)
SLABS_MB = (64, 128, 256)
K = max(int((1 - 0.9) * V), 1)


def timed(fn, iters):
    """ms per call: `iters` back-to-back calls between two device events"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def measure(variants, iters, rounds, warm=2):
    for fn in variants.values():
        for _ in range(warm):
            fn()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    return {k: statistics.median(ts) for k, ts in times.items()}, {k: max(ts) - min(ts) for k, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-e2e', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'filtered_sample_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    torch.set_grad_enabled(False)
    g = torch.Generator(device='cuda').manual_seed(0)
    lines = [f'Top-k filtered vocabulary head, tools/filtered_sample_time.py --iters {args.iters} --rounds {args.rounds}',
             f'device: {torch.cuda.get_device_name(0)}; ms per call, median of {args.rounds} rounds of {args.iters} back-to-back calls between device events, the arms',
             'alternating in one process; spread = max - min over the rounds', '']

    # 1. the select kernel alone
    lines += ['1. pk_logits_topk_sample alone on one slab of f32 logits (V = 65 536, counter-hash noise, with the log-sum-exp)',
              f'  {"rows":>5s} {"k":>6s} {"ms":>9s} {"spread":>8s} {"GB/s (one read of the slab)":>28s}']
    for rows in (256, 512, 1024):
        slab = torch.randn(rows, V, device='cuda', generator=g) * 3
        pred = torch.empty(rows, device='cuda', dtype=torch.long)
        scores = torch.empty(rows, device='cuda')
        for k in (K, 1, V):
            med, spread = measure(dict(sel=lambda: L.logits_topk_sample(slab, rows, V, k, 0.7, None, None, 0, 7, True, None, None, pred, scores)),
                                  args.iters, args.rounds)
            lines.append(f'  {rows:5d} {k:6d} {med["sel"]:9.4f} {spread["sel"]:8.4f} {rows * V * 4 / med["sel"] / 1e6:28.0f}')
            print(lines[-1], flush=True)
        del slab
    lines.append('')

    # 2. the filtered head against the plain head
    W32 = torch.randn(V, D, device='cuda', generator=g) / math.sqrt(D) * 3
    Wd = W32.to(torch.bfloat16)
    bias = torch.randn(V, device='cuda', generator=g) * 0.1
    lines += [f'2. the head at rows x {V} x {D}, bf16, k = {K}: plain = pk_vocab_sample(need_lse) + pk_vocab_reduce; filtered = per slab pk_gemm (f32 out) +',
              '   pk_logits_topk_sample',
              f'  {"rows":>5s} {"plain":>9s} ' + ' '.join(f'{f"slab {mb} MB":>12s}' for mb in SLABS_MB) + '   filtered / plain     spread (plain, filtered...)']
    best = {}
    for M in ROWS:
        A = torch.randn(M, D, device='cuda', generator=g).to(torch.bfloat16)
        partials = torch.empty(5 * L.vocab_ntiles(V) * M, device='cuda')
        pred = torch.empty(M, device='cuda', dtype=torch.long)
        ids = torch.zeros(M, device='cuda', dtype=torch.long)
        mask = torch.ones(M, device='cuda', dtype=torch.uint8)
        scores = torch.empty(M, device='cuda')
        slabs = {mb: torch.empty(((mb << 20) // (4 * V), V), device='cuda') for mb in SLABS_MB}

        def plain():
            L.vocab_sample(L.BF16, A, Wd, bias, M, V, D, 0.7, None, None, 7, True, partials)
            L.vocab_reduce(partials, M, V, None, mask, ids, pred, scores, True)

        variants = dict(plain=plain)
        for mb in SLABS_MB:
            variants[mb] = (lambda s: lambda: L.vocab_sample_filtered(L.BF16, A, Wd, bias, M, V, D, K, 0.7, None, None, 7, True, mask, ids, pred, scores, s))(slabs[mb])
        med, spread = measure(variants, args.iters, args.rounds)
        best[M] = min(SLABS_MB, key=lambda mb: med[mb])
        lines.append(f'  {M:5d} {med["plain"]:9.4f} ' + ' '.join(f'{med[mb]:12.4f}' for mb in SLABS_MB) + '   ' +
                     ' '.join(f'{med[mb] / med["plain"]:5.2f}x' for mb in SLABS_MB) + '   ' + ', '.join(f'{spread[k]:.4f}' for k in variants))
        print(lines[-1], flush=True)
        del slabs, partials, A
        torch.cuda.empty_cache()
    lines += [f'  fastest slab: ' + ', '.join(f'{M} rows: {mb} MB' for M, mb in best.items()) + f'; the default in _lib.FILTER_SLAB_MB is {L.FILTER_SLAB_MB}', '']
    del W32, Wd

    # 3. end to end
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
        lines += ['3. Phenaki.sample, B = 8, 17 frames (n = 576), 18 steps, bf16, TokenCritic, cond_scale 5, random weights; ms per call',
                  f'  {"mode":<8s} {"plain":>10s} {"filter_thres=0.9":>17s} {"ratio":>7s}   spread (plain, filtered)']
        for graph in (False, True):
            ph.enable_sample_graph(graph)
            med, spread = measure(dict(plain=lambda: ph.sample(**kw), filt=lambda: ph.sample(filter_thres=0.9, **kw)), max(args.iters // 5, 2), args.rounds)
            lines.append(f'  {"hipGraph" if graph else "eager":<8s} {med["plain"]:10.2f} {med["filt"]:17.2f} {med["filt"] / med["plain"]:6.3f}x   '
                         f'{spread["plain"]:.2f}, {spread["filt"]:.2f}')
            print(lines[-1], flush=True)
        ph.enable_sample_graph(False)
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
