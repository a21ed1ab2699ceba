"""Times forward + backward of the masked-token cross entropy (`train._VocabCrossEntropy`: vocabulary pass, pk_vocab_ce, the slab loop of the backward) at the
benchmark's head shape, 4 608 rows x 65 536 x 512, with device events, in bf16 and bf16x3, the variants alternating in one process:

  off      label_smoothing = z_loss_weight = 0: the plain entry points, what every build launches
  eps      label_smoothing = 0.1: + pk_vocab_weight_mean (one pass over the W image) + the mean-logit dot product
  zeta     z_loss_weight = 1e-2: only arithmetic in the two kernels
  on       both
  wmean    pk_vocab_weight_mean alone

    python tools/ce_regularised_time.py [--iters 5] [--rounds 5] [--off-only]

--off-only with PK_LIB_PATH=<an older libphenaki_hip.so> times `off` on a build from before the regularisers (same box, same Python): the number the
`off` row of this build is compared with."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phenaki_pytorch_amd import _lib as L  # noqa: E402
from phenaki_pytorch_amd import train as T  # noqa: E402

M, V, D = 4608, 65536, 512


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


def measure(mode, args):
    dt = T.resolve_dtype(mode)
    g = torch.Generator(device='cuda').manual_seed(0)
    lin = torch.nn.Linear(D, V).cuda()
    with torch.no_grad():
        lin.weight.copy_(torch.randn(V, D, device='cuda', generator=g) / D ** 0.5 * 3)
    E = (torch.randn(M, D, device='cuda', generator=g)).requires_grad_()
    t = torch.randint(0, V, (M,), device='cuda', generator=g)
    head = T.linear_images(lin, dt)                   # the W and W^T images the training step hands over
    head.refresh()

    def step(reg):
        def fn():
            E.grad = lin.weight.grad = lin.bias.grad = None
            with torch.enable_grad():
                loss = T._VocabCrossEntropy.apply(E, lin.weight, lin.bias, t, None, dt, T.CE_SLAB, head.pair, None, reg)
            loss.backward()
        return fn

    variants = dict(off=step((0., 0.)))
    if not args.off_only:
        variants.update(eps=step((0.1, 0.)), zeta=step((0., 1e-2)), on=step((0.1, 1e-2)),
                        wmean=lambda: L.vocab_weight_mean(dt, head.pair[0], lin.bias.detach(), V, D))
    for fn in variants.values():                      # warm-up: allocator, images
        for _ in range(2):
            fn()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, args.iters))
    out = dict(mode=mode, shape=[M, V, D], slab=T.CE_SLAB, iters=args.iters, rounds=args.rounds, lib=os.path.basename(os.path.dirname(os.path.abspath(L.LIB_PATH))))
    for k, ts in times.items():
        out[k + '_ms'] = round(statistics.median(ts), 4)
        out[k + '_spread_ms'] = round(max(ts) - min(ts), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--off-only', action='store_true')
    args = ap.parse_args()
    torch.manual_seed(0)
    for mode in ('bf16', 'bf16x3'):
        print(json.dumps(measure(mode, args)), flush=True)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
