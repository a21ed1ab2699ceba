"""Times the validation pass of the vocabulary head, L.vocab_eval (pk_vocab_eval + pk_vocab_eval_reduce: arg-max, lse, nll, rank, entropy without
the logits), at the benchmark's head shape -- 4 608 and 1 152 rows x 65 536 tokens x 512 -- in each compute dtype, with device events, the variants
alternating in one process, against two yardsticks:

  sample+ce     vocab_sample(need_lse) + vocab_ce on the tiled kernel (PK_VOCAB_RESIDENT=0): what the training objective's VALUE costs today and the
                closest existing pass (same main loop, the noise-drawing epilogue; it yields lse and nll but neither rank nor entropy).  With
                --parent-lib PATH the two calls go to a libphenaki_hip.so built from the parent commit; without it to this tree's library, whose
                sampling kernels this change leaves as they were.
  torch         torch's own formulation on the same device, f32 and bf16: mm -> log_softmax -> gather for the nll, compare-and-sum for the rank,
                -(p * logp).sum for the entropy, argmax; it writes the (rows, 65 536) logits.

Operands are COLD: every call reads the next of `copies` copies of W and A, enough of them to exceed the 256 MB last-level cache between two uses
of the same copy.  Writes the table to --out.

    python tools/maskgit_metrics_time.py [--iters 20] [--rounds 3] [--parent-lib tools/_bin/libphenaki_hip_parent.so]
"""
import argparse
import ctypes
import math
import os
import statistics
import sys

os.environ['PK_VOCAB_RESIDENT'] = '0'            # the tiled kernel for the sampling yardstick (read once, when a library launches first)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phenaki_pytorch_amd import _lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, D = 65536, 512
ROWS = (4608, 1152)
COLD_BYTES = 600e6


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


def parent_library(path):
    lib = ctypes.CDLL(path)
    for name in ('pk_vocab_sample', 'pk_vocab_ce'):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = L.SIGNATURES[name], ctypes.c_int
    return lib


class Rotation:
    """`copies` device copies of a tensor, handed out in turn"""

    def __init__(self, t, copies):
        self.items, self.i = [t] + [t.clone() for _ in range(copies - 1)], 0

    def next(self):
        self.i = (self.i + 1) % len(self.items)
        return self.items[self.i]


def torch_stats(A, W, bias, tg):
    logits = torch.addmm(bias.to(A.dtype), A, W.t())
    logp = torch.log_softmax(logits.float(), dim=-1)
    t = logits.gather(1, tg[:, None])
    nll = -logp.gather(1, tg[:, None]).squeeze(1)
    rank = (logits > t).sum(dim=-1)
    entropy = -(logp.exp() * logp).sum(dim=-1)
    return logits.argmax(dim=-1), nll, rank, entropy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-lib', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'maskgit_metrics_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    parent = parent_library(args.parent_lib) if args.parent_lib else None
    g = torch.Generator(device='cuda').manual_seed(0)
    W32 = torch.randn(V, D, device='cuda', generator=g) / math.sqrt(D) * 3
    bias = torch.randn(V, device='cuda', generator=g) * 0.1
    lines = [f'Validation pass of the vocabulary head at rows x {V} x {D}, tools/maskgit_metrics_time.py --iters {args.iters} --rounds {args.rounds}',
             f'device: {torch.cuda.get_device_name(0)}; ms per call, median of {args.rounds} rounds of {args.iters} back-to-back calls between device events, the',
             'variants alternating, cold operands (rotating copies of A and W); sample+ce = vocab_sample(need_lse) + vocab_ce on the tiled kernel',
             '(PK_VOCAB_RESIDENT=0) of ' + ('the PARENT commit\'s library' if parent else 'this tree\'s library (sampling kernels unchanged by this change)')
             + '; torch = mm -> log_softmax -> gather / compare-and-sum', '',
             f'  {"rows":>5s} {"dtype":<7s} {"vocab_eval":>11s} {"sample+ce":>11s} {"torch":>11s}   eval / sample+ce   eval vs torch   spread (eval, sample+ce)']
    notes = []
    with torch.no_grad():
        for M in ROWS:
            A32 = torch.randn(M, D, device='cuda', generator=g)
            tg = torch.randint(0, V, (M,), device='cuda', generator=g)
            for mode, dt in (('bf16', L.BF16), ('bf16x3', L.BF16X3), ('fp32', L.F32)):
                td = L.tdtype(dt)
                Wd = L.split_planes(W32) if mode == 'bf16x3' else W32.to(td)
                copies = int(COLD_BYTES // (Wd.numel() * Wd.element_size())) + 2
                Ws, As = Rotation(Wd, copies), Rotation(A32.to(td), copies)
                f32 = lambda: torch.empty(M, device='cuda')
                out = dict(pred=torch.empty(M, device='cuda', dtype=torch.long), lse=f32(), nll=f32(), rank=torch.empty(M, device='cuda', dtype=torch.int32),
                           entropy=f32())
                work = torch.empty(L.vocab_eval_words(M, V), device='cuda')
                partials = torch.empty(5 * L.vocab_ntiles(V) * M, device='cuda')
                loss, lse = f32(), f32()

                def new():
                    L.vocab_eval(dt, As.next(), Ws.next(), bias, M, V, D, tg, None, workspace=work, **out)

                def old():
                    a, w = As.next(), Ws.next()
                    if parent is None:
                        L.vocab_sample(dt, a, w, bias, M, V, D, 1.0, None, None, 7, True, partials)
                        L.vocab_ce(dt, partials, M, V, a, w, bias, D, tg, None, loss, lse)
                        return
                    s = L.stream(a)
                    rc = parent.pk_vocab_sample(dt, a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), bias.data_ptr(), M, V, D, 1.0, None, None, 7, None, 1,
                                                partials.data_ptr(), s)
                    rc = rc or parent.pk_vocab_ce(dt, partials.data_ptr(), M, V, a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), bias.data_ptr(), D,
                                                  tg.data_ptr(), None, loss.data_ptr(), lse.data_ptr(), s)
                    assert rc == 0, f'parent library: error {rc}'

                variants = dict(new=new, old=old)
                if mode != 'bf16x3':                                       # torch has no split-bf16 product: its two columns are bf16 and f32
                    Wt, At = Rotation(W32.to(td), copies), Rotation(A32.to(td), copies)
                    variants['torch'] = lambda: torch_stats(At.next(), Wt.next(), bias, tg)
                ref = None
                for k, fn in variants.items():                             # warm-up: code objects, the mm algorithm, the allocator
                    for _ in range(3):
                        r = fn()
                    if k == 'torch':
                        ref = r
                times = {k: [] for k in variants}
                for _ in range(args.rounds):
                    for k, fn in variants.items():
                        times[k].append(timed(fn, args.iters))
                med = {k: statistics.median(ts) for k, ts in times.items()}
                spread = {k: max(ts) - min(ts) for k, ts in times.items()}
                tcol = f'{med["torch"]:11.4f}' if 'torch' in med else f'{"-":>11s}'
                vs_t = f'{med["torch"] / med["new"]:10.2f}x' if 'torch' in med else f'{"-":>11s}'
                lines.append(f'  {M:5d} {mode:<7s} {med["new"]:11.4f} {med["old"]:11.4f} {tcol}   {med["new"] / med["old"]:16.3f} {vs_t}     {spread["new"]:.4f}, {spread["old"]:.4f}')
                agree = f'{M} {mode}: max |nll - sample+ce| / max = {float((out["nll"] - loss).abs().max() / loss.abs().max()):.2e}'
                if ref is not None:
                    agree += (f'; against torch: nll {float((out["nll"] - ref[1]).abs().max() / ref[1].abs().max()):.2e} rel, entropy '
                              f'{float((out["entropy"] - ref[3]).abs().max()):.2e} abs, rank equal on {float((out["rank"] == ref[2]).float().mean()):.4f} of the rows, '
                              f'pred on {float((out["pred"] == ref[0]).float().mean()):.4f}')
                notes.append('  ' + agree)
                del Ws, As, variants
                torch.cuda.empty_cache()
    lines += ['', 'agreement of the outputs (torch rounds its logits to the dtype; ranks within rounding of a tie may differ):'] + notes
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
