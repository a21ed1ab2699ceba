"""A/B of the A-resident FF1 kernel (csrc/gemm_resident.hpp, pk_set_ff1_resident) against the tiled kernel of the same build, in one process:

    python tools/ff1_resident_ab.py [--rows 4608 2304 9216] [--rounds 7] [--steps 60] [--reps 20] [--call-replays 500] [--captures 3] > ff1_resident_ab.txt

1. per call: the FF1 call of a bf16 transformer block with the operands attention.py gives it (LayerNorm fold from to_out's row statistics, GEGLU,
   bf16 C) at every --rows value.  `resident` is pk_set_ff1_resident(2) -- the resident kernel at any M, so rows outside the shipped window can be
   probed; `tiled` is 0.  Every setting is one hipGraph of `reps` launches; the settings are timed in interleaved rounds of `call-replays` replays
   after one round that is thrown away.  The two settings' outputs must be the same bytes, and the launch counter must show which kernel ran.
2. whole step: the C-ViViT encode exactly as bench.py runs it (three rotating videos, one hipGraph per video), switch 1 (the shipped dispatch)
   against 0.  A captured graph keeps the kernel it was captured with; every setting is captured `captures` times, all graphs are timed in
   interleaved rounds of `steps` replays; the token ids of every graph equal the switch-off eager ids.
Verdict per line: the project's keep rule -- a setting wins only if its median is lower by more than the larger min-max spread."""
import argparse
import itertools
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_models, capture, synthetic_video  # noqa: E402
from phenaki_pytorch_amd import _lib as L  # noqa: E402
from phenaki_pytorch_amd import attention as A  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, nargs='+', default=[4608, 2304, 9216])
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--steps', type=int, default=60)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--captures', type=int, default=3)
ap.add_argument('--call-replays', type=int, default=500, help='replays of the per-call graph in one timed round')
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--skip-step', action='store_true')
args = ap.parse_args()
torch.set_grad_enabled(False)
L.set_cache_policy(L.get_cache_policy() & ~(3 | (3 << 16)))       # the GEMM sites plain, as in the default build


def timed(replay, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        replay()
    e0.record()
    for _ in range(n):
        replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def verdict(a, b):
    """a against b (lists of us): (delta of medians, 'WINS' | 'loses' | 'within noise')"""
    d = statistics.median(a) - statistics.median(b)
    spread = max(max(a) - min(a), max(b) - min(b))
    return d, ('WINS' if -d > spread else ('loses' if d > spread else 'within noise'))


def line(name, t):
    return f'  {name:28s} {statistics.median(t):8.2f} {min(t):8.2f} {max(t):8.2f}'


# ---------------------------------------------------------------------------------------------- 1. per call
D, dt = 512, L.BF16
dev = torch.device('cuda')
attn, ff = A.Attention(D, heads=8).to(dev), A.FeedForward(D).to(dev)
w1g, s1, t1, _ = ff._packed_folded(dt)
ip = ff._packed(dt)[2]
print(f'# 1. FF1 per call, N = {2 * ip}, K = {D}, bf16; us per launch, one hipGraph of {args.reps} launches per setting, {args.rounds} interleaved rounds of '
      f'{args.call_replays} replays; outputs byte-identical')
print(f'# {"rows / setting":28s} {"median":>8s} {"min":>8s} {"max":>8s}   resident - tiled, verdict')
for M in args.rows:
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(M, D, generator=gen).to(dev)
    o = torch.randn(M, D, generator=gen).to(dev).to(torch.bfloat16)
    out, out_t, stats = attn._finish(o, x, dt, 'stats')
    hmid = {s: torch.empty((M, ip), device=dev, dtype=torch.bfloat16) for s in ('resident', 'tiled')}
    graphs = {}
    for setting, mode in (('resident', 2), ('tiled', 0)):
        L.set_ff1_resident(mode)
        fn = lambda c=hmid[setting]: L.gemm(dt, out_t, w1g, M, 2 * ip, D, C=c, act=L.ACT_GEGLU, ln=(s1, t1, ff[0].eps), ln_stats=stats)
        before = L.ff1_resident_launches()
        fn()
        assert L.ff1_resident_launches() - before == (1 if mode else 0), f'M = {M}, {setting}: the other kernel ran'

        def many(fn=fn):
            for _ in range(args.reps):
                fn()
        graphs[setting] = capture(many)[0]
    L.set_ff1_resident(1)
    torch.cuda.synchronize()
    assert torch.equal(hmid['resident'].view(torch.int16), hmid['tiled'].view(torch.int16)), f'M = {M}: the outputs differ'
    times = {'resident': [], 'tiled': []}
    for r in range(-1, args.rounds):                       # round -1: warm-up, not kept
        for setting in (('resident', 'tiled') if r % 2 == 0 else ('tiled', 'resident')):
            t = timed(graphs[setting], args.call_replays) / args.reps
            if r >= 0:
                times[setting].append(t)
    d, v = verdict(times['resident'], times['tiled'])
    tf = 2.0 * M * 2 * ip * D / statistics.median(times['resident']) * 1e-6
    print(line(f'M = {M} resident', times['resident']) + f'   ({tf:.0f} TF)')
    print(line(f'M = {M} tiled', times['tiled']) + f'   {d:+6.2f}  {v}', flush=True)

if args.skip_step:
    sys.exit(0)

# ---------------------------------------------------------------------------------------------- 2. whole step
cv = build_models('bf16', False)[0]
videos = [synthetic_video(args.batch, 17, 256, seed=i).cuda() for i in range(3)]
L.set_ff1_resident(0)
ids0 = [cv(v, return_only_codebook_ids=True).clone() for v in videos]
torch.cuda.synchronize()
graphs = []                                                # (setting, capture index, replay of the three videos)
taken = {}
for c in range(args.captures):
    for setting, mode in (('resident', 1), ('tiled', 0)):
        L.set_ff1_resident(mode)
        reps = []
        before = L.ff1_resident_launches()
        for v, want in zip(videos, ids0):
            rp, ids = capture(lambda v=v: cv(v, return_only_codebook_ids=True))
            rp()
            torch.cuda.synchronize()
            assert torch.equal(ids, want), f'{setting}: the token ids changed'
            reps.append(rp)
        taken[setting] = L.ff1_resident_launches() - before
        cyc = itertools.cycle(reps)
        graphs.append((setting, c, lambda cyc=cyc: next(cyc)()))
L.set_ff1_resident(1)
times = {(s, c): [] for s, c, _ in graphs}
for r in range(args.rounds):
    for s, c, rp in (graphs if r % 2 == 0 else graphs[::-1]):
        times[(s, c)].append(timed(rp, args.steps))
print(f'# 2. encode step, batch {args.batch}, bf16, one hipGraph per video; us per step, {args.captures} captures per setting, '
      f'{args.rounds} interleaved rounds of {args.steps} replays; token ids identical in every graph')
print(f'# resident launches while capturing one set of three videos (warm-up included): resident {taken["resident"]}, tiled {taken["tiled"]}')
print(f'# {"setting / capture":28s} {"median":>8s} {"min":>8s} {"max":>8s}')
for s, c, _ in graphs:
    print(line(f'{s} capture {c}', times[(s, c)]))
allt = {s: [t for (s2, _), ts in times.items() if s2 == s for t in ts] for s in ('resident', 'tiled')}
d, v = verdict(allt['resident'], allt['tiled'])
print(line('resident, all captures', allt['resident']))
print(line('tiled, all captures', allt['tiled']) + f'   {d:+6.2f}  {v}', flush=True)
