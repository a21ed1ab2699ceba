"""A/B of the compile-time GEMM epilogue forms (pk_set_gemm_hot_forms) against the generic epilogue of the same build, in one process:

    python tools/gemm_hot_forms_ab.py [--rounds 7] [--steps 60] [--reps 20] [--call-replays 500] [--captures 3] > gemm_hot_forms_ab.txt

1. per call: the three layer calls of a bf16 transformer block at M = 4608 rows (batch-8 encode), with the operands attention.py gives
   them (to_out: f32 residual, f32 C, bf16 C2, row statistics; FF1: LayerNorm fold from those statistics, GEGLU, bf16 C; FF2: f32 residual,
   f32 C, with / without the bf16 C2).  Every setting is one hipGraph of `reps` launches; the settings are timed in interleaved rounds of `call-replays`
   replays (a tenth of a second and more per figure), after one round that is thrown away (clocks, code objects).
2. whole step: the C-ViViT encode exactly as bench.py runs it (three rotating videos, one hipGraph per video).  A captured graph keeps
   the form it was captured with; every setting is captured `captures` times (fresh buffers: the spread between captures of one setting
   is buffer placement), all graphs are timed in interleaved rounds of `steps` replays.
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
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--steps', type=int, default=60)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--captures', type=int, default=3)
ap.add_argument('--call-replays', type=int, default=500, help='replays of the per-call graph in one timed round')
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--rows', type=int, default=4608)
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
M, D, dt = args.rows, 512, L.BF16
dev = torch.device('cuda')
attn, ff = A.Attention(D, heads=8).to(dev), A.FeedForward(D).to(dev)
gen = torch.Generator().manual_seed(0)
x = torch.randn(M, D, generator=gen).to(dev)
o = torch.randn(M, D, generator=gen).to(dev).to(torch.bfloat16)
out, out_t, stats = attn._finish(o, x, dt, 'stats')
w1g, s1, t1, _ = ff._packed_folded(dt)
w1p, w2p, ip = ff._packed(dt)
hmid = torch.empty((M, ip), device=dev, dtype=torch.bfloat16)
L.gemm(dt, out_t, w1g, M, 2 * ip, D, C=hmid, act=L.ACT_GEGLU, ln=(s1, t1, ff[0].eps), ln_stats=stats)
wo = A.linear_weight(attn.to_out, dt)
c_f32, c_bf, st2 = torch.empty_like(x), torch.empty_like(out_t), torch.empty_like(stats)
calls = [
    ('to_out (OUT)', L.EPI_OUT, lambda: L.gemm(dt, o, wo, M, D, D, C=c_f32, res=x, C2=c_bf, stats_out=st2)),
    ('FF1', L.EPI_FF1, lambda: L.gemm(dt, out_t, w1g, M, 2 * ip, D, C=hmid, act=L.ACT_GEGLU, ln=(s1, t1, ff[0].eps), ln_stats=stats)),
    ('FF2 with C2 (FF2A)', L.EPI_FF2A, lambda: L.gemm(dt, hmid, w2p, M, D, ip, C=c_f32, res=out, C2=c_bf)),
    ('FF2 without C2 (FF2B)', L.EPI_FF2B, lambda: L.gemm(dt, hmid, w2p, M, D, ip, C=c_f32, res=out)),
]
print(f'# 1. per call, M = {M}, bf16; us per launch, one hipGraph of {args.reps} launches per setting, {args.rounds} interleaved rounds of {args.call_replays} replays')
print(f'# {"call / setting":28s} {"median":>8s} {"min":>8s} {"max":>8s}   hot - generic, verdict')
for name, form, fn in calls:
    graphs = {}
    for setting, on in (('hot', 1), ('generic', 0)):
        L.set_gemm_hot_forms(on)

        def many(fn=fn):
            for _ in range(args.reps):
                fn()
        graphs[setting] = capture(many)[0]
    L.set_gemm_hot_forms(1)
    times = {'hot': [], 'generic': []}
    for r in range(-1, args.rounds):                       # round -1: warm-up, not kept
        for setting in (('hot', 'generic') if r % 2 == 0 else ('generic', 'hot')):
            t = timed(graphs[setting], args.call_replays) / args.reps
            if r >= 0:
                times[setting].append(t)
    d, v = verdict(times['hot'], times['generic'])
    print(line(name + ' hot', times['hot']))
    print(line(name + ' generic', times['generic']) + f'   {d:+6.2f}  {v}', flush=True)

if args.skip_step:
    sys.exit(0)

# ---------------------------------------------------------------------------------------------- 2. whole step
cv = build_models('bf16', False)[0]
videos = [synthetic_video(args.batch, 17, 256, seed=i).cuda() for i in range(3)]
L.set_gemm_hot_forms(0)
ids0 = [cv(v, return_only_codebook_ids=True).clone() for v in videos]
torch.cuda.synchronize()
graphs = []                                                # (setting, capture index, replay of the three videos)
for c in range(args.captures):
    for setting, on in (('hot', 1), ('generic', 0)):
        L.set_gemm_hot_forms(on)
        reps = []
        for v, want in zip(videos, ids0):
            rp, ids = capture(lambda v=v: cv(v, return_only_codebook_ids=True))
            rp()
            torch.cuda.synchronize()
            assert torch.equal(ids, want), f'{setting}: the token ids changed'
            reps.append(rp)
        cyc = itertools.cycle(reps)
        graphs.append((setting, c, lambda cyc=cyc: next(cyc)()))
L.set_gemm_hot_forms(1)
times = {(s, c): [] for s, c, _ in graphs}
for r in range(args.rounds):
    for s, c, rp in (graphs if r % 2 == 0 else graphs[::-1]):
        times[(s, c)].append(timed(rp, args.steps))
print(f'# 2. encode step, batch {args.batch}, bf16, one hipGraph per video; us per step, {args.captures} captures per setting, '
      f'{args.rounds} interleaved rounds of {args.steps} replays; token ids identical in every graph')
print(f'# {"setting / capture":28s} {"median":>8s} {"min":>8s} {"max":>8s}')
for s, c, _ in graphs:
    print(line(f'{s} capture {c}', times[(s, c)]))
allt = {s: [t for (s2, _), ts in times.items() if s2 == s for t in ts] for s in ('hot', 'generic')}
d, v = verdict(allt['hot'], allt['generic'])
print(line('hot, all captures', allt['hot']))
print(line('generic, all captures', allt['generic']) + f'   {d:+6.2f}  {v}', flush=True)
