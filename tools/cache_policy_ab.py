"""Per-site A/B of the cache policies (pk_set_cache_policy) on the headline leg, in one process:

    python tools/cache_policy_ab.py [--rounds 7] [--steps 60] [--masks 0x..,0x..] > cache_policy_sites.txt

The C-ViViT encode at batch 8, bf16, exactly as bench.py runs it (CViViT.forward(video, return_only_codebook_ids=True), three rotating
videos, one hipGraph per video).  A captured graph keeps the policy it was captured with, so every mask gets its own three graphs; the
masks are then timed in interleaved rounds (round r: every mask once, `steps` replays between two events) and the median / min / max of
the rounds is printed per mask, next to the plain mask's.  Default masks: plain, then every store site alone at write-through and at
non-temporal, every load site alone at non-temporal.  The token ids of every mask are compared with the plain ones (must be identical)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_models, capture, synthetic_video  # noqa: E402
from phenaki_pytorch_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--steps', type=int, default=60)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--masks', default='', help='comma-separated masks to time next to 0 instead of the per-site list')
args = ap.parse_args()
torch.set_grad_enabled(False)

cv = build_models('bf16', False)[0]
videos = [synthetic_video(args.batch, 17, 256, seed=i).cuda() for i in range(3)]
L.set_cache_policy(0)
ids0 = [cv(v, return_only_codebook_ids=True).clone() for v in videos]
torch.cuda.synchronize()

if args.masks:
    configs = [('plain', 0)] + [(m, int(m, 0)) for m in args.masks.split(',')]
else:
    configs = [('plain', 0)]
    for s in L.CP_STORE_SITES:
        configs += [(f'{s}=wt', L.cache_policy_mask(**{s: L.CP_WT})), (f'{s}=nt', L.cache_policy_mask(**{s: L.CP_NT}))]
    configs += [(f'{s}=nt', L.cache_policy_mask(**{s: L.CP_NT})) for s in L.CP_LOAD_SITES]

graphs = {}
for name, mask in configs:
    L.set_cache_policy(mask)
    assert L.get_cache_policy() == mask
    reps = []
    for v, want in zip(videos, ids0):
        rp, out = capture(lambda v=v: cv(v, return_only_codebook_ids=True))
        rp()
        torch.cuda.synchronize()
        assert torch.equal(out, want), f'{name}: the token ids changed'
        reps.append(rp)
    graphs[name] = reps
L.set_cache_policy(0)


def timed(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(6):
        reps[i % 3]()
    e0.record()
    for i in range(args.steps):
        reps[i % 3]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps          # us per step


times = {name: [] for name, _ in configs}
for r in range(args.rounds):
    order = configs if r % 2 == 0 else configs[::-1]
    for name, _ in order:
        times[name].append(timed(graphs[name]))

print(f'# encode step, batch {args.batch}, bf16, one hipGraph per video; us per step, {args.rounds} interleaved rounds of {args.steps} replays')
print(f'# {"site=policy":22s} {"mask":>8s} {"median":>8s} {"min":>8s} {"max":>8s} {"vs plain":>9s}  verdict (wins only beyond the larger min-max spread)')
p = times['plain']
pm, pspread = statistics.median(p), max(p) - min(p)
for name, mask in configs:
    t = times[name]
    med, spread = statistics.median(t), max(t) - min(t)
    d = med - pm
    verdict = '' if name == 'plain' else ('WINS' if -d > max(spread, pspread) else ('loses' if d > max(spread, pspread) else 'within noise'))
    print(f'  {name:22s} {mask:#8x} {med:8.2f} {min(t):8.2f} {max(t):8.2f} {d:+9.2f}  {verdict}', flush=True)
