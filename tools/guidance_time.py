"""Times the guided-sampling additions on one MI355X, everything in one process, variants alternating, and writes profiles/guidance_time.txt:

  kernels   pk_cfg_mix (unchanged) against pk_guidance_mix with P = 1, 2, 3 conditional branches and a base, at B = 8, n = 576, D = 512, bf16
            output, every row.  A launch of a few us is shorter than a ctypes call, so each variant is captured once as a linear hipGraph of
            `--launches` back-to-back launches and the replays are timed between two device events: us per launch, device side.
  loop      a B = 8, 17-frame `Phenaki.sample` (18 steps, TokenCritic, bf16, hipGraph replay): the scalar path (cond_scale=5.) against the table
            path with P = 1 (cond_scale=[5.] * 8: the same work), and the table path with J = 3 (a negative prompt and a blend of two) and
            J = 4 (a blend of three and a negative prompt) branches: ms per call, host clock around a synchronised call.
            The P = 1 table path is judged against the scalar path's own run-to-run spread (max - min over the rounds of this run); J = 3 and
            J = 4 do proportionally more trunk work and are recorded, not judged.

    python tools/guidance_time.py [--launches 200] [--rounds 7] [--calls 2] [--no-loop] [--out profiles/guidance_time.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import phenaki_pytorch_amd as P  # noqa: E402
from phenaki_pytorch_amd import _lib as L  # noqa: E402
from tools.infill_time import CFG, graph_of, replay_us  # noqa: E402

B, N, D = 8, 576, 512


def kernels(args):
    gen = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn((4 * B * N, D), device='cuda', generator=gen)
    out = torch.empty((B * N, D), device='cuda', dtype=torch.bfloat16)
    coef = {p: torch.cat((torch.full((p * B,), 1. / p), torch.full((B,), 5.))).cuda() for p in (1, 2, 3)}
    variants = dict(cfg_mix=lambda: L.cfg_mix(x, B, N, 0, None, B * N, 5., True, out, D))
    for p in (1, 2, 3):
        variants[f'guidance_mix_P{p}'] = lambda p=p: L.guidance_mix(x, B, N, 0, None, B * N, coef[p], p, True, out, D)
    graphs = {k: graph_of(fn, args.launches) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, g in graphs.items():
            times[k].append(replay_us(g, args.launches))
    res = dict(what='kernels', B=B, n=N, D=D, out='bf16', launches_per_graph=args.launches, rounds=args.rounds)
    for k, ts in times.items():
        res[k + '_us'] = round(statistics.median(ts), 3)
        res[k + '_spread_us'] = round(max(ts) - min(ts), 3)
    for p in (1, 2, 3):                                  # f32 bytes read per branch + bf16 bytes written, over the median time
        res[f'guidance_mix_P{p}_GBps'] = round(B * N * D * (4 * (p + 1) + 2) / (res[f'guidance_mix_P{p}_us'] * 1e3), 1)
    return res


def loop(args):
    torch.manual_seed(0)
    cv = P.CViViT(use_vgg_and_gan=False, **CFG['cvivit']).cuda().eval()
    mg, cr = P.MaskGit(**CFG['maskgit']).cuda().eval(), P.TokenCritic(**CFG['critic']).cuda().eval()
    ph = P.Phenaki(maskgit=mg, cvivit=cv, critic=cr, steps=CFG['steps'], text_embed_dim=768).cuda().eval()
    for m in (cv, mg, cr, ph):
        P.set_compute_dtype(m, 'bf16')
    ctx = {k: torch.randn(1, 12, 768, device='cuda') for k in ('x', 'y', 'z', 'neg')}
    ph.encode_texts = lambda texts, output_device=None: torch.cat([ctx[t] for t in texts], dim=0)
    texts = ['x'] * B
    ph.enable_sample_graph(True)
    kw = dict(texts=texts, num_frames=17)
    variants = dict(scalar=lambda: ph.sample(cond_scale=5., **kw),
                    table_P1=lambda: ph.sample(cond_scale=[5.] * B, **kw),
                    table_J3=lambda: ph.sample(cond_scale=[5.] * B, blend=[('y', 0.3)], negative_texts='neg', **kw),
                    table_J4=lambda: ph.sample(cond_scale=[5.] * B, blend=[('y', 0.3), ('z', 0.2)], negative_texts='neg', **kw))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls
    for fn in variants.values():                     # eager pass + capture, then a pure replay
        fn()
        fn()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    ph.enable_sample_graph(False)
    res = dict(what='loop', B=B, frames=17, steps=CFG['steps'], dtype='bf16', launch='graph', calls=args.calls, rounds=args.rounds)
    for k, ts in times.items():
        res[k + '_ms'] = round(statistics.median(ts), 3)
        res[k + '_spread_ms'] = round(max(ts) - min(ts), 3)
        res[k + '_rounds_ms'] = [round(t, 3) for t in ts]
    return res


def verdict(res):
    diff, spread = res['table_P1_ms'] - res['scalar_ms'], res['scalar_spread_ms']
    line = (f"table path P = 1 against the scalar path: {res['table_P1_ms']:.3f} ms vs {res['scalar_ms']:.3f} ms per call (medians of {res['rounds']} rounds), "
            f"difference {diff:+.3f} ms; the scalar path's own run-to-run spread in this run is {spread:.3f} ms: ")
    return line + ('SLOWER by more than that spread' if diff > spread else 'within that spread (or faster)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=2)
    ap.add_argument('--no-loop', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'guidance_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('guidance_time: needs an MI355X (no CPU timing)')
    lines = ['# tools/guidance_time.py on ' + torch.cuda.get_device_name(0) + ': one process, variants alternating; *_us device events around graph replays,',
             '# *_ms host clock around synchronised calls; spread = max - min over the rounds']
    lines.append(json.dumps(kernels(args)))
    if not args.no_loop:
        with torch.no_grad():
            res = loop(args)
        lines += [json.dumps(res), verdict(res),
                  f"recorded, not judged: J = 3 {res['table_J3_ms']:.3f} ms, J = 4 {res['table_J4_ms']:.3f} ms per call (3 / 2 and 4 / 2 of the trunk work of J = 2)"]
    text = '\n'.join(lines) + '\n'
    print(text, end='', flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
