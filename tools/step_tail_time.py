"""Times the tail of a training step at the real parameter shapes (BASELINE geometry, random gradients), with device events, the variants
alternating in one process:

  (a) torch.nn.utils.clip_grad_norm_ + HipAdamW.step()          -- what a user had to write before
  (b) phenaki_pytorch_amd.clip_grad_norm_ + HipAdamW.step()     -- norm pass, in-place scale, plain update
  (c) HipAdamW(max_grad_norm).step()                            -- norm pass, scaled update, .grad untouched
  (d) HipAdamW.step() alone
  (e) EMA.update() (the averaging step) against torch._foreach_lerp_ on the same tensors

for two parameter sets: MaskGit + TokenCritic, and the C-ViViT tokenizer.

    python tools/step_tail_time.py [--iters 50] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phenaki_pytorch_amd as P  # noqa: E402

CVIVIT = dict(dim=512, codebook_size=65536, image_size=256, patch_size=32, temporal_patch_size=2, spatial_depth=4, temporal_depth=4, dim_head=64, heads=8)
MASKGIT = dict(dim=512, num_tokens=65536, max_seq_len=1024, depth=6, heads=8, dim_head=64, dim_context=768)
CRITIC = dict(**MASKGIT, has_cross_attn=True)


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


def measure(name, modules, args):
    params = [p for m in modules for p in m.parameters() if p.requires_grad and p.numel()]
    numel = sum(p.numel() for p in params)
    g = torch.Generator(device='cuda').manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, device='cuda', generator=g) * 1e-2
    max_norm = 0.5
    plain = P.get_optimizer(params, lr=1e-6, wd=1e-2)
    fused = P.get_optimizer(params, lr=1e-6, wd=1e-2, max_grad_norm=max_norm)
    fused.state = plain.state                         # one set of moments: the variants stream the same bytes
    with_grad = [p for p in params]

    def a():
        torch.nn.utils.clip_grad_norm_(with_grad, max_norm)
        plain.step()

    def b():
        P.clip_grad_norm_(with_grad, max_norm)
        plain.step()

    def regrow():                                     # (a) and (b) shrink the gradients every call: put them back between rounds
        for p in params:
            p.grad.normal_(generator=g).mul_(1e-2)

    variants = dict(a_torch_clip_then_step=a, b_hip_clip_then_step=b, c_fused_clipped_step=fused.step, d_step_alone=plain.step,
                    norm_only=lambda: P._lib.grad_norm_coef([p.grad for p in params], max_norm, params[0].device),
                    hip_clip_only=lambda: P.clip_grad_norm_(with_grad, max_norm),
                    torch_clip_only=lambda: torch.nn.utils.clip_grad_norm_(with_grad, max_norm))
    times = {k: [] for k in variants}
    for k, fn in variants.items():                    # warm-up: optimizer state, workspaces, allocator
        for _ in range(3):
            fn()
    for _ in range(args.rounds):
        for k, fn in variants.items():
            regrow()
            times[k].append(timed(fn, args.iters))
    out = dict(set=name, tensors=len(params), numel=numel, iters=args.iters, rounds=args.rounds)
    for k, ts in times.items():
        out[k + '_ms'] = round(statistics.median(ts), 4)
        out[k + '_spread_ms'] = round(max(ts) - min(ts), 4)
    return out


def measure_ema(name, module, args):
    ema = P.EMA(module, update_after_step=0, update_every=1)
    ema.update(), ema.update()                         # the two copies; from here on every update averages
    pairs = [(e, x) for _, e, x in ema._pairs() if e.is_floating_point() and e.numel()]
    es, xs = [e for e, _ in pairs], [x.detach() for _, x in pairs]
    numel = sum(e.numel() for e in es)

    def foreach():
        with torch.no_grad():
            torch._foreach_lerp_(es, xs, 1e-4)

    variants = dict(e_hip_ema_update=ema.update, e_torch_foreach_lerp=foreach)
    times = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(3):
            fn()
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, args.iters))
    assert ema.next_decision() == 'lerp'
    out = dict(set=name + '_ema', tensors=len(es), numel=numel, iters=args.iters, rounds=args.rounds)
    for k, ts in times.items():
        out[k + '_ms'] = round(statistics.median(ts), 4)
        out[k + '_spread_ms'] = round(max(ts) - min(ts), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    torch.manual_seed(0)
    mg, cr = P.MaskGit(**MASKGIT).cuda(), P.TokenCritic(**CRITIC).cuda()
    print(json.dumps(measure('maskgit_critic', [mg, cr], args)), flush=True)
    del mg, cr
    torch.cuda.empty_cache()
    cv = P.CViViT(use_vgg_and_gan=False, **CVIVIT).cuda()
    print(json.dumps(measure('cvivit', [cv], args)), flush=True)
    for p in cv.parameters():
        p.grad = None
    print(json.dumps(measure_ema('cvivit', cv, args)), flush=True)


if __name__ == '__main__':
    main()
