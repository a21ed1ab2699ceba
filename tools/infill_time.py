"""Times the infilling additions on one MI355X, everything in one process, variants alternating:

  kernels   pk_topk_mask (unchanged) against pk_topk_mask_keep at B = 8, n = 576, k = 288.  A launch of ~6 us is shorter than a ctypes call, so
            each variant is captured once as a linear hipGraph of `--launches` back-to-back launches and the replays are timed between two device
            events: us per launch, device side.
              topk_mask        the plain kernel
              keep_none        known = NULL, uniform k: the same selection through the new kernel
              keep_half        the right half of every 8 x 8 token frame known (F = 288), k = 288 of its scores
              keep_step0       the same mask, scores = NULL: step 0's compaction
  loop      a B = 8 `Phenaki.infill` of the right half of a 17-frame 256 x 256 clip (tokenise, 18 steps over F = 288 free tokens per sample,
            decode, composite) against a full `Phenaki.sample` (18 steps over 576 tokens, decode), hipGraph replay, CFG 5, TokenCritic, bf16:
            ms per call, host clock around a synchronised call.

    python tools/infill_time.py [--launches 200] [--rounds 7] [--calls 3] [--no-loop]

It records; it gates nothing (the plain sampler's speed is protected by the dispatch test: the same calls)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phenaki_pytorch_amd as P  # noqa: E402
from phenaki_pytorch_amd import _lib as L  # noqa: E402

B, N, K = 8, 576, 288
CFG = dict(
    cvivit=dict(dim=512, codebook_size=65536, image_size=256, patch_size=32, temporal_patch_size=2, spatial_depth=4, temporal_depth=4, dim_head=64, heads=8),
    maskgit=dict(dim=512, num_tokens=65536, max_seq_len=1024, depth=6, heads=8, dim_head=64, dim_context=768),
    critic=dict(dim=512, num_tokens=65536, max_seq_len=1024, depth=6, heads=8, dim_head=64, dim_context=768, has_cross_attn=True),
    steps=18)


def graph_of(fn, launches):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    return g


def replay_us(g, launches, replays=20):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g.replay()
    torch.cuda.synchronize()
    start.record()
    for _ in range(replays):
        g.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / (replays * launches)


def kernels(args):
    gen = torch.Generator(device='cuda').manual_seed(0)
    scores = torch.randn((B, N), device='cuda', generator=gen)
    mask = torch.empty((B, N), device='cuda', dtype=torch.uint8)
    ids = torch.zeros((B, N), device='cuda', dtype=torch.int64)
    rows = torch.empty((B * N,), device='cuda', dtype=torch.int32)
    nxt = torch.empty((B, N), device='cuda')
    kd = torch.full((B,), K, device='cuda', dtype=torch.int32)
    off = torch.arange(B, device='cuda', dtype=torch.int32) * K
    known = torch.zeros((B, 9, 8, 8), device='cuda', dtype=torch.uint8)
    known[..., 4:] = 1
    known = known.reshape(B, N).contiguous()
    variants = dict(topk_mask=lambda: L.topk_mask(scores, B, N, K, 65536, mask, ids, rows, scores_next=nxt),
                    keep_none=lambda: L.topk_mask_keep(scores, B, N, kd, off, None, 65536, mask, ids, rows, nxt),
                    keep_half=lambda: L.topk_mask_keep(scores, B, N, kd, off, known, 65536, mask, ids, rows, nxt),
                    keep_step0=lambda: L.topk_mask_keep(None, B, N, kd, off, known, 65536, mask, ids, rows, nxt))
    graphs = {k: graph_of(fn, args.launches) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, g in graphs.items():
            times[k].append(replay_us(g, args.launches))
    out = dict(what='kernels', B=B, n=N, k=K, launches_per_graph=args.launches, rounds=args.rounds)
    for k, ts in times.items():
        out[k + '_us'] = round(statistics.median(ts), 3)
        out[k + '_spread_us'] = round(max(ts) - min(ts), 3)
    return out


def loop(args):
    torch.manual_seed(0)
    cv = P.CViViT(use_vgg_and_gan=False, **CFG['cvivit']).cuda().eval()
    mg, cr = P.MaskGit(**CFG['maskgit']).cuda().eval(), P.TokenCritic(**CFG['critic']).cuda().eval()
    ph = P.Phenaki(maskgit=mg, cvivit=cv, critic=cr, steps=CFG['steps'], text_embed_dim=768).cuda().eval()
    for m in (cv, mg, cr, ph):
        P.set_compute_dtype(m, 'bf16')
    ctx = torch.randn(B, 12, 768, device='cuda')
    ph.encode_texts = lambda texts, output_device=None: ctx[:len(texts)]
    video = torch.randn(B, 3, 17, 256, 256, device='cuda')
    edit = torch.zeros((1, 17, 256, 256), dtype=torch.bool, device='cuda')
    edit[..., 128:] = True
    texts = ['x'] * B
    ph.enable_sample_graph(True)
    variants = dict(sample=lambda: ph.sample(texts=texts, num_frames=17, cond_scale=5.),
                    infill=lambda: ph.infill(video, edit, texts=texts, cond_scale=5., composite=True))

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
    out = dict(what='loop', B=B, frames=17, steps=CFG['steps'], dtype='bf16', launch='graph', calls=args.calls, rounds=args.rounds,
               free_tokens_per_sample=dict(sample=N, infill=K))
    for k, ts in times.items():
        out[k + '_ms'] = round(statistics.median(ts), 3)
        out[k + '_spread_ms'] = round(max(ts) - min(ts), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--no-loop', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('infill_time: needs an MI355X (no CPU timing)')
    print(json.dumps(kernels(args)), flush=True)
    if not args.no_loop:
        with torch.no_grad():
            print(json.dumps(loop(args)), flush=True)


if __name__ == '__main__':
    main()
