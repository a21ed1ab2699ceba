"""bench.py -- the BASELINE.json metric on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A "step" is one pass of the hot path over one batch of synthetic input: BASELINE.json configs[1], the C-ViViT tokenizer
(dim 512, patch 32, temporal patch 2, depth 4+4, LFQ 65 536) encoding a (8, 3, 17, 256, 256) f32 video that is already
resident in HBM into (8, 9, 8, 8) int64 token ids, bf16 MFMA operands / f32 accumulation.  With N > 1 every rank encodes
its own 8 videos (batch sharding, weak scaling, no collective on the data path).  After W warm-up steps, exactly K steps are
timed as one region bracketed by barrier + synchronize (max over ranks); ms_per_step is that region over K.  The steps rotate
through `--rotate` distinct input batches (3 x 107 MB > the 256 MB Infinity Cache) so the video really comes from HBM.
`--dump-outputs DIR` writes the token ids of the last timed step to DIR/ids.npy (float64; seeded inputs and weights, so two
builds can be compared output for output).

A plain run does only the headline and prints its JSON line.  With `--full` the same JSON line also carries
  roofline     : the encode leg's dominant kernel -- algorithmic flops per launch over its live HIP-event duration, plus the
                 fabric traffic per launch from the committed rocprofv3 PMC passes (profiles/pmc_traffic_rNN.json);
  kernels      : every kernel of the encode / decode / sampling legs against ITS roofline (HBM GB/s for the patch / VQ /
                 norm / PEG kernels, MFMA TFLOP/s for the GEMM / attention / vocab-head kernels), from in-run HIP events;
  decode       : C-ViViT decode ids -> pixels, frames/s;
  sample       : MaskGIT sampled tokens/s of an 18-step Phenaki.sample (configs[2]; with N > 1 through sample_sharded,
                 i.e. WITH the one RCCL all-gather of the decoded videos inside the timed region), eager and hipGraph;
  sample_cfg3  : the same at configs[3]'s per-GPU batch (32 videos over 8 GPUs = 4 per GPU);
  make_video   : configs[4], 3 scenes (17, 14, 14 frames, prime K = 5), one video per GPU, tokens/s and wall-clock;
  parity_mode  : the split-bf16 ("bf16x3") mode -- held by the tests to bit-exact ids / 1e-3 against the reference, like exact f32 --
                 timed on the same legs; parity_mode_f32: the exact-f32 mode beside it;
  encode_b32 / sample_b32 : the same legs with 32 videos per GPU (what the kernels reach when the GPU is full);
  train_step / cvivit_train_step : one full training step (forward + backward + AdamW) of Phenaki.forward on token ids, and of the tokenizer on
                 its reconstruction loss;
  cpu_baseline : the CPU oracle (a port of the reference algorithm, oracle/phenaki_oracle.py) on a bounded sample of
                 the same workload on this box's host cores.
--no-sample / --no-cpu / --no-parity-mode / --no-kernels / --encode-only / --legs / --groups select among these and only act with --full.
"""
import argparse
import json
import os
import statistics
import sys
import time

# kernel arguments in device memory: the ROCm 7.2 default on this GPU, pinned here because the sampling loop is ~3 000 short
# launches per call (measured: 65.6 ms with it, 70.6 ms with HIP_FORCE_DEV_KERNARG=0); must be set before HIP initialises
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0        # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3          # f32-input MFMA = the f32 vector rate
PEAK_HBM_GBS = 8000.0            # HBM3E spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dump-outputs', metavar='DIR', help='write the token ids of the last timed step to DIR/ids.npy (float64)')
    ap.add_argument('--full', action='store_true', help='also run the legs, per-kernel rooflines, parity modes and CPU baseline')
    ap.add_argument('--groups', type=int, default=25, help='--full: timed regions of the decode / encode_b32 / parity-mode legs (median reported)')
    ap.add_argument('--rotate', type=int, default=3, help='distinct input batches the steps rotate through')
    ap.add_argument('--batch', type=int, default=8, help='videos per GPU (configs[1]: 8)')
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32', 'bf16x3'])
    ap.add_argument('--no-graph', action='store_true', help='launch eagerly instead of replaying captured hipGraphs')
    ap.add_argument('--no-sample', action='store_true', help='skip the MaskGIT sampling / make_video / objective legs')
    ap.add_argument('--no-cpu', action='store_true', help='skip the CPU baseline leg')
    ap.add_argument('--no-parity-mode', action='store_true', help='skip the exact-f32 timing')
    ap.add_argument('--no-kernels', action='store_true', help='skip the per-kernel roofline table')
    ap.add_argument('--encode-only', action='store_true', help='--full: only the headline leg and its kernel table (profiling runs)')
    ap.add_argument('--legs', default='decode,encode_b32,sample,sample_cfg3,sample_b32,make_video,scaling_projection,objective,train_step,cvivit_train_step,cvivit_gan_step',
                    help='comma list of the legs reported beside the headline encode leg')
    ap.add_argument('--sample-batch', type=int, default=8)
    ap.add_argument('--cpu-seconds', type=float, default=12.0)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be at least 1 and --warmup at least 0')
    return args


def _free_port():
    import socket
    sk = socket.socket()
    sk.bind(('127.0.0.1', 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def spawn_ranks_if_needed(args):
    """`python bench.py --gpus N` (N > 1, no launcher): start the N ranks ourselves -- one process per GPU under
    torch.distributed.run, RCCL over xGMI -- as a child process whose exit status this one returns, so the single JSON line still comes from
    rank 0 on stdout.  (A child, not exec: device_count() may already have opened the HIP runtime in this process.)
    Under a launcher (WORLD_SIZE set) this is a no-op.  Fewer than N visible devices is an error, never a silent 1-rank run."""
    if args.gpus <= 1 or 'WORLD_SIZE' in os.environ:
        return
    one_device = bool(os.environ.get('PK_BENCH_ONE_DEVICE'))
    ndev = torch.cuda.device_count()
    if ndev < args.gpus and not one_device:
        raise SystemExit(f'bench.py --gpus {args.gpus}: only {ndev} HIP device(s) visible (PK_BENCH_ONE_DEVICE=1 dry-runs the '
                         'multi-rank path on one device over gloo)')
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    sys.stderr.flush()
    import subprocess
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def init_dist(n):
    rank = int(os.environ.get('RANK', 0))
    local = int(os.environ.get('LOCAL_RANK', 0))
    ws = int(os.environ.get('WORLD_SIZE', 1))
    one_device = bool(os.environ.get('PK_BENCH_ONE_DEVICE'))   # dry run of the N > 1 code path on a 1-GPU box: every rank on cuda:0,
    if one_device:                                              # gloo instead of RCCL (which refuses two ranks on one device)
        local = 0
    if ws > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        torch.cuda.set_device(local)
        if one_device:
            dist.init_process_group('gloo', rank=rank, world_size=ws)
        else:
            dist.init_process_group('nccl', rank=rank, world_size=ws, device_id=torch.device('cuda', local))
    else:
        torch.cuda.set_device(0)
    if ws != n:
        raise SystemExit(f'bench.py --gpus {n} but {ws} rank(s) are running (WORLD_SIZE={os.environ.get("WORLD_SIZE")}): refusing to report a '
                         f'{ws}-rank number as an {n}-GPU one')
    return rank, local, ws


def barrier_sync(ws):
    if ws > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()


def max_over_ranks(x, ws):
    if ws == 1:
        return x
    import torch.distributed as dist
    t = torch.tensor([x], device='cuda', dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def timed_groups(fn, steps, groups, ws):
    """`groups` timed regions of exactly `steps` calls of fn(i), each bracketed by barrier + synchronize, max over ranks per
    region; returns the list of region times (s)."""
    out, i = [], 0
    for _ in range(groups):
        barrier_sync(ws)
        t0 = time.perf_counter()
        for _ in range(steps):
            fn(i)
            i += 1
        barrier_sync(ws)
        out.append(max_over_ranks(time.perf_counter() - t0, ws))
    return out


# BASELINE.json configs[1..2]: C-ViViT dim 512 / codebook 65 536 / 256x256 / patch 32 / temporal patch 2 / depth 4+4;
# MaskGit and TokenCritic dim 512 / depth 6 / 8 heads / T5-base context (768); 18 sampling steps
BASELINE_CFG = dict(
    cvivit=dict(dim=512, codebook_size=65536, image_size=256, patch_size=32, temporal_patch_size=2,
                spatial_depth=4, temporal_depth=4, dim_head=64, heads=8),
    maskgit=dict(dim=512, num_tokens=65536, max_seq_len=1024, depth=6, heads=8, dim_head=64, dim_context=768),
    critic=dict(dim=512, num_tokens=65536, max_seq_len=1024, depth=6, heads=8, dim_head=64, dim_context=768,
                has_cross_attn=True),
    steps=18,
)


def build_models(dtype, with_sampler):
    """random-init weights of the BASELINE architecture (the modules' own default initialisers under a fixed seed; no
    checkpoints offline).  The GPU legs of this file use the product package only -- nothing under oracle/ or tests/."""
    import phenaki_pytorch_amd as P
    torch.manual_seed(0)
    cv = P.CViViT(use_vgg_and_gan=False, **BASELINE_CFG['cvivit'])
    mg = P.MaskGit(**BASELINE_CFG['maskgit']) if with_sampler else None
    cr = P.TokenCritic(**BASELINE_CFG['critic']) if with_sampler else None
    cv = cv.cuda().eval()
    ph = None
    if with_sampler:
        mg, cr = mg.cuda().eval(), cr.cuda().eval()
        ph = P.Phenaki(maskgit=mg, cvivit=cv, critic=cr, steps=BASELINE_CFG['steps'],
                       text_embed_dim=BASELINE_CFG['maskgit']['dim_context']).cuda().eval()
    for m in (cv, mg, cr, ph):
        if m is not None:
            P.set_compute_dtype(m, dtype)
    return cv, mg, cr, ph


def synthetic_video(batch, frames, size, seed):
    g = torch.Generator(device='cpu')
    g.manual_seed(1000 + seed)
    return torch.randn(batch, 3, frames, size, size, generator=g)


def synthetic_context(batch, length, dim, seed):
    """stands in for the cached T5 encoder output (no all-zero rows: every context token is real)"""
    g = torch.Generator(device='cpu')
    g.manual_seed(2000 + seed)
    return torch.randn(batch, length, dim, generator=g)


def capture(fn):
    """fn() captured as one hipGraph (after a side-stream warm-up); returns (replay, outputs)"""
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        out = fn()
    return graph.replay, out


# ------------------------------------------------------------------------------------------ per-kernel rooflines

# template order: T, TM, TN, WM, WN, STAGES, ROWB, PW (the names rocprofv3 prints)
# rocprofv3 kernel names: gemm_dma_kernel<T, TM, TN, WM, WN, STAGES, ROWB, PW, LNF> (LNF 0 plain, 1 / 2 LayerNorm fold with in-loop / handed-over statistics)
VARIANT_KERNEL = {1: 'gemm_kernel<T,TA,2,2>', 2: 'gemm_kernel<T,TA,4,4>', 3: 'gemm_dma_kernel<T,2,2,2,2,4,128,0,0>',
                  8: 'gemm_dma_kernel<T,2,2,2,2,2,128,0,0>', 9: 'gemm_dma_kernel<T,4,4,2,2,2,128,0,0>',
                  24: 'gemm_dma_kernel<T,4,2,2,4,2,128,0,0>', 27: 'gemm_dma_kernel<T,4,2,2,2,2,128,0,0>',
                  33: 'gemm_dma_kernel<T,2,2,2,2,3,128,2,0>', 50: 'gemm_p8_kernel<T,0,4,0>'}


def _esz(t):
    return 0 if t is None else t.element_size()


class KernelProfiler:
    """live HIP-event timing of every libphenaki_hip launch of one (untimed, eager) pass, on the stream the kernels run on:
    each launch of the pass is recorded with its live operands, then re-issued REPS times back to back (as one captured
    hipGraph) between two HIP events (an event pair around ONE ~10 us kernel mostly measures the events).  Every launch carries its algorithmic work:
    flops for the MFMA kernels, bytes for the HBM-bound ones (DESIGN.md section 4 lists the per-unit figures)."""
    REPS = 10

    def __init__(self, leg, mode='bf16'):
        # mode: the compute dtype of the models under the profiler ('bf16' | 'fp32' | 'bf16x3'; True / False = legacy f32 flag)
        mode = {True: 'fp32', False: 'bf16'}.get(mode, mode)
        self.leg, self.mode, self.f32 = leg, mode, mode == 'fp32'
        self.calls = []

    # (label, bound, work) of one wrapper call; work = flops ('mfma') or bytes ('hbm')
    def _model(self, name, a, kw):
        lib = self._lib
        if name == 'gemm':
            dtype, A, W, M, N, K = a[:6]
            a_is_f32 = 1 if A.dtype == torch.float32 else 0
            rows = A.shape[0] if kw.get('a_rows') is not None else M
            v = kw.get('variant') or lib.load().pk_gemm_auto_variant(dtype, a_is_f32, M, N, K, kw.get('lda') or A.stride(-2), W.stride(0), rows)
            t = {lib.BF16: 'pk::bf16', lib.BF16X3: 'pk::bf16x3'}.get(dtype, 'float')
            label = VARIANT_KERNEL.get(v, f'gemm variant{v}').replace('TA', 'float' if a_is_f32 else t).replace('T', t)
            if kw.get('ln'):                                  # LayerNorm-folded instantiation: 64x64 or 128x128 by the same size rule
                big = VARIANT_KERNEL[9] if dtype == self._lib.BF16X3 else VARIANT_KERNEL[24]        # (split-bf16 folds on its 4-wave 128 x 128 tile, gemm.hip)
                label = (big if v in (24, 2, 9) else VARIANT_KERNEL[8]).replace('T', t)[:-2] + ('2>' if kw.get('ln_stats') is not None else '1>')
            return label, 'mfma', 2.0 * M * N * K
        if name == 'qkv_project':
            xq, xkv, wq, wkv, S, nseq, h, K = a[:8]
            return f'qkv_project_kernel[n={nseq}]', 'mfma', 2.0 * S * nseq * K * 64 * h * (3 if xkv is not None else 1)
        if name == 'qkv_attn':
            xq, xkv, wq, wkv, S, n, h, K = a[:8]
            return f'qkv_attn_kernel[n={n}]', 'mfma', 2.0 * S * n * K * 192 * h + 4.0 * S * h * n * n * 64
        if name == 'q_attn_cached':
            xq, wq, S, n, h, K = a[:6]
            n_kv, nnull = a[11], a[12]
            return f'q_attn_cached_kernel[nk={n_kv + nnull}]', 'mfma', 2.0 * S * n * K * 64 * h + 4.0 * S * h * n * (n_kv + nnull) * 64
        if name == 'attn_fwd':
            dtype, Qp, Kp, Vt, O, S, h, nq, n_kv, nnull = a[:10]
            return f'attn_fwd[nq={nq},nk={n_kv + nnull}]', 'mfma', 4.0 * S * h * nq * (n_kv + nnull) * 64
        if name == 'attn_small':
            S, h, n = a[6:9]
            return f'attn_small_kernel[n={n}]', 'valu', 4.0 * S * h * n * n * 64
        if name == 'vocab_sample':
            dtype, A, W, bias, M, V, D = a[:7]
            return 'vocab_sample_kernel', 'mfma', 2.0 * M * V * D
        if name == 'layernorm':
            x, gamma, beta, M, D = a[:5]
            b = 4 * M * D + sum(_esz(kw.get(k)) * M * D for k in ('out', 'out2', 'raw'))
            return f'ln_rows_kernel[D={D}]', 'hbm', b
        if name == 'layernorm_lfq':
            M, D = a[6], a[7]
            return 'ln_lfq_kernel', 'hbm', 4 * M * D + 8 * M
        if name == 'patchify_ln':
            video, f0, nt, pt, ph, pw, weight, bias, out = a[:9]
            B, C, F, H, W = video.shape
            rows, P = B * nt * (H // ph) * (W // pw), C * pt * ph * pw
            return f'patchify_ln_kernel[P={P}]', 'hbm', rows * P * (4 + _esz(out))
        if name == 'patch_embed':
            video, ph, pw, N, groups = a[:5]
            B, C, F, H, W = video.shape
            fl = sum(2.0 * (B * nt * (H // ph) * (W // pw)) * N * (C * pt * ph * pw) for (_, _, _, _, f0, nt, pt) in groups)
            return 'patch_embed_kernel', 'mfma', fl
        if name == 'patch_embed_splitk':
            # the patch embedding is HBM-bound on paper (13.37 MB of f32 video per 17-frame clip, read once); algorithmic bytes =
            # the video frames the groups cover + the token rows the finish writes (f32 + bf16), per launch pair -- reported on the HBM axis
            video, ph, pw, N, groups = a[:5]
            B, C, F, H, W = video.shape
            by = sum(4.0 * B * C * nt * pt * H * W for (_, _, _, f0, nt, pt) in groups)
            return 'patch_embed_wide_kernel', 'hbm', by
        if name == 'patch_embed_finish':
            part = a[0]
            ns, rows, N = part.shape
            outs = sum(_esz(kw.get(k)) for k in ('out2', 'out'))
            return 'patch_embed_finish_kernel', 'hbm', rows * N * (4.0 * ns + outs)
        if name == 'patch_embed_finish_groups':          # (round 5: both frame groups' finish in one launch)
            outs = sum(_esz(kw.get(k)) for k in ('out2', 'out'))
            return 'patch_embed_finish_pair_kernel', 'hbm', sum(g[0].shape[1] * g[0].shape[2] * (4.0 * g[0].shape[0] + outs) for g in a[0])
        if name == 'gemm_splitk':
            dtype, A, W, M, N, K = a[:6]
            t = {lib.BF16: 'pk::bf16', lib.BF16X3: 'pk::bf16x3'}.get(dtype, 'float')
            return f'gemm_dma_splitk_kernel<{t}>', 'mfma', 2.0 * M * N * K
        if name == 'sum_batch':
            src, S, out, E = a[:4]
            return 'sum_batch_kernel', 'hbm', 4.0 * E * (S + 1)
        if name == 'unpatchify':
            pix, video, f0, nt, pt, ph, pw = a[:7]
            B, C, F, H, W = video.shape
            return 'unpatchify_kernel', 'hbm', 8 * B * nt * pt * C * H * W
        if name == 'peg':
            B, T, H, W, D = a[4:9]
            return 'peg_row_kernel', 'hbm', 8 * B * T * H * W * D
        if name == 'lfq_encode':
            M, D = a[5], a[6]
            return 'lfq_encode_kernel', 'hbm', 4 * M * D + 8 * M
        if name == 'lfq_decode':
            M, D = a[4], a[5]
            return 'lfq_decode_kernel', 'hbm', 4 * M * D + 8 * M
        if name == 'embed':
            ids, tok, pos, out, S, n, D = a[:7]
            npr = kw['ids_prime'].shape[-1] if kw.get('ids_prime') is not None else 0
            return 'embed_kernel', 'hbm', 8 * S * (n + npr) * D
        if name == 'cfg_mix':
            x, nb, n_tot, n_prime, rows, nrows, scale, has_null, out, D = a[:10]
            return 'cfg_mix_kernel', 'hbm', nrows * D * (4 * (2 if has_null else 1) + _esz(out))
        if name == 'critic_head':
            x, w, b, D, nb, n_tot, n_prime, has_null = a[:8]
            return 'critic_head_kernel', 'hbm', 4 * nb * (n_tot - n_prime) * D * (2 if has_null else 1)
        if name == 'attn_prep':
            dtype, q, kv = a[:3]
            return 'attn_prep kernels', 'hbm', q.numel() * 4 + (kv.numel() * 4 if kv is not None else 0)
        if name in ('vocab_reduce', 'topk_mask', 'l2norm_rows', 'cpb_input', 'vocab_ce', 'sqdiff_sum'):
            return f'{name} kernel', 'latency', 0
        return None

    def __enter__(self):
        from phenaki_pytorch_amd import _lib
        self._lib = _lib
        self._orig = {}
        prof = self
        names = ['gemm', 'patch_embed', 'patch_embed_splitk', 'patch_embed_finish', 'patch_embed_finish_groups', 'gemm_splitk', 'sum_batch', 'qkv_project', 'qkv_attn', 'q_attn_cached', 'attn_fwd', 'attn_small', 'vocab_sample', 'layernorm', 'layernorm_lfq', 'patchify_ln',
                 'unpatchify', 'peg', 'lfq_encode', 'lfq_decode', 'embed', 'cfg_mix', 'critic_head', 'attn_prep', 'vocab_reduce',
                 'topk_mask', 'l2norm_rows']

        def wrap(name, fn):
            def inner(*a, **kw):
                prof.calls.append((name, fn, a, kw))
                return fn(*a, **kw)
            return inner
        for n in names:
            self._orig[n] = getattr(_lib, n)
            setattr(_lib, n, wrap(n, self._orig[n]))
        return self

    def __exit__(self, *exc):
        for n, fn in self._orig.items():
            setattr(self._lib, n, fn)
        torch.cuda.synchronize()

    def table(self):
        by = {}
        for name, fn, a, kw in self.calls:
            m = self._model(name, a, kw)
            if m is None:
                continue
            label, bound, work = m
            # the REPS re-issues are captured into ONE hipGraph and the replay is timed: issued from Python, launches shorter
            # than the ~8 us ctypes call would measure the host, not the kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn(*a, **kw)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(self.REPS):
                    fn(*a, **kw)
            graph.replay()
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            d = by.setdefault((label, bound), [0, 0.0, 0.0])
            d[0] += 1
            d[1] += work
            d[2] += e0.elapsed_time(e1) * 1e-3 / self.REPS
            del graph
        self.calls = []
        rows = []
        for (label, bound), (launches, work, secs) in by.items():
            r = dict(kernel=label, leg=self.leg, launches=launches, avg_us=secs / launches * 1e6, us_total=secs * 1e6, bound=bound)
            if bound in ('mfma', 'valu'):
                # split-bf16 spends 3 bf16 MFMAs per algorithmic product: its roofline is a third of the bf16 peak
                split = self.mode == 'bf16x3' and 'float' not in label and bound != 'valu'
                peak = PEAK_BF16_TFLOPS / 3 if split else (PEAK_F32_TFLOPS if (self.f32 or bound == 'valu' or 'float' in label) else PEAK_BF16_TFLOPS)
                r.update(achieved=work / secs / 1e12, unit='TFLOP/s', peak=peak, algorithmic_flops_per_launch=work / launches)
            elif bound == 'hbm':
                r.update(achieved=work / secs / 1e9, unit='GB/s', peak=PEAK_HBM_GBS, algorithmic_bytes_per_launch=work / launches)
            if 'achieved' in r:
                r['frac'] = r['achieved'] / r['peak']
            rows.append(r)
        rows.sort(key=lambda r: -r['us_total'])
        return rows


def pmc_traffic(kernel, section=None):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes of this bench's legs (counters need their own rocprofv3 runs --
    they cannot be collected from inside this process): the NEWEST profiles/pmc_traffic_rNN.json, written by tools/pmc_traffic.py from separate
    --pmc FETCH_SIZE / WRITE_SIZE passes with the gfx950 x2 read correction.  section None: the bf16 encode leg; 'sample' / 'bf16x3_encode' /
    'bf16x3_sample': the passes of that leg (the same kernel template runs other shapes there)."""
    import glob
    found = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'pmc_traffic_r[0-9][0-9].json')))
    path = found[-1] if found else None
    if path is None:
        return None, None
    try:
        doc = json.load(open(path))
    except (OSError, ValueError):
        return None, None
    tab = doc.get('kernels', {}) if section is None else doc.get('sections', {}).get(section, {})
    key = kernel.replace(' ', '')
    for name, rec in tab.items():
        if name.replace(' ', '') == key:
            return rec.get('hbm_bytes_per_launch'), f"{os.path.basename(path)}{'' if section is None else ' [' + section + ']'}: {doc.get('source')}"
    return None, None


def roofline_of(rows, dtype, with_traffic=True, section=None):
    """the roofline object of a leg: its dominant MFMA kernel by total time; traffic from the committed PMC passes of that leg (`section`)"""
    cand = [r for r in rows if r['bound'] == 'mfma']
    if not cand:
        return None
    r = cand[0]
    traffic, src = pmc_traffic(r['kernel'], section) if with_traffic else (None, None)
    return {'bound': 'mfma', 'kernel': r['kernel'], 'achieved': r['achieved'], 'peak': r['peak'], 'unit': 'TFLOP/s', 'frac': r['frac'],
            'traffic': traffic, 'traffic_unit': 'fabric bytes per launch (L2 memory-side requests: Infinity-Cache hits are counted)', 'traffic_source': src,
            'launches_per_step': r['launches'], 'avg_launch_us': r['avg_us'], 'algorithmic_flops_per_launch': r['algorithmic_flops_per_launch']}


# ------------------------------------------------------------------------------------------ legs

def bench_encode(cv, args, ws, want_kernels, leg='encode', groups=None):
    """`groups` (default args.groups) timed regions of args.steps steps; returns (region times, hipGraph used, kernel rows, token ids of the
    last timed step)"""
    B, R = args.batch, max(1, args.rotate)
    rank = int(os.environ.get('RANK', 0))
    videos = [synthetic_video(B, 17, 256, seed=7 * rank + i).cuda() for i in range(R)]
    # the metric's own entry point: CViViT.forward(video, return_only_codebook_ids=True)
    ids0 = cv(videos[0], return_only_codebook_ids=True)            # builds the packed weights / bias caches
    torch.cuda.synchronize()
    steps_fn = [(lambda v=v: cv(v, return_only_codebook_ids=True)) for v in videos]
    used_graph = False
    if not args.no_graph:
        try:
            replays = []
            for i, f in enumerate(steps_fn):
                rp, out = capture(f)
                rp()
                torch.cuda.synchronize()
                if i == 0:
                    assert torch.equal(out, ids0), 'graph replay changed the token ids'
                replays.append(lambda rp=rp, out=out: (rp(), out)[1])          # a replay refills the captured output tensor
            steps_fn, used_graph = replays, True
        except Exception as e:                     # noqa: BLE001  (recorded in the JSON, never silent)
            print(f'[bench] hipGraph capture failed ({type(e).__name__}: {e}); running eagerly', file=sys.stderr)
            torch.cuda.synchronize()
    last = [None]

    def step(i):
        last[0] = steps_fn[i % R]()
    for i in range(args.warmup):
        step(i)
    times = timed_groups(step, args.steps, args.groups if groups is None else groups, ws)
    ids = last[0].clone()
    rows = None
    if want_kernels:
        with KernelProfiler(leg, args.dtype) as prof:
            cv(videos[0], return_only_codebook_ids=True)
        rows = prof.table()
    return times, used_graph, rows, ids


def bench_encode_big(cv, args, ws, B, want_kernels):
    """the encode leg at B videos per GPU (default 32): same entry point, hipGraph, 2 rotating inputs (2 x 428 MB > Infinity Cache)"""
    import copy
    a = copy.copy(args)
    a.batch, a.rotate, a.groups, a.steps = B, 2, max(5, args.groups // 3), max(5, args.steps // 2)
    times, used_graph, rows, _ = bench_encode(cv, a, ws, want_kernels, leg=f'encode_b{B}')
    med = statistics.median(times)
    out = dict(metric='cvivit_encode_frames_per_sec', value=B * 17 * a.steps * ws / med, unit='frames/s', ms_per_step=med / a.steps * 1e3,
               batch_per_gpu=B, token_rows_per_step=B * 576, hip_graph=used_graph, groups=a.groups, steps=a.steps,
               note='not the BASELINE batch: shows what the same kernels reach when every CU has several tiles')
    if rows:
        out['roofline'] = roofline_of(rows, args.dtype, with_traffic=False)
        flops = sum(r.get('algorithmic_flops_per_launch', 0) * r['launches'] for r in rows if r['bound'] == 'mfma')
        out['step_tflops'] = flops / (med / a.steps) / 1e12
    return out, rows


def bench_decode(cv, args, ws, want_kernels):
    """C-ViViT decode leg (cvivit.py:437-516): (B, 576) token ids -> (B, 3, 17, 256, 256) pixels, frames/s"""
    B, R = args.batch, max(1, args.rotate)
    g = torch.Generator(device='cpu')
    g.manual_seed(5)
    idsets = [torch.randint(0, 65536, (B, 576), generator=g).cuda() for _ in range(R)]
    cv.decode_from_codebook_indices(idsets[0])
    torch.cuda.synchronize()
    fns = [(lambda t=t: cv.decode_from_codebook_indices(t)) for t in idsets]
    used_graph = False
    if not args.no_graph:
        try:
            fns = [capture(f)[0] for f in fns]
            used_graph = True
        except Exception as e:                     # noqa: BLE001
            print(f'[bench] decode hipGraph capture failed ({type(e).__name__}: {e}); running eagerly', file=sys.stderr)
            fns = [(lambda t=t: cv.decode_from_codebook_indices(t)) for t in idsets]
    step = lambda i: fns[i % R]()
    for i in range(args.warmup):
        step(i)
    groups = max(5, args.groups // 3)
    times = timed_groups(step, args.steps, groups, ws)
    med = statistics.median(times)
    out = dict(metric='cvivit_decode_frames_per_sec', value=B * 17 * args.steps * ws / med, unit='frames/s', ms_per_step=med / args.steps * 1e3,
               batch_per_gpu=B, hip_graph=used_graph, groups=groups,
               roofline_note='13.37 MB f32 pixels written per video is the HBM floor (SURVEY.md 8d); per-kernel fractions in `kernels`')
    rows = None
    if want_kernels:
        with KernelProfiler('decode', args.dtype) as prof:
            cv.decode_from_codebook_indices(idsets[0])
        rows = prof.table()
    return out, rows


def _sample_call(ph, B_local, ws, ctx, **kw):
    """one Phenaki.sample of the whole job: B_local videos per GPU; with ws > 1 through sample_sharded, i.e. including the
    RCCL all-gather of the decoded videos (the one collective of the design)"""
    from phenaki_pytorch_amd import sample_sharded
    if ws == 1:
        return ph.sample(texts=['x'] * B_local, num_frames=17, cond_scale=5., **kw)
    return sample_sharded(ph, texts=['x'] * (B_local * ws), num_frames=17, cond_scale=5., **kw)


def collective_info(ws, B):
    """what moved the gathered videos, and how long that one collective takes on its own: the all_gather_into_tensor of sample_sharded
    on a (B, 3, 17, 256, 256) f32 shard per rank, 5 timed repetitions between HIP events on the current stream (max over ranks)"""
    if ws == 1:
        return dict(collective='none (1 GPU)')
    import torch.distributed as dist
    from phenaki_pytorch_amd.dist import all_gather_batch
    backend = dist.get_backend()
    lib = 'RCCL' if backend == 'nccl' else backend
    ver = None
    if backend == 'nccl':
        try:
            ver = '.'.join(str(v) for v in torch.cuda.nccl.version())
        except Exception:                                       # noqa: BLE001
            ver = None
    shard = torch.randn(B, 3, 17, 256, 256, device='cuda')
    all_gather_batch(shard, B * ws)
    barrier_sync(ws)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        all_gather_batch(shard, B * ws)
    e1.record()
    torch.cuda.synchronize()
    us = max_over_ranks(e0.elapsed_time(e1) * 1e3 / 5, ws)
    nbytes = shard.numel() * 4
    return dict(collective=f'one all_gather_into_tensor of ({B},3,17,256,256) f32 per rank ({lib}), inside the timed region',
                backend=backend, nccl_version=ver, all_gather_us=us, shard_bytes=nbytes,
                all_gather_algbw_GBs=nbytes * (ws - 1) / (us * 1e-6) / 1e9)


def bench_sample(ph, args, ws, B, name, want_kernels, leg='sample', runs=3):
    """configs[2] / [3]: 18-step MaskGIT sampling (CFG scale 5, TokenCritic) with frozen random C-ViViT weights and a cached
    (random) T5 context; tokens/sec = global batch * 576 / wall time of the sample call (final decode and, with N > 1, the
    all-gather of the decoded videos included)."""
    ctx = synthetic_context(B, 12, 768, seed=1).cuda()
    ph.encode_texts = lambda texts, output_device=None: ctx[:len(texts)]
    torch.manual_seed(0)
    res = {}
    for mode in (['eager'] if args.no_graph else ['eager', 'graph']):
        ph.enable_sample_graph(mode == 'graph')
        try:
            _sample_call(ph, B, ws, ctx)                       # warm-up (packs weights, position bias; captures the graph)
            _sample_call(ph, B, ws, ctx)
            ts = timed_groups(lambda i: _sample_call(ph, B, ws, ctx), 1, runs, ws)
            res[mode] = statistics.median(ts)
        except Exception as e:                                  # noqa: BLE001
            print(f'[bench] sample leg in {mode} mode failed ({type(e).__name__}: {e})', file=sys.stderr)
            torch.cuda.synchronize()
    ph.enable_sample_graph(False)
    best = min(res, key=res.get)
    dt = res[best]
    out = dict(metric='maskgit_sampled_tokens_per_sec', value=B * 576 * ws / dt, unit='tokens/s', seconds_per_sample_call=dt, launch_mode=best,
               seconds_by_launch_mode=res, batch_per_gpu=B, global_batch=B * ws, steps=ph.steps, cond_scale=5.0,
               critic='TokenCritic depth 6 cross-attn', tokens_per_video=576, noise='in-kernel counter hash (FAST mode)',
               workload=name, **collective_info(ws, B))
    rows = None
    if want_kernels:
        # per-kernel rooflines of this leg: 2 untimed sampling steps under the profiler
        steps = ph.steps
        try:
            ph.steps = 2
            with KernelProfiler(leg, args.dtype) as prof:
                ph.sample(texts=['x'] * B, num_frames=17, cond_scale=5.)
            rows = prof.table()
        finally:
            ph.steps = steps
        sec = {'bf16': 'sample', 'bf16x3': 'bf16x3_sample'}.get(args.dtype) if (leg == 'sample' and B == 8) else None      # the legs the PMC passes cover
        out['roofline'] = roofline_of(rows, args.dtype, with_traffic=sec is not None, section=sec)
    return out, rows


def bench_make_video(ph, args, ws):
    """configs[4]: make_video, 3 scenes of (17, 14, 14) frames, prime K = 5, 256x256, one video per GPU (batch 8 over 8 GPUs);
    1 472 sampled tokens per video; tokens/s and wall-clock of the whole call (priming encodes, 3 x 18 steps, 3 decodes, and with
    N > 1 the single all-gather of the final 45-frame videos)."""
    from phenaki_pytorch_amd import make_video_sharded
    ctx = synthetic_context(1, 12, 768, seed=3).cuda()
    ph.encode_texts = lambda texts, output_device=None: ctx.expand(len(texts), -1, -1).contiguous()
    texts = [['a', 'b', 'c']] * ws
    call = lambda: make_video_sharded(ph, texts, (17, 14, 14), 5)
    res = {}
    # one video per GPU: 2 x 576 token rows per launch, i.e. launch-bound when every kernel is launched from Python -> the captured
    # sampling loops (one hipGraph per scene configuration, Phenaki.enable_sample_graph) are timed beside the eager launches
    for mode in (['eager'] if args.no_graph else ['eager', 'graph']):
        ph.enable_sample_graph(mode == 'graph')
        try:
            video = call()
            assert tuple(video.shape) == (ws, 3, 45, 256, 256), tuple(video.shape)
            call()
            res[mode] = statistics.median(timed_groups(lambda i: call(), 1, 3, ws))
        except Exception as e:                                  # noqa: BLE001
            print(f'[bench] make_video leg in {mode} mode failed ({type(e).__name__}: {e})', file=sys.stderr)
            torch.cuda.synchronize()
    ph.enable_sample_graph(False)
    best = min(res, key=res.get)
    dt = res[best]
    ntok = 576 + 2 * 448
    return dict(metric='make_video_sampled_tokens_per_sec', value=ws * ntok / dt, unit='tokens/s', wall_clock_s=dt, launch_mode=best,
                wall_clock_s_by_launch_mode=res, videos=ws,
                videos_per_gpu=1, scenes=[17, 14, 14], prime_frames=5, tokens_per_video=ntok, frames_out=45)


def bench_scaling_projection(ph, args, result):
    """VERDICT r5 #6b -- what the 1 -> 8 GPU curves of configs[3] / configs[4] would be, PROJECTED from one-GPU measurements (no 8-GPU node was
    ever available to this repo; these are projections and labelled so).  The path shards the batch with no collective inside the loop, so an
    N-GPU run of a fixed job costs one GPU its per-GPU SHARE of the batch plus the one all-gather of the decoded videos:
      t(N) = t_one_gpu(B / N) + t_all_gather(N),   strong scaling S(N) = t(1) / t(N)        (weak scaling: t_one_gpu(B) + t_all_gather(N))
    t_one_gpu is measured here at every share; t_all_gather is MODELLED on the xGMI full mesh (7 links x ~153 GB/s per GPU, point to point):
    'direct' = every rank writes its shard to its 7 peers over 7 links at once (shard / 153 GB/s), 'ring' = one ring over one link per
    hop ((N - 1) shards / 153 GB/s) -- RCCL lands between the two; both are small beside the sampling loop."""
    from phenaki_pytorch_amd import make_video_sharded
    LINK = 153e9
    out = {'note': 'PROJECTION from 1-GPU measurements + an xGMI model; not a multi-GPU measurement', 'xgmi_link_GBs': LINK / 1e9}
    # ---- configs[3]: Phenaki.sample, batch 32 over N GPUs
    t = {}
    have = {32: result.get('sample_b32'), 8: result.get('sample'), 4: result.get('sample_cfg3')}
    for B in (32, 16, 8, 4):
        if have.get(B):
            t[B] = have[B]['seconds_per_sample_call']
        else:
            r, _ = bench_sample(ph, args, 1, B, f'configs[3] share: {B} videos on one GPU', False, runs=2)
            t[B] = r['seconds_per_sample_call']
    rows = []
    for N in (1, 2, 4, 8):
        share = 32 // N
        shard = share * 3 * 17 * 256 * 256 * 4.0
        ag = dict(direct=0.0 if N == 1 else shard / LINK, ring=0.0 if N == 1 else (N - 1) * shard / LINK)
        rows.append(dict(n_gpus=N, videos_per_gpu=share, one_gpu_seconds=t[share], all_gather_model_s=ag,
                         strong_scaling=dict(direct=t[32] / (t[share] + ag['direct']), ring=t[32] / (t[share] + ag['ring'])),
                         tokens_per_s=dict(direct=32 * 576 / (t[share] + ag['direct']), ring=32 * 576 / (t[share] + ag['ring']))))
    out['configs3_sample_batch32'] = rows
    out['configs3_weak'] = [dict(n_gpus=N, videos_per_gpu=4, tokens_per_s_ring=N * 4 * 576 / (t[4] + (0.0 if N == 1 else (N - 1) * 4 * 13369344.0 / LINK)))
                            for N in (1, 2, 4, 8)]
    # ---- configs[4]: make_video, batch 8 over N GPUs (one hipGraph per scene configuration when graphs are on)
    ctx = synthetic_context(1, 12, 768, seed=3).cuda()
    ph.encode_texts = lambda texts, output_device=None: ctx.expand(len(texts), -1, -1).contiguous()
    ph.enable_sample_graph(not args.no_graph)
    tm = {}
    try:
        for B in (8, 4, 2, 1):
            texts = [['a', 'b', 'c']] * B
            call = lambda: make_video_sharded(ph, texts, (17, 14, 14), 5)
            call(); call()
            tm[B] = statistics.median(timed_groups(lambda i: call(), 1, 3, 1))
    finally:
        ph.enable_sample_graph(False)
    ntok = 576 + 2 * 448
    rows = []
    for N in (1, 2, 4, 8):
        share = 8 // N
        shard = share * 3 * 45 * 256 * 256 * 4.0
        ring = 0.0 if N == 1 else (N - 1) * shard / LINK
        rows.append(dict(n_gpus=N, videos_per_gpu=share, one_gpu_seconds=tm[share], all_gather_ring_model_s=ring,
                         strong_scaling_ring=tm[8] / (tm[share] + ring), tokens_per_s_ring=8 * ntok / (tm[share] + ring)))
    out['configs4_make_video_batch8'] = rows
    return out


def bench_objective(ph, args, ws):
    """SURVEY.md 8f row 1, first slice: Phenaki.forward -- the VALUE of the training objective (masked cross entropy without
    logits + token-critic BCE) on B videos' worth of token ids; videos/sec.  Reported beside the headline legs."""
    B = args.sample_batch
    ctx = synthetic_context(B, 12, 768, seed=1).cuda()
    g = torch.Generator(device='cpu')
    g.manual_seed(4)
    ids = torch.randint(0, 65536, (B, 9, 8, 8), generator=g).cuda()
    torch.manual_seed(0)
    ph(video_codebook_ids=ids, text_embeds=ctx)                 # warm-up
    ts = timed_groups(lambda i: ph(video_codebook_ids=ids, text_embeds=ctx), 5, 3, ws)
    dt = statistics.median(ts) / 5
    loss = ph(video_codebook_ids=ids, text_embeds=ctx)
    return dict(metric='phenaki_forward_objective_videos_per_sec', value=B * ws / dt, unit='videos/s', ms_per_call=dt * 1e3,
                batch_per_gpu=B, tokens_per_video=576, loss=float(loss),
                note='forward value only (no autograd graph): MaskGit trunk + vocab head with fused gumbel sampling and '
                     'cross entropy (logits never written) + TokenCritic trunk + BCE; random-init weights, random ids')


def bench_train_step(args, ws, mode):
    """ONE training step of the reference's PhenakiTrainer inner loop (phenaki_trainer.py:351-388) at BASELINE geometry --
    zero_grad, loss = Phenaki.forward(token ids, text embeddings) [MaskGit CE + TokenCritic BCE], loss.backward(), AdamW step on the MaskGit
    and critic parameters -- every arithmetic kernel this library's (train.py, optim.py).  videos/sec; its own models (grad mode on)."""
    import phenaki_pytorch_amd as P
    B = args.sample_batch
    cv, mg, cr, ph = build_models(mode, True)
    for m in (mg, cr):
        m.train()
    ctx = synthetic_context(B, 12, 768, seed=1).cuda()
    g = torch.Generator(device='cpu')
    g.manual_seed(4)
    ids = torch.randint(0, 65536, (B, 9, 8, 8), generator=g).cuda()
    params = [p for p in list(mg.parameters()) + list(cr.parameters()) if p.requires_grad]
    opt = P.get_optimizer(params, lr=1e-4, wd=1e-2)
    torch.manual_seed(0)
    losses = []
    reducer = P.GradientReducer(params) if ws > 1 else None         # 64 MB buckets, each all-reduced (RCCL) as soon as backward has filled it

    def step(i):
        with torch.enable_grad():
            opt.zero_grad(set_to_none=True)
            loss = ph(video_codebook_ids=ids, text_embeds=ctx)
            loss.backward()
        if reducer is not None:
            reducer.finish()
        opt.step()
        losses.append(loss.detach())

    step(0)
    step(1)                                                        # warm-up (allocator, optimizer state)
    torch.cuda.reset_peak_memory_stats()
    ts = timed_groups(step, 3, 3, ws)
    dt = statistics.median(ts) / 3
    out = dict(metric='phenaki_train_step_videos_per_sec', value=B * ws / dt, unit='videos/s', ms_per_step=dt * 1e3, dtype=mode, batch_per_gpu=B,
               tokens_per_video=576, trained_parameters=sum(p.numel() for p in params), loss_first=float(losses[0]), loss_last=float(losses[-1]),
               peak_memory_gb=torch.cuda.max_memory_allocated() / 2 ** 30, optimizer='AdamW (pk_adamw), lr 1e-4, wd 1e-2',
               note='forward + backward + optimizer step on fixed token ids / text embeddings (the tokenizer and T5 are frozen in the reference\'s '
                    'step too); activations f32, every block keeps what its backward needs')
    del cv, mg, cr, ph, opt
    torch.cuda.empty_cache()
    return out


def bench_cvivit_train_step(args, ws, mode):
    """ONE step of the reference's CViViTTrainer generator loop without the GAN terms (cvivit_trainer.py:241-249 with
    use_vgg_and_gan = False) at BASELINE geometry -- zero_grad, loss = CViViT.forward(video) [reconstruction MSE through the straight-through
    LFQ], loss.backward(), AdamW step on every tokenizer parameter (train_cvivit.py).  frames/sec, comparable with the encode headline."""
    import phenaki_pytorch_amd as P
    B = args.batch
    torch.manual_seed(0)
    cv = P.CViViT(use_vgg_and_gan=False, **BASELINE_CFG['cvivit']).cuda().train()
    P.set_compute_dtype(cv, mode)
    video = synthetic_video(B, 17, 256, 5).cuda()
    params = [p for p in cv.parameters() if p.requires_grad]
    opt = P.get_optimizer(params, lr=1e-4, wd=0.)
    reducer = P.GradientReducer(params) if ws > 1 else None
    losses = []

    def step(i):
        with torch.enable_grad():
            opt.zero_grad(set_to_none=True)
            loss = cv(video)
            loss.backward()
        if reducer is not None:
            reducer.finish()
        opt.step()
        losses.append(loss.detach())

    step(0)
    step(1)
    torch.cuda.reset_peak_memory_stats()
    ts = timed_groups(step, 3, 3, ws)
    dt = statistics.median(ts) / 3
    out = dict(metric='cvivit_train_step_frames_per_sec', value=B * 17 * ws / dt, unit='frames/s', ms_per_step=dt * 1e3, dtype=mode, batch_per_gpu=B,
               frames_per_video=17, trained_parameters=sum(p.numel() for p in params), loss_first=float(losses[0]), loss_last=float(losses[-1]),
               peak_memory_gb=torch.cuda.max_memory_allocated() / 2 ** 30, optimizer='AdamW (pk_adamw), lr 1e-4',
               note='forward + backward + optimizer step of the tokenizer on the reconstruction loss (use_vgg_and_gan = False); the GAN objective is the cvivit_gan_step leg')
    del cv, opt
    torch.cuda.empty_cache()
    return out


def bench_cvivit_gan_step(args, ws, mode):
    """SURVEY.md 8f row 4, both halves of one CViViTTrainer.train_step (cvivit_trainer.py:226-270) at BASELINE geometry with use_vgg_and_gan = True:
    (generator) loss = vae(video) [recon + perceptual through a caller-supplied feature network + adaptive_weight * hinge generator loss],
    backward, AdamW on the tokenizer; (discriminator) loss = vae(video, return_discr_loss=True) [hinge + gradient penalty on 256 x 256 frames],
    backward, AdamW on the discriminator.  The perceptual network here is a small pooling + Linear stand-in (torchvision's VGG16 is not available
    offline): its cost is NOT the reference's VGG16 cost, everything else is the reference's step."""
    import phenaki_pytorch_amd as P
    from torch import nn
    B = args.batch
    torch.manual_seed(0)
    vgg = nn.Sequential(nn.AvgPool2d(4), nn.Flatten(), nn.Linear(3 * 64 * 64, 64), nn.Tanh(), nn.Linear(64, 32))
    for q in vgg.parameters():
        q.requires_grad_(False)
    cv = P.CViViT(use_vgg_and_gan=True, vgg=vgg, **BASELINE_CFG['cvivit']).cuda().train()
    P.set_compute_dtype(cv, mode)
    video = synthetic_video(B, 17, 256, 5).cuda()
    gen_params = [p for n, p in cv.named_parameters() if p.requires_grad and not n.startswith('discr.')]
    dis_params = [p for p in cv.discr.parameters() if p.requires_grad]
    opt, dopt = P.get_optimizer(gen_params, lr=1e-4, wd=0.), P.get_optimizer(dis_params, lr=1e-4, wd=0.)
    out = {}

    def gen_step(i):
        with torch.enable_grad():
            opt.zero_grad(set_to_none=True)
            loss = cv(video)
            loss.backward()
        opt.step()
        out['gen_loss'] = loss.detach()

    def discr_step(i, gp=True):
        with torch.enable_grad():
            dopt.zero_grad(set_to_none=True)
            loss = cv(video, return_discr_loss=True, apply_grad_penalty=gp)
            loss.backward()
        dopt.step()
        out['discr_loss'] = loss.detach()

    for fn in (gen_step, discr_step, lambda i: discr_step(i, False)):
        fn(0)
    torch.cuda.reset_peak_memory_stats()
    t_gen = statistics.median(timed_groups(gen_step, 2, 3, ws)) / 2
    t_dis = statistics.median(timed_groups(discr_step, 2, 3, ws)) / 2
    t_dis_nogp = statistics.median(timed_groups(lambda i: discr_step(i, False), 2, 3, ws)) / 2
    # the discriminator's work per step (cvivit.py:141-213 at 256 x 256, B frames): 2 * MACs of its 7 blocks + head
    res = dict(metric='cvivit_gan_step_frames_per_sec', value=B * 17 * ws / (t_gen + t_dis), unit='frames/s', dtype=mode, batch_per_gpu=B,
               generator_step_ms=t_gen * 1e3, discriminator_step_ms=t_dis * 1e3, discriminator_step_no_penalty_ms=t_dis_nogp * 1e3,
               gen_loss=float(out['gen_loss']), discr_loss=float(out['discr_loss']), peak_memory_gb=torch.cuda.max_memory_allocated() / 2 ** 30,
               trained_parameters=dict(tokenizer=sum(p.numel() for p in gen_params), discriminator=sum(p.numel() for p in dis_params)),
               note='one generator step + one discriminator step (gradient penalty on every step; the reference trainer applies it every 4th)')
    del cv, opt, dopt
    torch.cuda.empty_cache()
    return res


def bench_parity_mode(args, ws, mode='bf16x3'):
    """a PARITY-GRADE mode -- a configuration the parity tests hold to bit-exact ids (margin-audited) / 1e-3 against the REAL
    reference -- timed on the same workloads:
      'bf16x3' split-bf16: every product as three bf16 MFMAs on (hi, lo) operand planes, f32 activations (roofline 2.5 PF / 3);
      'fp32'   exact f32 (v_mfma_f32_16x16x4_f32: 157.3 TFLOP/s peak, 1/16 of bf16)."""
    import copy
    a = copy.copy(args)
    a.dtype, a.groups, a.no_graph = mode, max(5, args.groups // 5), args.no_graph
    cv, mg, cr, ph = build_models(mode, not args.no_sample)
    times, used_graph, rows, _ = bench_encode(cv, a, ws, True)
    med = statistics.median(times)
    out = dict(dtype={'fp32': 'f32'}.get(mode, mode), metric='cvivit_encode_frames_per_sec', value=a.batch * 17 * a.steps * ws / med, unit='frames/s',
               ms_per_step=med / a.steps * 1e3, hip_graph=used_graph, roofline=roofline_of(rows, mode, with_traffic=mode == 'bf16x3', section='bf16x3_encode'),
               tolerance='ids bit-exact (margin-audited), logits / pixels 1e-3 vs the reference goldens (tests/test_modules_gpu.py)')
    if not args.no_sample:
        s, _ = bench_sample(ph, a, ws, args.sample_batch, f'BASELINE configs[2] in {mode}', True)
        out['sample'] = {k: s[k] for k in ('metric', 'value', 'unit', 'seconds_per_sample_call', 'launch_mode', 'batch_per_gpu', 'roofline') if k in s}
    del cv, mg, cr, ph
    torch.cuda.empty_cache()
    return out


def cpu_baseline(args):
    """the CPU oracle (port of the reference algorithm) on a bounded sample: B = 2 videos per call, repeated for
    ~cpu_seconds; frames/sec on this box's host cores; then ONE real (short) Phenaki.sample of the port: 4 steps, B = 1."""
    from oracle import phenaki_oracle as O
    from oracle import weights
    from oracle.configs import FULL, oracle_cfgs, state_dicts
    from oracle import hostcpu
    hostcpu.configure()          # fastest thread count <= affinity / cgroup quota (os.cpu_count() oversubscribes GPU boxes)
    cv_sd, mg_sd, cr_sd = state_dicts('full')
    cvc, mgc, crc = oracle_cfgs(FULL)
    video = weights.synthetic_video(2, 17, 256, 256, seed=0)
    with torch.no_grad():
        O.cvivit_tokenize(cv_sd, cvc, video)
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < args.cpu_seconds:
            O.cvivit_tokenize(cv_sd, cvc, video)
            n += 1
        dt = time.perf_counter() - t0
    out = dict(value=n * 2 * 17 / dt, unit='frames/s', cores=torch.get_num_threads(), kind='port',
               sample=f'{n} calls of oracle cvivit_tokenize on (2,3,17,256,256) f32, {dt:.1f} s')
    # the REAL reference timed at survey time on the build container's 8 cores; /root/reference does not exist on the GPU box
    out['reference_measured'] = {'encode_frames_per_sec': 186.0, 'sample_tokens_per_sec': 24.5, 'cores': 8, 'where': 'SURVEY.md 6, build container'}
    if not args.no_sample:
        ctx = weights.synthetic_context(1, 12, 768, seed=1)
        steps = 4
        nf = lambda kind, step, shape: weights.uniform_noise(tuple(shape), 100 + 2 * step + (1 if kind == 'critic' else 0))
        with torch.no_grad():
            t0 = time.perf_counter()
            O.sample(cv_sd, cvc, mg_sd, mgc, cr_sd, crc, num_frames=17, batch_size=1, context=ctx, steps=steps, cond_scale=5., noise_fn=nf)
            ts = time.perf_counter() - t0
        out['sample'] += f'; sampler: one real oracle.sample, {steps} steps (of 18), B=1, CFG 5, TokenCritic, incl. decode: {ts:.1f} s'
        # per-step cost is constant (every step runs the full 2 x 576-token trunks): 18 steps ~ 18/4 of the timed loop
        out['sample_tokens_per_sec'] = 576 / (ts * 18 / steps)
        out['sample_kind'] = 'port, 4 of 18 steps timed, scaled by 18/4'
    return out


def _r(x, nd=4):
    return round(x, nd) if isinstance(x, float) else x


def compact_line(full):
    """the ONE line the driver parses (<= 4 KB): headline + roofline + cpu_baseline + the parity-grade mode + the sampler metric.  Everything
    else (per-kernel table, b32 / training / make_video legs) goes to gpurun_out/bench_full.json and to stderr."""
    keep = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data')
    line = {k: _r(full[k]) for k in keep if k in full}
    cfg = full.get('config', {})
    line['config'] = {k: cfg[k] for k in ('workload', 'global_batch', 'parallelism', 'hip_graph') if k in cfg}
    rf = full.get('roofline')
    if rf:
        line['roofline'] = {k: _r(rf[k]) for k in ('bound', 'kernel', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'launches_per_step', 'avg_launch_us',
                                                   'algorithmic_flops_per_launch') if k in rf}
    hb = full.get('roofline_hbm')
    if hb:
        line['roofline_hbm'] = {k: _r(v) for k, v in hb.items()}
    cb = full.get('cpu_baseline')
    if cb:
        line['cpu_baseline'] = {k: _r(cb[k]) for k in ('value', 'unit', 'cores', 'kind', 'sample', 'sample_tokens_per_sec', 'reference_measured') if k in cb}
        line['cpu_baseline']['sample'] = str(line['cpu_baseline'].get('sample', ''))[:200]
    sm = full.get('sample')
    if sm:
        line['sample'] = {'metric': sm['metric'], 'value': _r(sm['value'], 1), 'unit': sm['unit'], 'ms': _r(sm['seconds_per_sample_call'] * 1e3, 3),
                          'batch_per_gpu': sm['batch_per_gpu'], 'launch_mode': sm['launch_mode']}
        for k in ('global_batch', 'collective', 'backend', 'nccl_version', 'all_gather_us', 'shard_bytes'):      # what moved the videos (N > 1)
            if k in sm:
                line['sample'][k] = _r(sm[k])
        if sm.get('roofline'):
            line['sample']['roofline_frac'] = _r(sm['roofline']['frac'])
            line['sample']['roofline_kernel'] = sm['roofline']['kernel']
    pm = full.get('parity_mode')
    if pm:
        par = {'dtype': pm['dtype'], 'encode_frames_per_sec': _r(pm['value'], 1), 'encode_ms_per_step': _r(pm['ms_per_step']),
               'tolerance': 'ids bit-exact, logits/pixels 1e-3 vs reference goldens'}
        if pm.get('roofline'):
            par['roofline_frac'] = _r(pm['roofline']['frac'])
            par['roofline_kernel'] = pm['roofline']['kernel']
        if pm.get('sample'):
            par['sample_tokens_per_sec'] = _r(pm['sample']['value'], 1)
        line['parity'] = par
    pf = full.get('parity_mode_f32')
    if pf:
        line['parity_f32'] = {'encode_frames_per_sec': _r(pf['value'], 1)}
        if pf.get('sample'):
            line['parity_f32']['sample_tokens_per_sec'] = _r(pf['sample']['value'], 1)
    for leg, key in (('decode', 'value'), ('make_video', 'value'), ('train_step', 'ms_per_step'), ('train_step_bf16', 'ms_per_step'),
                     ('cvivit_train_step', 'ms_per_step'), ('cvivit_gan_step', 'generator_step_ms'), ('encode_b32', 'value'), ('sample_b32', 'value'), ('sample_cfg3', 'value')):
        if leg in full and key in full[leg]:
            line.setdefault('legs', {})[leg] = {key: _r(full[leg][key], 3), 'unit': full[leg].get('unit')}
    sp = full.get('scaling_projection')
    if sp:
        r8 = sp['configs3_sample_batch32'][-1]
        m8 = sp['configs4_make_video_batch8'][-1]
        line['scaling_projection'] = {'note': 'projected from 1-GPU shares + xGMI ring model, NOT measured', 'configs3_strong_8gpu': _r(r8['strong_scaling']['ring'], 3),
                                      'configs4_strong_8gpu': _r(m8['strong_scaling_ring'], 3)}
    line['full_report'] = 'gpurun_out/bench_full.json (also on stderr)'
    return line


def emit(full):
    """full report -> gpurun_out/bench_full.json + stderr; compact line (<= 4 KB) -> the LAST line of stdout"""
    text = json.dumps(full)
    try:
        os.makedirs(os.path.join(ROOT, 'gpurun_out'), exist_ok=True)
        with open(os.path.join(ROOT, 'gpurun_out', 'bench_full.json'), 'w') as f:
            f.write(text + '\n')
    except OSError as e:
        print(f'[bench] could not write gpurun_out/bench_full.json ({e})', file=sys.stderr)
    print('[bench] full report: ' + text, file=sys.stderr)
    sys.stderr.flush()
    line = json.dumps(compact_line(full), separators=(',', ':'))
    while len(line) > 4000:                                     # never let the parsed line grow past the driver's window again
        c = json.loads(line)
        for k in ('scaling_projection', 'legs', 'parity_f32', 'roofline_hbm', 'sample'):
            if k in c:
                del c[k]
                break
        else:
            c['config'] = {'workload': c['config']['workload'][:120]}
            line = json.dumps(c, separators=(',', ':'))
            break
        line = json.dumps(c, separators=(',', ':'))
    print(line)
    sys.stdout.flush()


def main():
    args = parse()
    spawn_ranks_if_needed(args)
    torch.set_grad_enabled(False)
    from __graft_entry__ import build
    rank, local, ws = init_dist(args.gpus)
    if rank == 0:
        build()
    barrier_sync(ws)
    sampler = args.full and not (args.no_sample or args.encode_only)
    cv, mg, cr, ph = build_models(args.dtype, sampler)
    want_k = not (args.no_kernels or args.encode_only)

    times, used_graph, enc_rows, ids = bench_encode(cv, args, ws, args.full and not args.no_kernels, groups=1)
    med = times[0]
    frames = args.batch * 17 * args.steps * ws
    result = {
        'metric': 'cvivit_encode_frames_per_sec', 'value': frames / med, 'unit': 'frames/s', 'n_gpus': ws,
        'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': med / args.steps * 1e3, 'higher_is_better': True,
        'scaling': 'weak', 'vs_baseline': None, 'dtype': args.dtype if args.dtype == 'bf16' else 'f32', 'data': 'synthetic',
        'config': {'workload': 'BASELINE configs[1]: C-ViViT (dim 512, patch 32, tpatch 2, depth 4+4, LFQ 65536) encode '
                               f'video -> token ids, ({args.batch},3,17,256,256) f32 per GPU resident in HBM',
                   'global_batch': args.batch * ws, 'frames_per_video': 17, 'parallelism': f'batch-shard x{ws}, no data-path collective',
                   'hip_graph': used_graph, 'input_rotation': f'{args.rotate} distinct batches ({args.rotate * args.batch * 13.37:.0f} MB) per GPU',
                   'timing': f'one region of {args.steps} steps after {args.warmup} warm-up steps, {med:.4f} s'},
    }
    if args.dump_outputs:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        name = 'ids' if ws == 1 else f'ids_rank{rank}'
        np.save(os.path.join(args.dump_outputs, name + '.npy'), ids.cpu().numpy().astype(np.float64))
    if not args.full:
        if rank == 0:
            line = {k: v for k, v in compact_line(result).items() if k != 'full_report'}         # a plain run writes no full report
            print(json.dumps(line, separators=(',', ':')))
            sys.stdout.flush()
        if ws > 1:
            import torch.distributed as dist
            dist.destroy_process_group()
        return
    kernels = []
    if enc_rows:
        result['roofline'] = roofline_of(enc_rows, args.dtype)
        kernels += enc_rows
        pe = [r for r in enc_rows if r['kernel'].startswith(('patch_embed', 'patchify_ln', 'gemm_dma_splitk', 'sum_batch'))]
        if pe:
            # the north star's first-named kernel on the axis SURVEY 8d prescribes for it: the whole patch embedding (every launch it takes in
            # this mode) against the f32 video bytes it has to read once + the token rows it writes
            us = sum(r['us_total'] for r in pe)
            alg = args.batch * 3 * 17 * 256 * 256 * 4.0 + args.batch * 576 * 512 * 6.0
            result['roofline_hbm'] = {'kernel': 'patch embedding (' + ' + '.join(sorted({r['kernel'] for r in pe})) + ')', 'bound': 'hbm', 'us': us,
                                      'algorithmic_bytes': alg, 'achieved': alg / us / 1e3, 'unit': 'GB/s', 'peak': PEAK_HBM_GBS, 'frac': alg / us / 1e3 / PEAK_HBM_GBS}
    legs = set() if args.encode_only else set(x for x in args.legs.split(',') if x)
    if 'decode' in legs:
        result['decode'], dec_rows = bench_decode(cv, args, ws, want_k)
        kernels += dec_rows or []
    if 'encode_b32' in legs:
        # the same leg with the GPU full (32 videos = 18 432 token rows per GPU): separates "the kernels' ceiling" from "B = 8 is one
        # partial wave of tiles" -- the headline stays the BASELINE batch of 8
        result['encode_b32'], b32_rows = bench_encode_big(cv, args, ws, 32, want_k)
        kernels += b32_rows or []
    if sampler and 'sample' in legs:
        result['sample'], s_rows = bench_sample(ph, args, ws, args.sample_batch, 'BASELINE configs[2]', want_k)
        kernels += s_rows or []
    if sampler and 'sample_cfg3' in legs:
        s3, _ = bench_sample(ph, args, ws, 4, 'BASELINE configs[3] per-GPU share (32 videos over 8 GPUs = 4 per GPU)', False)
        result['sample_cfg3'] = s3
    if sampler and 'sample_b32' in legs:
        result['sample_b32'], sb_rows = bench_sample(ph, args, ws, 32, 'configs[2] with 32 videos per GPU (GPU full: 36 864 trunk rows per step)', want_k,
                                                      leg='sample_b32', runs=2)
        kernels += sb_rows or []
    if sampler and 'make_video' in legs:
        result['make_video'] = bench_make_video(ph, args, ws)
    if sampler and 'scaling_projection' in legs and ws == 1:
        try:
            result['scaling_projection'] = bench_scaling_projection(ph, args, result)
        except Exception as e:                                  # noqa: BLE001
            print(f'[bench] scaling_projection leg failed ({type(e).__name__}: {e})', file=sys.stderr)
            torch.cuda.synchronize()
    if sampler and 'objective' in legs:
        result['objective'] = bench_objective(ph, args, ws)
    if kernels:
        keep = ('kernel', 'leg', 'launches', 'avg_us', 'bound', 'achieved', 'unit', 'peak', 'frac')
        result['kernels'] = [{k: (round(r[k], 4) if isinstance(r[k], float) else r[k]) for k in keep if k in r} for r in kernels]
    del cv, mg, cr, ph
    torch.cuda.empty_cache()
    if sampler and 'train_step' in legs:
        try:
            result['train_step'] = bench_train_step(args, ws, 'bf16x3' if args.dtype == 'bf16' else args.dtype)
            if args.dtype == 'bf16':
                result['train_step_bf16'] = bench_train_step(args, ws, 'bf16')
        except Exception as e:                                  # noqa: BLE001 -- a training-leg failure must not cost the headline line
            print(f'[bench] train_step leg failed ({type(e).__name__}: {e})', file=sys.stderr)
            torch.cuda.synchronize()
    if 'cvivit_gan_step' in legs and not args.encode_only:
        try:
            result['cvivit_gan_step'] = bench_cvivit_gan_step(args, ws, 'bf16x3' if args.dtype == 'bf16' else args.dtype)
        except Exception as e:      # noqa: BLE001
            print(f'[bench] cvivit_gan_step leg failed ({type(e).__name__}: {e})', file=sys.stderr)
    if 'cvivit_train_step' in legs and not args.encode_only:
        try:
            result['cvivit_train_step'] = bench_cvivit_train_step(args, ws, 'bf16x3' if args.dtype == 'bf16' else args.dtype)
        except Exception as e:                                  # noqa: BLE001
            print(f'[bench] cvivit_train_step leg failed ({type(e).__name__}: {e})', file=sys.stderr)
            torch.cuda.synchronize()
    if not (args.no_parity_mode or args.encode_only) and args.dtype == 'bf16':
        result['parity_mode'] = bench_parity_mode(args, ws, 'bf16x3')
        result['parity_mode_f32'] = bench_parity_mode(args, ws, 'fp32')
        for k in ('value',):
            f32v, x3v = result['parity_mode_f32'][k], result['parity_mode'][k]
            result['parity_mode']['speedup_vs_exact_f32'] = dict(encode=x3v / f32v)
        if 'sample' in result['parity_mode'] and 'sample' in result['parity_mode_f32']:
            result['parity_mode']['speedup_vs_exact_f32']['sample'] = result['parity_mode']['sample']['value'] / result['parity_mode_f32']['sample']['value']
    if rank == 0 and ws == 1 and not (args.no_cpu or args.encode_only):
        result['cpu_baseline'] = cpu_baseline(args)
    if rank == 0:
        emit(result)
    if ws > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
