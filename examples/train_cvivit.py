"""The training step of the reference's CViViTTrainer (cvivit_trainer.py:226-270) on the MI355X kernels.  Default: the generator step without
the GAN terms -- zero_grad -> CViViT.forward (reconstruction MSE through the straight-through LFQ) -> backward -> [gradient all-reduce] -> AdamW.
`--gan`: both halves of train_step -- the generator objective recon + perceptual + adaptive_weight * hinge generator loss (cvivit.py:585-671; the
perceptual network is whatever module is passed as `vgg=`: by default a small stand-in, because torchvision's pretrained VGG16 cannot be downloaded
offline; `--vgg16 PATH` loads a torchvision vgg16 state dict into P.VGG16Features, the reference's network on this library's kernels), then the
discriminator's hinge loss with the gradient penalty every `--gp-every`-th step (cvivit_trainer.py:224, 251-270).  Finally the
reconstruction of one batch is written as a GIF (data.py:103-113).  `--folder` trains on the GIFs of a directory through VideoDataset /
DataLoader (data.py:177-265); without it synthetic videos stand in.  One process per GPU (`torchrun --nproc-per-node N ...`).

    python examples/train_cvivit.py --steps 20 --small --gif /tmp/recon.gif
    python examples/train_cvivit.py --steps 20 --small --gan
    python examples/train_cvivit.py --steps 20 --gan --vgg16 vgg16.pt
    python examples/train_cvivit.py --steps 20 --small --vq-kmeans-init --vq-dead-code 2
    python examples/train_cvivit.py --steps 20 --small --ema --eval-every 10

`--vq-kmeans-init` / `--vq-dead-code T` train the Phenaki paper's cosine-sim VectorQuantize tokenizer (lookup_free_quantization=False) with the
published module's codebook upkeep: k-means initialisation from the first batch, and replacement of codes whose EMA cluster size fell below T.
Under torchrun the codebook statistics are computed from every rank's rows (sync_codebook), so all ranks keep one codebook.

`--eval-every N` is the validation step of the reference's trainer (cvivit_trainer.py:284-323, every save_results_every steps the EMA tokenizer
reconstructs held-out clips) with numbers instead of image grids: every N steps rank 0 runs `--eval-batches` held-out batches through
P.TokenizerMetrics (the EMA copy with `--ema`) and prints PSNR, SSIM, the number of codes in use and the perplexity of the code histogram.
Under torchrun the validation is rank 0's alone (`compute(merge=False)`: no collective, the other ranks do not wait for it).
"""
import argparse
import contextlib
import os
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phenaki_pytorch_amd as P  # noqa: E402
from phenaki_pytorch_amd.data import DataLoader, VideoDataset, video_tensor_to_gif  # noqa: E402


def perceptual_stand_in(size):
    """any nn.Module mapping (B, 3, H, W) frames to features serves as `vgg=` (cvivit.py:346-347); offline there is no pretrained VGG16"""
    from torch import nn
    net = nn.Sequential(nn.AvgPool2d(4), nn.Flatten(), nn.Linear(3 * (size // 4) ** 2, 256), nn.Tanh(), nn.Linear(256, 64))
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--frames', type=int, default=17)
    ap.add_argument('--dtype', default='bf16x3', choices=['fp32', 'bf16x3', 'bf16'])
    ap.add_argument('--small', action='store_true', help='a small geometry (dim 128, 64 x 64 pixels) instead of the BASELINE one')
    ap.add_argument('--folder', default='', help='directory of GIFs to train on (VideoDataset); default: synthetic videos')
    ap.add_argument('--gif', default='', help='write the reconstruction of the last batch here')
    ap.add_argument('--save', default='')
    ap.add_argument('--max-grad-norm', type=float, default=None, help='clip the global gradient norm inside the AdamW update (cvivit_trainer.py:245-246)')
    ap.add_argument('--discr-max-grad-norm', type=float, default=None, help='the same for the discriminator optimizer of --gan (cvivit_trainer.py:268-269)')
    ap.add_argument('--ema', action='store_true', help='keep an exponential moving average of the tokenizer (cvivit_trainer.py:93, 282); saved as <save>.ema.pt')
    ap.add_argument('--gan', action='store_true', help='train with the perceptual + adversarial objective and a discriminator step')
    ap.add_argument('--vgg16', default='', metavar='PATH', help='with --gan: a torchvision vgg16 state dict (torch.save(vgg16.state_dict(), PATH)); the '
                    'perceptual network is then the real VGG16 (P.VGG16Features) instead of the stand-in')
    ap.add_argument('--gp-every', type=int, default=4, help='apply the gradient penalty every this many steps (cvivit_trainer.py:224)')
    ap.add_argument('--vq-kmeans-init', action='store_true', help='the cosine-sim VectorQuantize tokenizer, its codebook initialised by k-means on the first batch')
    ap.add_argument('--vq-dead-code', type=float, default=0., metavar='T', help='the cosine-sim VectorQuantize tokenizer with threshold_ema_dead_code = T: '
                    'a code whose EMA cluster size falls below T is replaced by a row of the batch')
    ap.add_argument('--eval-every', type=int, default=0, metavar='N', help='every N steps rank 0 validates on held-out clips: PSNR, SSIM, codebook usage '
                    '(the EMA tokenizer with --ema)')
    ap.add_argument('--eval-batches', type=int, default=2, metavar='K', help='held-out batches per validation')
    args = ap.parse_args()
    ws = int(os.environ.get('WORLD_SIZE', '1'))
    if ws > 1:
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
        dist.init_process_group('nccl')
    rank = dist.get_rank() if ws > 1 else 0
    torch.manual_seed(1)                   # the model is built under a rank-INDEPENDENT seed (and GradientReducer broadcasts rank 0's weights anyway)

    dim, size, patch, vocab = (128, 64, 16, 256) if args.small else (512, 256, 32, 65536)
    vgg = None
    use_vq = args.vq_kmeans_init or args.vq_dead_code > 0
    if args.gan:
        # .eval(): the reference's trainer leaves the VGG's Dropout(0.5) active (vae.train() reaches it); a fixed feature extractor is the evident intent
        vgg = P.VGG16Features().load(args.vgg16).eval() if args.vgg16 else perceptual_stand_in(size)
    cvivit = P.CViViT(dim=dim, codebook_size=vocab, image_size=size, patch_size=patch, temporal_patch_size=2, spatial_depth=2 if args.small else 4,
                      temporal_depth=2 if args.small else 4, dim_head=64, heads=dim // 64, use_vgg_and_gan=args.gan,
                      vgg=vgg, lookup_free_quantization=not use_vq)
    if use_vq:
        # the reference constructs the quantizer without keywords (cvivit.py:321): replace it (k-means starts from an empty codebook) and set the threshold
        if args.vq_kmeans_init:
            cvivit.vq = P.quantize.VectorQuantize(dim=dim, codebook_size=vocab, kmeans_init=True)
        cvivit.vq.threshold_ema_dead_code = args.vq_dead_code
    cvivit = cvivit.cuda().train()
    if args.vgg16:
        cvivit.vgg.eval()
    P.set_compute_dtype(cvivit, args.dtype)
    # the reference keeps two optimizers: the tokenizer's parameters (everything but discr.*) and the discriminator's (cvivit_trainer.py:118-124)
    params = [p for n, p in cvivit.named_parameters() if p.requires_grad and not n.startswith('discr.')]
    opt = P.get_optimizer(params, lr=3e-4, wd=0., max_grad_norm=args.max_grad_norm)
    discr_params = list(cvivit.discr.parameters()) if args.gan else []
    discr_opt = P.get_optimizer(discr_params, lr=3e-4, wd=0., max_grad_norm=args.discr_max_grad_norm) if args.gan else None
    reducer = P.GradientReducer(params, buffers=list(cvivit.buffers())) if ws > 1 else None     # broadcasts rank 0's parameters, as DDP does at wrap time
    discr_reducer = P.GradientReducer(discr_params) if (ws > 1 and args.gan) else None
    ema = P.EMA(cvivit, update_after_step=min(100, args.steps // 2), update_every=10 if args.steps > 40 else 1) if (args.ema and rank == 0) else None
    torch.manual_seed(1 + rank)            # from here on (data order, frame masks) every rank draws its own stream

    if args.folder:
        loader = DataLoader(VideoDataset(args.folder, size, num_frames=args.frames), batch_size=args.batch, shuffle=True, drop_last=True)

        def batches():
            while True:
                for (clip,) in loader:
                    yield clip.cuda()
        stream = batches()
    else:
        fixed = torch.rand(args.batch, 3, args.frames, size, size, device='cuda')
        stream = iter(lambda: fixed, None)

    def held_out():
        """--eval-batches held-out batches: a second pass over the folder in its own fixed order, or a second fixed synthetic clip"""
        if args.folder:
            g = torch.Generator().manual_seed(12345)
            second = DataLoader(VideoDataset(args.folder, size, num_frames=args.frames), batch_size=args.batch, shuffle=True, drop_last=True, generator=g)
            for i, (clip,) in enumerate(second):
                if i >= args.eval_batches:
                    break
                yield clip.cuda()
        else:
            g = torch.Generator(device='cuda').manual_seed(12345)
            clip = torch.rand(args.batch, 3, args.frames, size, size, device='cuda', generator=g)
            for _ in range(args.eval_batches):
                yield clip

    def validate(step):
        model = ema.ema_model if ema is not None else cvivit
        tm = P.TokenizerMetrics(model)
        for clip in held_out():
            tm.update(clip)                                            # device-side sums only
        # the one synchronisation.  merge=False: only rank 0 validates (it holds the only EMA copy) while the other ranks go on to their next step,
        # so nothing may be sent here -- compute()'s default sums the state over the process group and is a collective every rank would have to join
        r = tm.compute(merge=False)
        print(f'eval: step {step:4d}  psnr {r["psnr"]:.2f} dB  ssim {r["ssim"]:.4f}  codes used {r["codes_used"]}/{r["codebook_size"]}  '
              f'perplexity {r["perplexity"]:.1f}', flush=True)

    t0 = None
    for step in range(args.steps):
        if step == 3:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        videos = next(stream)
        opt.zero_grad(set_to_none=True)
        loss = cvivit(videos)
        # the generator objective also reaches discr.* through gen_loss: those gradients are dropped below (discr_opt.zero_grad), so their
        # reducer must not start collectives for them -- a launched bucket would meet the discriminator step's own backward
        with (discr_reducer.no_sync() if discr_reducer is not None else contextlib.nullcontext()):
            loss.backward()
        if reducer is not None:
            reducer.finish()
        opt.step()
        discr_loss = None
        if args.gan:
            discr_opt.zero_grad(set_to_none=True)                      # also drops what the generator objective left in discr.*.grad
            discr_loss = cvivit(next(stream), return_discr_loss=True, apply_grad_penalty=(step % args.gp_every == 0))
            discr_loss.backward()
            if discr_reducer is not None:
                discr_reducer.finish()
            discr_opt.step()
        if ema is not None:
            ema.update()                                               # after the step's optimizer updates (cvivit_trainer.py:282)
        if rank == 0 and (step % 5 == 0 or step == args.steps - 1):
            tail = f'  discriminator loss {float(discr_loss.detach()):.5f}' if discr_loss is not None else ''
            print(f'step {step:4d}  {"vae" if args.gan else "reconstruction"} loss {float(loss.detach()):.5f}{tail}', flush=True)
        if rank == 0 and args.eval_every > 0 and (step + 1) % args.eval_every == 0:
            validate(step + 1)
    torch.cuda.synchronize()
    if rank == 0 and t0 is not None and args.steps > 3:
        dt = (time.perf_counter() - t0) / (args.steps - 3)
        print(f'{dt * 1e3:.1f} ms per step, {args.batch * args.frames * ws / dt:.0f} frames/s')
    if rank == 0 and args.gif:
        with torch.no_grad():
            recon = cvivit.eval()(videos[:1], return_recons_only=True)
        video_tensor_to_gif(recon[0].clamp(0, 1).cpu(), args.gif)
        print('wrote', args.gif)
    if rank == 0 and args.save:
        torch.save(cvivit.state_dict(), args.save)
        if ema is not None:
            torch.save(ema.state_dict(), args.save + '.ema.pt')
    if ws > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
