"""Times the validation metrics at the benchmark geometry, two f32 videos (8, 3, 17, 256, 256) of 107 MB each, with device events, the variants
alternating in one process:

  ssim          phenaki_pytorch_amd.ssim (pk_frame_ssim)
  ssim_torch    torch's own f32 formulation on the same device: one grouped F.conv2d of the five maps a, b, a^2, b^2, ab with the 11 x 11
                window, then the point formula and the means (the yardstick; the raw-pixel moments, as pytorch-msssim forms them)
  mse           phenaki_pytorch_amd.frame_mse (pk_frame_sqerr)
  psnr          the same pass with the PSNR output (phenaki_pytorch_amd.psnr)
  mse_torch     ((a - b) ** 2).mean(dim=(1, 3, 4))

and writes the times, the achieved GB/s (the two videos read once: 2 x 4 x numel bytes over the time) and the agreement of the variants to --out.

    python tools/metrics_time.py [--iters 20] [--rounds 3] [--out profiles/metrics_time.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phenaki_pytorch_amd as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (8, 3, 17, 256, 256)


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


def window():
    x = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(x * x) / (2 * 1.5 ** 2))
    g = g / g.sum()
    return torch.outer(g, g).float().cuda()[None, None].expand(5, 1, 11, 11).contiguous()


def ssim_torch(a, b, win, data_range=1.):
    B, C, Fr, H, W = a.shape
    x, y = a.permute(0, 2, 1, 3, 4).reshape(B * Fr * C, 1, H, W), b.permute(0, 2, 1, 3, 4).reshape(B * Fr * C, 1, H, W)
    m1, m2, e11, e22, e12 = F.conv2d(torch.cat((x, y, x * x, y * y, x * y), dim=1), win, groups=5).unbind(dim=1)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    smap = ((2 * m1 * m2 + c1) / (m1 * m1 + m2 * m2 + c1)) * ((2 * (e12 - m1 * m2) + c2) / ((e11 - m1 * m1) + (e22 - m2 * m2) + c2))
    return smap.mean(dim=(1, 2)).view(B, Fr, C).mean(dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'metrics_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    g = torch.Generator(device='cuda').manual_seed(0)
    a = torch.rand(SHAPE, device='cuda', generator=g)
    b = (a + 0.05 * torch.randn(SHAPE, device='cuda', generator=g)).contiguous()
    win = window()
    variants = dict(ssim=lambda: P.ssim(a, b), ssim_torch=lambda: ssim_torch(a, b, win), mse=lambda: P.frame_mse(a, b),
                    psnr=lambda: P.psnr(a, b), mse_torch=lambda: ((a - b) ** 2).mean(dim=(1, 3, 4)))
    with torch.no_grad():
        results = {}
        for k, fn in variants.items():                       # warm-up: code objects, workspaces, the conv algorithm
            for _ in range(3):
                results[k] = fn()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn, args.iters))
    gbytes = 2 * 4 * a.numel() / 1e9
    lines = [f'Validation metrics at {SHAPE} f32 (two videos of {4 * a.numel() / 1e6:.0f} MB), tools/metrics_time.py --iters {args.iters} --rounds {args.rounds}',
             f'device: {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds of {args.iters} back-to-back calls between device events,',
             'the variants alternating; GB/s = the two videos read once over the time', '']
    med = {k: statistics.median(ts) for k, ts in times.items()}
    for k, ts in times.items():
        lines.append(f'  {k:<11s} {med[k]:9.4f} ms   spread {max(ts) - min(ts):7.4f} ms   {gbytes / (med[k] * 1e-3):8.1f} GB/s')
    lines += ['', f'  ssim kernel vs torch formulation: {med["ssim_torch"] / med["ssim"]:.2f}x '
              + ('(the kernel is FASTER)' if med['ssim'] < med['ssim_torch'] else '(the kernel is NOT faster than the torch formulation)'),
              f'  mse kernel vs torch formulation:  {med["mse_torch"] / med["mse"]:.2f}x',
              f'  max |ssim - ssim_torch| = {float((results["ssim"] - results["ssim_torch"]).abs().max()):.2e}   '
              f'max rel |mse - mse_torch| = {float(((results["mse"] - results["mse_torch"]).abs() / results["mse_torch"]).max()):.2e}']
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
