"""Timing of the VGG16 perceptual network's 13 convolutions on the MI355X (GPU only: no device, no numbers).

Shape: 16 frames of 256 x 256, full widths, each compute type.  Legs, per layer and summed over the 13 layers:
    fwd        relu(conv(x) + b) on 16 frames
    fwd+bwd    the same on 8 frames plus the input gradient of relu(conv) on those 8 frames (what the reconstructed-frame branch of a generator step runs)
Three sides, alternated layer by layer inside one process (device events around each side's launches, median of the repeats, spread = (max - min) / median):
    a  pk_conv3x3: the direct convolution of VGG16Features (the ReLU backward fused into the backward-data convolution through the gate operand)
    b  pk_im2col + pk_gemm (+ pk_leaky_bwd, pk_gemm, pk_col2im backward): the same layers on the patch-matrix path the discriminator uses
    c  torch.nn.functional.conv2d in f32 (NCHW, MIOpen through torch autograd): what a caller passing torchvision's module gets
FLOP/s come from the shape arithmetic below (2 M Co 9 C per convolution, padding channels of the first layer included for a and b, 3 channels for c).
Also recorded: the tile choice of pk_conv3x3 on the short-and-wide deep layers (64 x 64 against 128 x 128 tiles), and the whole module forward /
forward + backward (pools and classifier included) against the torch.nn network.

    python tools/vgg_time.py [--out profiles/vgg16_perceptual.txt] [--frames 16] [--size 256] [--repeats 5]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS = (64, 128, 256, 512, 512)
LAYOUT = (2, 2, 3, 3, 3)


def layers(size):
    """[(name, H, C, Co)] of the 13 convolutions at a size x size input (C = 8 for the padded 3-channel frame)"""
    out, C, H = [], 8, size
    for blk, (w, n) in enumerate(zip(WIDTHS, LAYOUT), 1):
        for i in range(1, n + 1):
            out.append((f'conv{blk}_{i}', H, C, w))
            C = w
        H //= 2
    return out


def conv_flops(B, H, C, Co):
    return 2.0 * B * H * H * Co * 9 * C


def timed_alternating(fns, repeats, warmup=2):
    """{name: [ms] * repeats}: every function warmed up, then one timed call of each per round, round after round"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return ts


def timed(fn, repeats):
    return timed_alternating(dict(f=fn), repeats)['f']


def med(ts):
    return statistics.median(ts)


def spread(ts):
    return (max(ts) - min(ts)) / med(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vgg16_perceptual.txt'))
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--dtypes', default='fp32,bf16,bf16x3')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/vgg_time.py measures on the GPU; there is none here (no CPU fallback, no numbers)')
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd import _lib as L
    from phenaki_pytorch_amd.attention import resolve_dtype
    from phenaki_pytorch_amd.discriminator import _conv_matrix
    from phenaki_pytorch_amd.train import pack_operand
    from phenaki_pytorch_amd.vgg import conv_matrix_bwd

    dev = torch.device('cuda:0')
    torch.cuda.set_device(0)
    Bf, Bb, R = args.frames, args.frames // 2, args.repeats
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say(f'# VGG16 perceptual network, 13 convolutions: {Bf} frames of {args.size} x {args.size} forward; {Bb} frames forward + input backward')
    say(f'# device: {torch.cuda.get_device_name(0)}; device-event times in ms, median of {R} repeats (spread = (max - min) / median), sides alternated per layer')
    say('# a = pk_conv3x3 (direct)   b = pk_im2col + pk_gemm (+ pk_col2im)   c = torch conv2d f32 (MIOpen, autograd)')
    total_flops_f = sum(conv_flops(Bf, H, C, Co) for _, H, C, Co in layers(args.size))
    total_flops_fb = 2 * sum(conv_flops(Bb, H, C, Co) for _, H, C, Co in layers(args.size))
    say(f'# shape arithmetic: fwd {total_flops_f / 1e12:.3f} TFLOP, fwd+bwd {total_flops_fb / 1e12:.3f} TFLOP ({total_flops_f / Bf / 1e9:.1f} GFLOP per frame forward)')
    totals = {}
    torch.manual_seed(0)
    for name in args.dtypes.split(','):
        dt = resolve_dtype(name)
        act = L.tdtype(dt)
        say()
        say(f'## {name}')
        say(f'{"layer":9} {"M(fwd)":>8} {"C":>4} {"Co":>4} | {"a fwd":>8} {"TF/s":>6} {"b fwd":>8} {"c fwd":>8} | {"a f+b":>8} {"TF/s":>6} {"b f+b":>8} {"c f+b":>8} | worst spread')
        tot = {k: 0. for k in ('af', 'bf', 'cf', 'afb', 'bfb', 'cfb')}
        spr = {k: 0. for k in tot}
        losers = []
        for lname, H, C, Co in layers(args.size):
            Cin = 3 if C == 8 else C
            w = torch.randn(Co, Cin, 3, 3, device=dev) * (2.0 / (9 * Cin)) ** 0.5
            bias = torch.randn(Co, device=dev) * 0.1
            Wf, Wb = pack_operand(_conv_matrix(w, C), dt), pack_operand(conv_matrix_bwd(w, C), dt)
            WbT = pack_operand(_conv_matrix(w, C), dt, transpose=True)          # (9 C, Co): dcols = dz W
            M16, M8 = Bf * H * H, Bb * H * H
            x16 = torch.randn(M16, C, device=dev)
            if C == 8:
                x16[:, 3:] = 0.
            xa16 = x16.to(act) if C != 8 else x16                              # a, bf16 mode: activations live in HBM as bf16 (the frame itself is f32)
            x8, xa8 = x16[:M8].contiguous(), xa16[:M8].contiguous()
            ya16, ya8 = torch.empty(M16, Co, device=dev, dtype=act), torch.empty(M8, Co, device=dev, dtype=act)
            yb16, yb8 = torch.empty(M16, Co, device=dev), torch.empty(M8, Co, device=dev)
            dy8 = torch.randn(M8, Co, device=dev)
            dxa, dxb, dz = torch.empty(M8, C, device=dev), torch.empty(M8, C, device=dev), torch.empty(M8, Co, device=dev)
            cols = torch.empty(M16, 9 * C, device=dev)
            xc16 = x16[:, :Cin].reshape(Bf, H, H, Cin).permute(0, 3, 1, 2).contiguous()
            xc8 = xc16[:Bb].clone().requires_grad_(True)
            dyc8 = dy8.reshape(Bb, H, H, Co).permute(0, 3, 1, 2).contiguous()

            def a_fwd():
                L.conv3x3(dt, xa16, Wf, Bf, H, H, C, Co, ya16, bias=bias, relu=True)

            def a_fb():
                L.conv3x3(dt, xa8, Wf, Bb, H, H, C, Co, ya8, bias=bias, relu=True)
                L.conv3x3(dt, dy8, Wb, Bb, H, H, Co, C, dxa, gate=ya8)

            def b_fwd():
                L.im2col(x16, Bf, H, H, C, 3, 3, 1, 1, cols)
                L.gemm(dt, cols, Wf, M16, Co, 9 * C, C=yb16, bias=bias, act=L.ACT_RELU)

            def b_fb():
                c8 = cols[:M8]
                L.im2col(x8, Bb, H, H, C, 3, 3, 1, 1, c8)
                L.gemm(dt, c8, Wf, M8, Co, 9 * C, C=yb8, bias=bias, act=L.ACT_RELU)
                L.leaky_bwd(yb8, dy8, dz, M8, Co, 0.)
                L.gemm(dt, dz, WbT, M8, 9 * C, Co, C=c8)
                L.col2im(c8, Bb, H, H, C, 3, 3, 1, 1, dxb)

            def c_fwd():
                with torch.no_grad():
                    F.relu(F.conv2d(xc16, w, bias, padding=1))

            def c_fb():
                y = F.relu(F.conv2d(xc8, w, bias, padding=1))
                torch.autograd.grad(y, xc8, dyc8)

            res = timed_alternating(dict(af=a_fwd, bf=b_fwd, cf=c_fwd, afb=a_fb, bfb=b_fb, cfb=c_fb), R)
            # the two implementations of this library agree on this layer (a bf16 reads bf16 rows: compare at the compute type's grain)
            a_fb(), b_fb()
            tol = 2e-2 if name == 'bf16' else 1e-3
            ey = float((ya8.float() - yb8).abs().max() / yb8.abs().max())
            ex = float((dxa - dxb).abs().max() / dxb.abs().max())
            assert ey <= tol and ex <= 10 * tol, f'{lname} {name}: a and b disagree (y {ey:.2e}, dx {ex:.2e})'
            for k in tot:
                tot[k] += med(res[k])
                spr[k] = max(spr[k], spread(res[k]))
            ff, ffb = conv_flops(Bf, H, C, Co), 2 * conv_flops(Bb, H, C, Co)
            say(f'{lname:9} {M16:8d} {C:4d} {Co:4d} | {med(res["af"]):8.3f} {ff / med(res["af"]) / 1e9:6.1f} {med(res["bf"]):8.3f} {med(res["cf"]):8.3f} | '
                f'{med(res["afb"]):8.3f} {ffb / med(res["afb"]) / 1e9:6.1f} {med(res["bfb"]):8.3f} {med(res["cfb"]):8.3f} | {max(spread(v) for v in res.values()):.1%}')
            if med(res['af']) > med(res['cf']) or med(res['afb']) > med(res['cfb']):
                losers.append(lname)
        say(f'{"13 layers":9} {"":8} {"":4} {"":4} | {tot["af"]:8.3f} {total_flops_f / tot["af"] / 1e9:6.1f} {tot["bf"]:8.3f} {tot["cf"]:8.3f} | '
            f'{tot["afb"]:8.3f} {total_flops_fb / tot["afb"] / 1e9:6.1f} {tot["bfb"]:8.3f} {tot["cfb"]:8.3f} | {max(spr.values()):.1%}')
        say(f'{name}: a / b = {tot["af"] / tot["bf"]:.3f} (fwd), {tot["afb"] / tot["bfb"]:.3f} (fwd+bwd);  a / c = {tot["af"] / tot["cf"]:.3f} (fwd), '
            f'{tot["afb"] / tot["cfb"]:.3f} (fwd+bwd)')
        say(f'{name}: layers where a is slower than c (either leg): {", ".join(losers) if losers else "none"}')
        totals[name] = tot

        # tile choice on the short, wide deep layers: 64 x 64 against 128 x 128 tiles (tile 0 = what pk_conv3x3 picks)
        say(f'{name}: tile choice, forward on {Bf} frames, ms (auto / 64x64 / 128x128):')
        for lname, H, C, Co in layers(args.size):
            if C < 256:
                continue
            x = torch.randn(Bf * H * H, C, device=dev).to(act)
            y = torch.empty(Bf * H * H, Co, device=dev, dtype=act)
            w = torch.randn(Co, C, 3, 3, device=dev) * (2.0 / (9 * C)) ** 0.5
            Wf = pack_operand(_conv_matrix(w, C), dt)
            tt = timed_alternating({tile: (lambda tile=tile: L.conv3x3(dt, x, Wf, Bf, H, H, C, Co, y, relu=True, tile=tile)) for tile in (0, 1, 3)}, R)
            t = [med(tt[tile]) for tile in (0, 1, 3)]
            say(f'    {lname:9} M = {Bf * H * H:6d}  {t[0]:8.3f} {t[1]:8.3f} {t[2]:8.3f}')

    # the whole module (pools, classifier included) against the same network of torch.nn layers in f32
    say()
    say('## whole network (13 convolutions, 5 max-pools, adaptive pool, 2 Linear), random weights')
    net = P.VGG16Features().to(dev).eval()
    ref = torch.nn.Sequential(net.features, net.avgpool, torch.nn.Flatten(1), net.classifier)
    img16 = torch.rand(Bf, 3, args.size, args.size, device=dev) * 2 - 1
    img8 = img16[:Bb].clone().requires_grad_(True)

    def whole(fn):
        def fwd():
            with torch.no_grad():
                fn(img16)

        def fb():
            torch.autograd.grad(fn(img8).square().sum(), img8)
        return med(timed(fwd, R)), med(timed(fb, R))

    cf, cfb = whole(ref)
    say(f'torch.nn f32      : fwd {cf:8.3f} ms   fwd+bwd {cfb:8.3f} ms')
    for name in args.dtypes.split(','):
        P.set_compute_dtype(net, name)
        af, afb = whole(net)
        say(f'VGG16Features {name:6}: fwd {af:8.3f} ms   fwd+bwd {afb:8.3f} ms   (x{cf / af:.2f}, x{cfb / afb:.2f} against torch.nn f32)')

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    bad = [n for n, t in totals.items() if n != 'fp32' and not (t['af'] < t['bf'] and t['afb'] < t['bfb'])]
    if bad:
        raise SystemExit(f'acceptance: the direct convolution does not beat im2col + GEMM in {bad}')


if __name__ == '__main__':
    main()
