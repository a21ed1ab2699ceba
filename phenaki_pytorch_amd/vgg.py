"""The perceptual network of the tokenizer's GAN objective on the MI355X kernels: reference phenaki_pytorch/cvivit.py:349-352
(`torchvision.models.vgg16(pretrained=True)` with `classifier = classifier[:-2]`) and its use at :636-651
(`perceptual_loss = F.mse_loss(vgg(frame), vgg(recon frame))`, differentiated with respect to the reconstructed frame).

`VGG16Features` has torchvision's module tree and state_dict keys (`features.{0,2,5,...,28}.{weight,bias}` in OIHW, `classifier.{0,3}.{weight,bias}`):
a torchvision VGG16 checkpoint loads unchanged (`classifier.6.*`, the layer the reference cuts, is dropped).  The nn.Conv2d / nn.Linear objects are
parameter containers; the arithmetic is

    image (B, 3, H, W)    --pk_nchw_to_rows-->  channels-last pixel rows x[(b, y, x)][c], C padded to 8
    Conv2d 3x3 + ReLU     =  pk_conv3x3 (direct convolution, ReLU in the epilogue; csrc/vgg.hip)
    MaxPool2d(2, 2)       =  pk_maxpool2x2
    AdaptiveAvgPool2d(7)  =  pk_adaptive_avgpool, rows (b, i, j) -> the (B, 49 C) matrix in (h, w, c) order; classifier.0 is packed with its columns
                             permuted from torchvision's (c, h, w) flatten order
    Linear + ReLU         =  pk_gemm (act 3);  Dropout(0.5) between them (training mode only) = pk_dropout_mask + pk_mul

The whole network is ONE autograd.Function (first order).  Its backward computes the INPUT gradient only -- the parameters are created with
requires_grad = False and no weight gradient exists (the reference's trainer hands the VGG's parameters to the tokenizer's optimizer by
accident) -- with the ReLU backward fused into the backward-data convolution (pk_conv3x3's gate operand).  Nothing is saved when the input does not require
a gradient (the real-frame branch of the perceptual loss).
"""
import torch
from torch import nn

from . import _lib as L
from .attention import PackedModule, _cache, compute_dtype_of
from .discriminator import CPAD, _conv_matrix
from .train import _f32, pack_operand

VGG16_LAYOUT = (2, 2, 3, 3, 3)      # convolutions per block; every block ends in a 2x2 max-pool
POOLED = 7                          # nn.AdaptiveAvgPool2d((7, 7))


def conv_matrix_bwd(w, Cp):
    """nn.Conv2d weight (O, Cin, 3, 3) -> the weight matrix (Cp, 9 O) of the backward-data convolution in im2col column order:
    Wb[c][((2 - ky) * 3 + (2 - kx)) * O + o] = W[o][c][ky][kx] (the transposed, spatially flipped filter); rows Cin..Cp-1 (padding channels) are zero"""
    O, Cin, kh, kw = w.shape
    m = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, kh * kw * O)
    if Cp != Cin:
        m = torch.cat((m, m.new_zeros(Cp - Cin, kh * kw * O)))
    return m.contiguous()


def classifier0_matrix(w, C, S=POOLED):
    """classifier.0.weight (hidden, C S S) over torchvision's flatten order (c, h, w) -> columns in the (h, w, c) order of the pooled pixel rows"""
    return w.reshape(w.shape[0], C, S, S).permute(0, 2, 3, 1).reshape(w.shape[0], S * S * C).contiguous()


def adaptive_windows(s, out=POOLED):
    """[(start, end)] of nn.AdaptiveAvgPool2d along an axis of length s: [floor(i s / out), ceil((i + 1) s / out))"""
    return [((i * s) // out, -((-(i + 1) * s) // out)) for i in range(out)]


class _VGGFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, net, need_grad):
        dt = compute_dtype_of(net)
        act = L.tdtype(dt)                   # bf16 mode: the activations live in HBM as bf16
        dev = img.device
        B, Cimg, H, W = img.shape
        x = L.nchw_to_rows(img.detach().float().contiguous(), CPAD, _f32((B * H * W, CPAD), dev))
        C = CPAD
        saved, plan = [], []                 # saved: post-ReLU outputs (the gates, and the pools' inputs); plan: the layer sequence for the backward
        for layer in net.features:
            if isinstance(layer, nn.Conv2d):
                Wimg, _ = net._conv_images(layer, C, dt)
                y = torch.empty((B * H * W, layer.out_channels), device=dev, dtype=act)
                L.conv3x3(dt, x, Wimg, B, H, W, C, layer.out_channels, y, bias=layer.bias, relu=True)
                plan.append(('conv', layer, H, W, C, len(saved)))
                saved.append(y if need_grad else None)
                x, C = y, layer.out_channels
            elif isinstance(layer, nn.MaxPool2d):
                assert H >= 2 and W >= 2, 'the image is too small for the five 2x2 max-pools of VGG16 (32 x 32 at least)'
                y = torch.empty((B * (H // 2) * (W // 2), C), device=dev, dtype=act)
                L.maxpool2x2(x, B, H, W, C, y)
                plan.append(('pool', None, H, W, C, len(saved) - 1))
                x, H, W = y, H // 2, W // 2
        pooled = L.adaptive_avgpool(x, B, H, W, C, _f32((B, POOLED * POOLED * C), dev))
        lin0, lin3 = net.classifier[0], net.classifier[3]
        assert lin0.in_features == POOLED * POOLED * C
        hidden = lin0.out_features
        W0, _ = net._linear_images('c0', lin0, dt, C)
        W3, _ = net._linear_images('c3', lin3, dt, None)
        h1 = L.gemm(dt, pooled, W0, B, hidden, lin0.in_features, C=_f32((B, hidden), dev), bias=lin0.bias, act=L.ACT_RELU)
        keep = None
        site = L.DropSite.of(net.classifier[2], dev)
        h1d = h1
        if site is not None:
            keep = L.dropout_mask(site.seed, site.offset, B, hidden, site.p, dev).to(torch.float32).mul_(site.scale)
            h1d = L.mul(h1, keep, torch.empty_like(h1))
        out = L.gemm(dt, h1d, W3, B, lin3.out_features, hidden, C=_f32((B, lin3.out_features), dev), bias=lin3.bias, act=L.ACT_RELU)
        ctx.net, ctx.dt, ctx.plan, ctx.geom, ctx.has_keep = net, dt, plan, (B, Cimg, H, W, C), keep is not None
        if need_grad:
            tensors = [t for t in saved] + [h1, out] + ([keep] if keep is not None else [])
            ctx.save_for_backward(*tensors)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        net, dt, plan = ctx.net, ctx.dt, ctx.plan
        B, Cimg, H5, W5, C5 = ctx.geom
        tensors = ctx.saved_tensors
        if not tensors:
            raise RuntimeError('VGG16Features: backward through a forward pass whose input did not require a gradient')
        keep = tensors[-1] if ctx.has_keep else None
        h1, out = tensors[-3:-1] if ctx.has_keep else tensors[-2:]
        saved = tensors[:len(tensors) - (3 if ctx.has_keep else 2)]
        dev = dout.device
        lin0, lin3 = net.classifier[0], net.classifier[3]
        hidden = lin0.out_features
        _, W0t = net._linear_images('c0', lin0, dt, C5)
        _, W3t = net._linear_images('c3', lin3, dt, None)
        dout = dout.contiguous().float()
        g = _f32(tuple(out.shape), dev)
        L.leaky_bwd(out, dout, g, B, out.shape[1], 0.)                                   # ReLU backward from the output
        dh = L.gemm(dt, g, W3t, B, hidden, lin3.out_features, C=_f32((B, hidden), dev))  # g W3
        if keep is not None:
            L.mul(dh, keep, dh)
        L.leaky_bwd(h1, dh, dh, B, hidden, 0.)
        d = L.gemm(dt, dh, W0t, B, lin0.in_features, hidden, C=_f32((B, lin0.in_features), dev))
        d = L.adaptive_avgpool_bwd(d, B, H5, W5, C5, _f32((B * H5 * W5, C5), dev))
        for kind, layer, H, W, C, idx in reversed(plan):
            if kind == 'pool':
                d = L.maxpool2x2_bwd(saved[idx], d, B, H, W, C, _f32((B * H * W, C), dev))
            else:
                _, Wb = net._conv_images(layer, C, dt)
                dx = _f32((B * H * W, C), dev)
                d = L.conv3x3(dt, d, Wb, B, H, W, layer.out_channels, C, dx, gate=saved[idx])
        H, W = plan[0][2], plan[0][3]
        dimg = L.rows_to_nchw(d, CPAD, _f32((B, Cimg, H, W), dev))
        return dimg, None, None


class VGG16Features(PackedModule):
    """torchvision's VGG16 with `classifier[:-2]` (cvivit.py:349-352): forward((B, 3, H, W) f32) -> (B, hidden), the post-ReLU output of classifier.3.
    `widths` / `hidden` shrink the network for tests; the defaults are VGG16.  Parameters are frozen (requires_grad = False): the network is a fixed
    feature extractor, only the input gradient is computed.  Follows `set_compute_dtype`.  Load pretrained weights with `.load(path)` or
    `load_state_dict` (a torchvision `vgg16` state dict) -- a randomly initialised perceptual network is only good for tests."""

    def __init__(self, widths=(64, 128, 256, 512, 512), hidden=4096, channels=3):
        super().__init__()
        assert len(widths) == len(VGG16_LAYOUT) and all(w % 8 == 0 for w in widths), 'five block widths, each a multiple of 8'
        assert hidden % 8 == 0 and 0 < channels <= CPAD
        layers, cin = [], channels
        for width, n in zip(widths, VGG16_LAYOUT):
            for _ in range(n):
                layers += [nn.Conv2d(cin, width, 3, padding=1), nn.ReLU(inplace=True)]
                cin = width
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d((POOLED, POOLED))
        self.classifier = nn.Sequential(nn.Linear(cin * POOLED * POOLED, hidden), nn.ReLU(True), nn.Dropout(0.5), nn.Linear(hidden, hidden), nn.ReLU(True))
        self.channels = channels
        for p in self.parameters():
            p.requires_grad_(False)

    def load_state_dict(self, state_dict, *args, **kwargs):
        """accepts a full torchvision VGG16 checkpoint: `classifier.6.*` (the 1000-way layer the reference cuts) is dropped"""
        sd = {k: v for k, v in state_dict.items() if not k.startswith('classifier.6.')}
        return super().load_state_dict(sd, *args, **kwargs)

    def load(self, path, map_location='cpu'):
        self.load_state_dict(torch.load(path, map_location=map_location))
        return self

    # packed device images, built lazily and dropped by load_state_dict / .to() (PackedModule)
    def _conv_images(self, conv, Cp, dt):
        """(forward weight image (O, 9 Cp), backward-data weight image (Cp, 9 O)) of a convolution in compute dtype dt"""
        def build():
            w = conv.weight.detach().float()
            return pack_operand(_conv_matrix(w, Cp), dt), pack_operand(conv_matrix_bwd(w, Cp), dt)
        return _cache(self).get(('conv', id(conv), Cp, dt), (conv.weight,), build)

    def _linear_images(self, key, lin, dt, C):
        """(image of W for x W^T, image of W^T for g W); C: channel count of the pooled rows when the columns need the (c, h, w) -> (h, w, c) permutation"""
        def build():
            w = lin.weight.detach().float()
            if C is not None:
                w = classifier0_matrix(w, C)
            return pack_operand(w.contiguous(), dt), pack_operand(w.contiguous(), dt, transpose=True)
        return _cache(self).get((key, dt), (lin.weight,), build)

    def forward(self, img):
        L.require_device(img, 'images')
        assert img.ndim == 4 and img.shape[1] == self.channels, f'expected (B, {self.channels}, H, W) images, got {tuple(img.shape)}'
        need_grad = torch.is_grad_enabled() and img.requires_grad
        return _VGGFn.apply(img, self, need_grad)
