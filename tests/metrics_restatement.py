"""The validation metrics of phenaki_pytorch_amd/metrics.py restated in plain torch, float64 by default, written from the published definitions
and not from the kernels' structure: the SSIM window is the 2-D outer product applied by ONE conv2d (no separable passes, no tiles), the usage
numbers come from torch.bincount.  `dtype=torch.float32` runs the same formulas in f32: that run is the yardstick the kernels' tolerances are
derived from (tests/test_metrics_host.py keeps it measured).  `shift=True` subtracts one constant per plane (the plane's mean of `a`) from both
videos before the moments are accumulated -- a no-op for variances and covariance in exact arithmetic -- and adds it back for the luminance term;
`shift=False` is the textbook E[a^2] - E[a]^2 on the raw pixels."""
import math

import torch
import torch.nn.functional as F


def gaussian_window(size=11, sigma=1.5, dtype=torch.float64):
    x = torch.arange(size, dtype=torch.float64) - (size - 1) / 2
    g = torch.exp(-(x * x) / (2 * sigma * sigma))
    g = g / g.sum()
    return torch.outer(g, g).to(dtype)


def _five(a, b):
    """(B, C, F, H, W) or (B, C, H, W) -> both as (B, C, F, H, W)"""
    if a.ndim == 4:
        a, b = a.unsqueeze(2), b.unsqueeze(2)
    return a, b


def _clamped(a, clamp):
    return a if clamp is None else a.clamp(0., float(clamp))


def frame_mse(a, b, clamp=None, dtype=torch.float64):
    a, b = _five(a, b)
    a, b = _clamped(a.to(dtype), clamp), b.to(dtype)
    return ((a - b) ** 2).mean(dim=(1, 3, 4))


def psnr(a, b, data_range=1., clamp=None, dtype=torch.float64):
    r2 = float(data_range) ** 2
    return 10. * torch.log10(r2 / frame_mse(a, b, clamp, dtype).clamp(min=1e-10 * r2))


def ssim(a, b, data_range=1., clamp=None, dtype=torch.float64, shift=True):
    a, b = _five(a, b)
    a, b = _clamped(a.to(dtype), clamp), b.to(dtype)
    B, C, Fr, H, W = a.shape
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    x, y = a.permute(0, 2, 1, 3, 4).reshape(B * Fr * C, 1, H, W), b.permute(0, 2, 1, 3, 4).reshape(B * Fr * C, 1, H, W)
    s = x.mean(dim=(2, 3), keepdim=True) if shift else torch.zeros_like(x[:, :, :1, :1])
    x, y = x - s, y - s
    win = gaussian_window(dtype=dtype)[None, None]
    maps = F.conv2d(torch.cat((x, y, x * x, y * y, x * y), dim=1), win.expand(5, 1, 11, 11).contiguous(), groups=5)
    m1, m2, e11, e22, e12 = maps.unbind(dim=1)
    v1, v2, cov = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
    s = s[:, 0]
    mu1, mu2 = m1 + s, m2 + s
    smap = ((2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1)) * ((2 * cov + c2) / (v1 + v2 + c2))
    return smap.mean(dim=(1, 2)).view(B, Fr, C).mean(dim=2)


# ---- the case list shared by the host yardstick and the GPU parity tests -------------------------------------------------------------------------

SHAPES = [(11, 11),       # a single window
          (16, 12),
          (37, 45),       # ragged tiles, rows that do not start on 16 bytes
          (64, 64),       # 2 x 2 tiles of 32 x 32 window positions
          (75, 140)]      # more tiles than one row of them
CONTENTS = ['noise', 'smooth', 'flat', 'same', 'outside', 'outside_clamped', 'range255']


def make_case(content, H, W, B=2, C=3, Fr=3, seed=0):
    """(a, b, kwargs): two seeded f32 CPU videos (B, C, Fr, H, W) (Fr = None: a 4-D image batch) and the data_range / clamp keywords of the case"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W)
    shape = (B, C, H, W) if Fr is None else (B, C, Fr, H, W)
    rand = lambda: torch.rand(shape, generator=g)
    randn = lambda: torch.randn(shape, generator=g)
    kw = {}
    if content == 'noise':
        a = rand()
        b = a + 0.1 * randn()
    elif content == 'smooth':
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
        phase = 6.28 * torch.rand(shape[:-2], generator=g)[..., None, None]
        a = 0.5 + 0.4 * torch.sin(0.21 * yy + 0.13 * xx + phase)
        b = a + 0.02 * randn()
    elif content == 'flat':
        a = torch.full(shape, 0.9)
        b = 0.9 + 0.003 * randn()
    elif content == 'same':
        a = rand()
        b = a.clone()
    elif content in ('outside', 'outside_clamped'):
        a = 1.6 * rand() - 0.3
        b = rand()
        if content == 'outside_clamped':
            kw = dict(clamp=1.0)
    elif content == 'range255':
        a = 255. * rand()
        b = a + 25.5 * randn()
        kw = dict(data_range=255.)
    else:
        raise KeyError(content)
    return a.float().contiguous(), b.float().contiguous(), kw


def codebook_usage(ids, codebook_size, keep=None):
    ids = ids.reshape(-1).long().cpu()
    if keep is not None:
        ids = ids[keep.reshape(-1).bool().cpu()]
    counts = torch.bincount(ids, minlength=codebook_size)
    total = int(counts.sum())
    used = int((counts > 0).sum())
    if total == 0:
        return dict(counts=counts, used=0, usage=0., entropy=0., perplexity=1., max_share=0.)
    p = counts[counts > 0].double() / total
    entropy = float(-(p * p.log()).sum())
    return dict(counts=counts, used=used, usage=used / codebook_size, entropy=entropy, perplexity=math.exp(entropy), max_share=float(p.max()))
