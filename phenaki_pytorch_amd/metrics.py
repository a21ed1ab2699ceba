"""Validation metrics of the tokenizer on the MI355X kernels (csrc/metrics.hip): per-frame MSE / PSNR / SSIM of two videos, the usage statistics
of a batch of code ids, and `TokenizerMetrics`, the accumulator over held-out batches.

The reference's CViViTTrainer runs its EMA tokenizer on held-out clips every `save_results_every` steps and dumps image grids
(cvivit_trainer.py:284-323); it computes no number.  `CViViT.evaluate` is that pass with numbers: it costs about one extra read of the two
videos and nothing here synchronises with the host until `TokenizerMetrics.compute()`.

Always f32, whatever `set_compute_dtype` says: a validation number must not move with the compute mode of the model it validates (the rule LFQ
follows for its ids).  Inputs are (B, C, F, H, W) videos, or (B, C, H, W) image batches counted as one frame each; results are per frame, (B, F).
`clamp`: None / False = off, a number = the FIRST operand is read clamped to [0, clamp] inside the kernel (no clamped copy is written), True = the
data range.
"""
import torch

from . import _lib as L


def _pair(a, b, what, min_hw=1):
    """checks before anything is launched -> the two videos as contiguous (B, C, F, H, W)"""
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
        raise ValueError(f'{what}: two tensors are expected')
    if a.shape != b.shape:
        raise ValueError(f'{what}: shapes differ, {tuple(a.shape)} vs {tuple(b.shape)}')
    if a.ndim not in (4, 5):
        raise ValueError(f'{what}: (B, C, F, H, W) videos or (B, C, H, W) images are expected, got {tuple(a.shape)}')
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f'{what}: the metrics are float32 whatever the compute dtype of the model, got {a.dtype} and {b.dtype} (convert the inputs)')
    if a.numel() == 0:
        raise ValueError(f'{what}: empty input {tuple(a.shape)}')
    if a.shape[-2] < min_hw or a.shape[-1] < min_hw:
        raise ValueError(f'{what}: frames of {a.shape[-2]} x {a.shape[-1]} pixels are smaller than the {min_hw} x {min_hw} window')
    L.require_device(a, what + ' (first operand)')
    L.require_device(b, what + ' (second operand)')
    if a.device != b.device:
        raise ValueError(f'{what}: operands on {a.device} and {b.device}')
    if a.ndim == 4:
        a, b = a.unsqueeze(2), b.unsqueeze(2)
    return a.contiguous(), b.contiguous()


def _clamp_hi(clamp, data_range, what):
    if clamp is None or clamp is False:
        return 0.
    hi = float(data_range) if clamp is True else float(clamp)
    if not hi > 0.:
        raise ValueError(f'{what}: clamp must be a positive upper bound, got {clamp}')
    return hi


def _range(data_range, what):
    r = float(data_range)
    if not (r > 0. and r < float('inf')):
        raise ValueError(f'{what}: data_range must be positive and finite, got {data_range}')
    return r


def frame_mse(a, b, clamp=None):
    """mean of (a - b)^2 over the C H W pixels of every frame -> (B, F) f32 on the device"""
    hi = _clamp_hi(clamp, 1., 'frame_mse')
    a, b = _pair(a, b, 'frame_mse')
    return L.frame_sqerr(a, b, hi)


def _mse_psnr(a, b, data_range=1., clamp=None):
    """(frame_mse, psnr) in one pass over the videos"""
    r = _range(data_range, 'psnr')
    hi = _clamp_hi(clamp, r, 'psnr')
    a, b = _pair(a, b, 'psnr')
    return L.frame_sqerr(a, b, hi, r)


def psnr(a, b, data_range=1., clamp=None):
    """10 log10(R^2 / max(mse, 1e-10 R^2)) per frame -> (B, F) f32: identical frames give 100 dB, so means stay finite"""
    return _mse_psnr(a, b, data_range, clamp)[1]


def ssim(a, b, data_range=1., clamp=None):
    """SSIM of Wang et al. per frame, as pytorch-msssim / torchmetrics compute it: 11 x 11 Gaussian window with sigma 1.5, 'valid' positions,
    biased moments, C1 = (0.01 R)^2, C2 = (0.03 R)^2; the map averaged over the positions of a plane and the C planes of the frame -> (B, F) f32"""
    r = _range(data_range, 'ssim')
    hi = _clamp_hi(clamp, r, 'ssim')
    a, b = _pair(a, b, 'ssim', min_hw=11)
    return L.frame_ssim(a, b, r, hi)


def _usage_of_counts(counts32, codebook_size):
    u = L.code_usage(counts32)
    return dict(counts=counts32.long(), used=u[1].long(), usage=(u[1] / codebook_size).float(), entropy=u[2].float(), perplexity=u[3].float(),
                max_share=u[4].float())


def codebook_usage(ids, codebook_size, keep=None):
    """how a batch of code ids uses the codebook: dict of device tensors -- counts (V,) int64, used (codes with a count), usage = used / V,
    entropy = -sum p ln p over p > 0 (nats), perplexity = exp(entropy), max_share = max p.  keep: optional bool mask of the shape of `ids`; the
    ids it drops are not counted.  No id: used 0, entropy 0, perplexity 1, max_share 0.  An id outside [0, V) is not counted."""
    V = int(codebook_size)
    if V <= 0:
        raise ValueError(f'codebook_usage: codebook_size must be positive, got {codebook_size}')
    if not isinstance(ids, torch.Tensor) or ids.dtype not in (torch.int64, torch.int32) or ids.numel() == 0:
        raise ValueError('codebook_usage: ids must be a non-empty int64 (or int32) tensor')
    if ids.numel() >= 2 ** 31:
        raise ValueError(f'codebook_usage: {ids.numel()} ids in one call; the histogram kernel counts below 2^31')
    if keep is not None and keep.numel() != ids.numel():
        raise ValueError(f'codebook_usage: keep has {keep.numel()} entries for {ids.numel()} ids')
    L.require_device(ids, 'ids')
    flat = ids.reshape(-1).long().contiguous()
    k = None
    if keep is not None:
        L.require_device(keep, 'keep')
        k = keep.reshape(-1).to(torch.uint8).contiguous()
    return _usage_of_counts(L.code_hist(flat, k, V), V)


def _masked_mean(x, mask):
    """mean of the per-frame values `mask` (B, F) keeps (None: all), accumulated in float64 -> 0-dim f32; no frame kept: nan"""
    if mask is None:
        return x.double().mean().float()
    m = mask.to(torch.float64)
    return ((x.double() * m).sum() / m.sum()).float()


# ---- accumulator ---------------------------------------------------------------------------------------------------------------

STATE_KEYS = ('counts', 'frames', 'mse', 'psnr', 'ssim')


def merge_states(state, group=None):
    """sums a TokenizerMetrics state over the ranks of an initialised process group (world size > 1), in place, key by key in sorted order;
    otherwise returns it untouched.  A plain dict of tensors in, the same dict out: works on CPU tensors under gloo as on device tensors under RCCL."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
        return state
    for key in sorted(state):
        dist.all_reduce(state[key], op=dist.ReduceOp.SUM, group=group)
    return state


class TokenizerMetrics:
    """running validation statistics of a C-ViViT tokenizer over held-out batches.

        tm = TokenizerMetrics(ema.ema_model)
        for clip in held_out: tm.update(clip)         # device-side sums only, no host synchronisation
        numbers = tm.compute()                        # one synchronisation: plain Python floats

    state (device tensors): float64 sums of the per-frame mse / psnr / ssim over the kept frames, the int64 frame count and the int64 histogram of
    the code ids of the kept frames' tokens.  compute() first sums the state over the ranks of an initialised process group (merge_states), then
    derives the means and -- from the summed histogram, not from per-batch figures -- the codebook usage.

    With a process group of more than one rank compute() is a COLLECTIVE: every rank of the group has to call it (after its own update() calls), and
    every rank gets the same numbers.  A rank that validates on its own while the others go on -- rank 0 holding the only EMA copy, say -- calls
    compute(merge=False): nothing is sent, the numbers are that rank's alone."""

    def __init__(self, cvivit, data_range=1., clamp=True):
        self.cvivit, self.data_range, self.clamp = cvivit, data_range, clamp
        self.state = None

    def reset(self):
        self.state = None

    @torch.no_grad()
    def update(self, video, mask=None):
        r = self.cvivit.evaluate(video, mask=mask, data_range=self.data_range, clamp=self.clamp)
        m = torch.ones_like(r['mse'], dtype=torch.float64) if mask is None else mask.to(torch.float64)
        step = dict(mse=(r['mse'].double() * m).sum(), psnr=(r['psnr'].double() * m).sum(), ssim=(r['ssim'].double() * m).sum(),
                    frames=r['frames'].long(), counts=r['codebook_usage']['counts'])
        if self.state is None:
            self.state = step
        else:
            for k in STATE_KEYS:
                self.state[k] = self.state[k] + step[k]
        return self

    @torch.no_grad()
    def compute(self, group=None, merge=True):
        if self.state is None:
            raise RuntimeError('TokenizerMetrics.compute() before any update()')
        s = {k: v.clone() for k, v in self.state.items()}
        if merge:
            s = merge_states(s, group)
        V = s['counts'].numel()
        # the histogram kernel's counts are int32: a run of more than 2^31 - 1 tokens saturates here (usage and perplexity stay meaningful)
        u = L.code_usage(s['counts'].clamp(max=2 ** 31 - 1).to(torch.int32))
        frames = s['frames'].double()
        packed = torch.stack((s['mse'] / frames, s['psnr'] / frames, s['ssim'] / frames, frames, u[0], u[1], u[2], u[3], u[4])).tolist()
        mse, psnr_, ssim_, frames, tokens, used, entropy, perplexity, max_share = packed
        return dict(mse=mse, psnr=psnr_, ssim=ssim_, frames=int(frames), tokens=int(tokens), codes_used=int(used), codebook_size=V, usage=used / V,
                    entropy=entropy, perplexity=perplexity, max_share=max_share)
