"""The tail of a training step on the MI355X kernels (csrc/step_tail.hip): what the reference's trainers do between `loss.backward()` and the
next forward besides the optimizer.

`clip_grad_norm_` -- `accelerator.clip_grad_norm_(params, max_grad_norm)` of cvivit_trainer.py:245-246, 268-269 and phenaki_trainer.py:380-381, i.e.
torch.nn.utils.clip_grad_norm_ with norm_type 2: one norm pass over every gradient, the coefficient computed on the device, one in-place scale.
(`HipAdamW(max_grad_norm=...)` folds the scale into the update instead and leaves `.grad` alone.)

`EMA` -- the `EMA(vae, update_after_step=..., update_every=...)` of cvivit_trainer.py:93, 282, 293, 338.  Its schedule is restated from memory of the
published `ema_pytorch` package, which is not installable on this stack: PARITY WITH UPSTREAM IS UNPINNED, as it is for the quantizers.  The averaged
weights are written by pk_ema_multi and every written tensor's version is bumped, so the packed-weight caches and captured graphs of `ema_model`
follow them (a plain-torch EMA writing through `.data` would leave them stale: dropin.py)."""
import copy

import torch
from torch import nn

from . import _lib as L


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """scales every `.grad` in place by min(max_norm / (total_norm + 1e-6), 1) and returns total_norm, the L2 norm over all gradients, as a 0-dim f32
    device tensor -- nothing here synchronises.  Runs on the current stream (after GradientReducer.finish() it sees the reduced gradients).
    Non-finite norms behave as torch's default error_if_nonfinite=False: the coefficient is what the formula gives."""
    if float(norm_type) != 2.0:
        raise ValueError(f'clip_grad_norm_: only norm_type = 2 is built (got {norm_type})')
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    for p in params:
        L.require_device(p.grad, 'gradient')
    grads = []
    for i, p in enumerate(params):
        g = p.grad
        if g.dtype != torch.float32 or not g.is_contiguous():
            raise RuntimeError(f'clip_grad_norm_: the gradient of parameter {i} {tuple(p.shape)} is {g.dtype} '
                               f'{"contiguous" if g.is_contiguous() else "strided"}: the in-place scale needs contiguous float32 (it cannot work on a copy)')
        if g.numel() > 0:
            grads.append(g)
    if not grads:
        return torch.zeros((), dtype=torch.float32, device=params[0].grad.device if params else 'cpu')
    devices = {g.device for g in grads}
    if len(devices) > 1:
        raise RuntimeError(f'clip_grad_norm_: the gradients span more than one device ({sorted(map(str, devices))})')
    device = grads[0].device
    table, out = L.grad_norm_coef(grads, max_norm, device)
    L.scale_multi(table, out[1:], device)
    for g in grads:
        torch.autograd.graph.increment_version(g)
    return out[0]


def ema_decision(step, initted, update_after_step, update_every):
    """what update() does at host step counter `step` (before its increment): 'skip', 'copy' (online -> ema) or 'lerp'"""
    if step % update_every != 0:
        return 'skip'
    if step <= update_after_step or not initted:
        return 'copy'
    return 'lerp'


class EMA(nn.Module):
    """exponential moving average of `model`'s floating-point parameters and buffers (the VectorQuantize codebook statistics included); other
    buffers are copied.  `ema_model` is a deep copy with requires_grad off; the online model is held unregistered; forward delegates to ema_model.

    update(), restated from memory of the published ema_pytorch (upstream parity unpinned):
      1. s = step; step += 1                      2. s % update_every != 0: return
      3. s <= update_after_step: copy online into ema, return
      4. not initted: copy, set initted           5. else d = current_decay(); ema += (1 - d) (online - ema)
    current_decay(): epoch = max(step - update_after_step - 1, 0); 0 if epoch <= 0, else clamp(1 - (1 + epoch / inv_gamma) ** -power, min_value, beta).
    `step` and `initted` are host integers saved through get_extra_state / set_extra_state: update() never synchronises and a state_dict()
    round trip resumes the schedule."""

    def __init__(self, model, beta=0.9999, update_after_step=100, update_every=10, inv_gamma=1.0, power=2 / 3, min_value=0.0):
        super().__init__()
        self.beta, self.update_after_step, self.update_every = beta, update_after_step, update_every
        self.inv_gamma, self.power, self.min_value = inv_gamma, power, min_value
        self._online = [model]                               # a list keeps the online model out of _modules / state_dict
        self.ema_model = copy.deepcopy(model)
        self.ema_model.requires_grad_(False)
        self.step, self.initted = 0, False

    @property
    def online_model(self):
        return self._online[0]

    def get_extra_state(self):
        return dict(step=int(self.step), initted=bool(self.initted))

    def set_extra_state(self, state):
        self.step, self.initted = int(state['step']), bool(state['initted'])

    def current_decay(self):
        epoch = max(self.step - self.update_after_step - 1, 0)
        if epoch <= 0:
            return 0.
        value = 1 - (1 + epoch / self.inv_gamma) ** -self.power
        return min(max(value, self.min_value), self.beta)

    def next_decision(self):
        """what the next update() call will do: 'skip', 'copy' or 'lerp' (host only)"""
        return ema_decision(self.step, self.initted, self.update_after_step, self.update_every)

    def _pairs(self):
        ema_p, src_p = dict(self.ema_model.named_parameters()), dict(self.online_model.named_parameters())
        ema_b, src_b = dict(self.ema_model.named_buffers()), dict(self.online_model.named_buffers())
        for name, e in list(ema_p.items()) + list(ema_b.items()):
            yield name, e, (src_p[name] if name in ema_p else src_b[name])

    @torch.no_grad()
    def _write(self, weight):
        """ema += weight (online - ema) through pk_ema_multi (weight = 1: the exact copy); non-floating buffers are copied.  Everything is checked
        before anything is written."""
        by_device, copies = {}, []
        for name, e, x in self._pairs():
            L.require_device(x, name)
            L.require_device(e, 'ema_model.' + name)
            if e.shape != x.shape or e.device != x.device:
                raise RuntimeError(f'EMA: {name} is {tuple(x.shape)} on {x.device} online but {tuple(e.shape)} on {e.device} in ema_model')
            if not e.is_floating_point():
                copies.append((e, x))
                continue
            for t, what in ((e, 'ema_model.' + name), (x, name)):
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise RuntimeError(f'EMA: {what} is {t.dtype} {"contiguous" if t.is_contiguous() else "strided"}: the kernel averages contiguous '
                                       'float32 tensors (keep the modules in float32)')
            if e.numel() > 0:
                by_device.setdefault(e.device, []).append((e, x))
        for e, x in copies:
            e.copy_(x)
        for device, group in by_device.items():
            L.ema_multi(group, weight, device)
            for e, _ in group:
                torch.autograd.graph.increment_version(e)   # raw-pointer writes: packed-weight caches / captured graphs key on _version

    def copy_params_from_model_to_ema(self):
        self._write(1.0)

    def advance(self):
        """the host half of update(): moves `step` / `initted` on and returns what this call does -- 'skip', 'copy' or 'lerp'"""
        decision = self.next_decision()
        if decision == 'copy' and self.step > self.update_after_step:
            self.initted = True
        self.step += 1
        return decision

    def update(self):
        decision = self.advance()
        if decision != 'skip':
            self._write(1.0 if decision == 'copy' else 1.0 - self.current_decay())

    def forward(self, *args, **kwargs):
        return self.ema_model(*args, **kwargs)
