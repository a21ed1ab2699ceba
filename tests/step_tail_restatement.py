"""Plain-torch restatements the step-tail tests compare against (tests/test_step_tail_gpu.py, tests/test_step_tail_host.py).

The EMA schedule is restated from memory of the published `ema_pytorch` package (the trainers' `EMA(vae, update_after_step=..., update_every=...)`,
cvivit_trainer.py:93, 282): that package is not importable here, so PARITY WITH UPSTREAM IS UNPINNED -- these functions pin the product to the
semantics the project documents, written independently of phenaki_pytorch_amd/step_tail.py (one flat function per rule, float64 arithmetic)."""
import torch


def decay_closed_form(step, update_after_step, inv_gamma=1.0, power=2 / 3, min_value=0.0, beta=0.9999):
    """the decay an update uses when the host counter reads `step` (already incremented by that update)"""
    epoch = step - update_after_step - 1
    if epoch <= 0:
        return 0.0
    value = 1.0 - (1.0 + epoch / inv_gamma) ** (-power)
    return min(max(value, min_value), beta)


def cadence(calls, update_after_step, update_every):
    """the decisions of `calls` consecutive update() calls from a fresh EMA: 'copy' / 'skip' / 'lerp'"""
    out, initted = [], False
    for s in range(calls):
        if s % update_every != 0:
            out.append('skip')
        elif s <= update_after_step:
            out.append('copy')
        elif not initted:
            initted = True
            out.append('copy')
        else:
            out.append('lerp')
    return out


class EmaRestatement:
    """tensors by name on the CPU; update(online) takes the online tensors by the same names"""

    def __init__(self, online, beta=0.9999, update_after_step=100, update_every=10, inv_gamma=1.0, power=2 / 3, min_value=0.0):
        self.cfg = dict(update_after_step=update_after_step, inv_gamma=inv_gamma, power=power, min_value=min_value, beta=beta)
        self.update_after_step, self.update_every = update_after_step, update_every
        self.step, self.initted = 0, False
        self.ema = {k: v.detach().cpu().clone() for k, v in online.items()}

    def _copy(self, online):
        self.ema = {k: v.detach().cpu().clone() for k, v in online.items()}

    def update(self, online):
        s = self.step
        self.step += 1
        if s % self.update_every != 0:
            return 'skip'
        if s <= self.update_after_step:
            self._copy(online)
            return 'copy'
        if not self.initted:
            self._copy(online)
            self.initted = True
            return 'copy'
        d = decay_closed_form(self.step, **self.cfg)
        for k, v in online.items():
            v = v.detach().cpu()
            if v.is_floating_point():
                e = self.ema[k].double()
                self.ema[k] = (e + (1.0 - d) * (v.double() - e)).to(v.dtype)
            else:
                self.ema[k] = v.clone()
        return 'lerp'


def global_norm64(grads):
    """the L2 norm over a list of tensors, in float64 on the CPU"""
    return float(torch.sqrt(sum((g.detach().double().cpu() ** 2).sum() for g in grads)))
