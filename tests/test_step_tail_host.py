"""Host side of the step tail (phenaki_pytorch_amd/step_tail.py, optim.py): names, argument errors, the optimizer's unchanged state_dict and the
EMA schedule -- everything that needs no device."""
import pytest
import torch
from torch import nn

from tests.step_tail_restatement import cadence, decay_closed_form


def _cpu_params():
    ps = [nn.Parameter(torch.randn(4, 3)), nn.Parameter(torch.randn(5))]
    for p in ps:
        p.grad = torch.randn_like(p)
    return ps


def test_names_are_exported():
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd import _lib
    for name in ('clip_grad_norm_', 'EMA', 'HipAdamW', 'get_optimizer'):
        assert name in P.__all__ and hasattr(P, name)
    for sym in ('pk_grad_sumsq_parts', 'pk_grad_sumsq', 'pk_grad_clip_coef', 'pk_scale_multi', 'pk_adamw_multi_scaled', 'pk_ema_multi'):
        assert sym in _lib.SIGNATURES


def test_other_norm_types_are_refused():
    import phenaki_pytorch_amd as P
    with pytest.raises(ValueError):
        P.clip_grad_norm_(_cpu_params(), 1.0, norm_type=1)
    with pytest.raises(ValueError):
        P.clip_grad_norm_(_cpu_params(), 1.0, norm_type=float('inf'))


def test_cpu_tensors_have_no_fallback():
    import phenaki_pytorch_amd as P
    ps = _cpu_params()
    before = [p.grad.clone() for p in ps]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        P.clip_grad_norm_(ps, 1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        P.clip_grad_norm_(ps[0], 1.0)                                  # a single parameter is accepted like an iterable
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        P.HipAdamW(ps, max_grad_norm=0.5).step()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        P.get_optimizer(ps, max_grad_norm=0.5).step()
    assert all(torch.equal(p.grad, b) for p, b in zip(ps, before))
    ema = P.EMA(nn.Linear(3, 2), update_after_step=0, update_every=1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ema.update()


def test_max_grad_norm_is_not_a_state_dict_key():
    import phenaki_pytorch_amd as P
    plain = P.HipAdamW(_cpu_params())
    clipped = P.HipAdamW(_cpu_params(), max_grad_norm=0.5)
    keys = {'lr', 'betas', 'eps', 'weight_decay', 'params'}
    for opt in (plain, clipped):
        for group in opt.state_dict()['param_groups']:
            assert 'max_grad_norm' not in group
            assert keys <= set(group)
    assert [set(g) for g in plain.state_dict()['param_groups']] == [set(g) for g in clipped.state_dict()['param_groups']]
    assert plain.max_grad_norm is None and clipped.max_grad_norm == 0.5 and clipped.last_grad_norm is None
    both = P.get_optimizer(_cpu_params(), wd=1e-2, max_grad_norm=0.25)
    assert both.max_grad_norm == 0.25 and len(both.param_groups) == 2
    assert P.get_optimizer(_cpu_params(), wd=0, max_grad_norm=0.25).max_grad_norm == 0.25
    assert P.get_optimizer(_cpu_params()).max_grad_norm is None


@pytest.mark.parametrize('cfg', [dict(update_after_step=3, update_every=2), dict(update_after_step=10, update_every=1, inv_gamma=2.0, power=0.75, min_value=0.3, beta=0.85)])
def test_current_decay_matches_the_closed_form(cfg):
    import phenaki_pytorch_amd as P
    ema = P.EMA(nn.Linear(3, 2), **cfg)
    seen = set()
    for step in range(51):
        ema.step = step
        want = decay_closed_form(step, cfg['update_after_step'], cfg.get('inv_gamma', 1.0), cfg.get('power', 2 / 3), cfg.get('min_value', 0.0), cfg.get('beta', 0.9999))
        assert ema.current_decay() == pytest.approx(want, rel=1e-12, abs=0)
        assert cfg.get('min_value', 0.0) <= ema.current_decay() <= cfg.get('beta', 0.9999) or want == 0.0
        seen.add(round(want, 6))
    assert 0.0 in seen and len(seen) > 5
    if 'beta' in cfg:
        assert cfg['beta'] in seen and cfg['min_value'] in seen         # both clamps are reached within 50 steps


def test_update_cadence_is_a_host_sequence():
    import phenaki_pytorch_amd as P
    ema = P.EMA(nn.Linear(3, 2), update_after_step=3, update_every=2)
    got = []
    for _ in range(12):
        assert ema.next_decision() == ema.next_decision()               # looking does not advance
        got.append(ema.advance())
    assert got == ['copy', 'skip', 'copy', 'skip', 'copy', 'skip', 'lerp', 'skip', 'lerp', 'skip', 'lerp', 'skip']
    assert got == cadence(12, 3, 2)
    assert ema.step == 12 and ema.initted
    for uas, every in ((0, 1), (1, 2), (5, 3), (100, 10)):
        e = P.EMA(nn.Linear(3, 2), update_after_step=uas, update_every=every)
        assert [e.advance() for _ in range(40)] == cadence(40, uas, every)


def test_extra_state_round_trip():
    import phenaki_pytorch_amd as P
    model = nn.Linear(3, 2)
    ema = P.EMA(model, update_after_step=3, update_every=2)
    for _ in range(7):
        ema.advance()
    assert ema.get_extra_state() == dict(step=7, initted=True)
    sd = ema.state_dict()
    assert '_extra_state' in sd and 'ema_model.weight' in sd and not any(k.startswith('_online') or k.startswith('online') for k in sd)
    fresh = P.EMA(nn.Linear(3, 2), update_after_step=3, update_every=2)
    fresh.load_state_dict(sd)
    assert (fresh.step, fresh.initted) == (7, True)
    assert fresh.current_decay() == ema.current_decay() and fresh.next_decision() == ema.next_decision()
    assert torch.equal(fresh.ema_model.weight, ema.ema_model.weight)
    assert [fresh.advance() for _ in range(6)] == [ema.advance() for _ in range(6)]
    assert not any(p.requires_grad for p in ema.ema_model.parameters())
    assert list(ema.parameters()) == list(ema.ema_model.parameters())   # the online model is not registered
    assert ema.online_model is model
