"""SOLVER.OPTIMIZING_METHOD dispatch of construct_optimizer (slowfast/models/optimizer.py:82-108) on the CPU: the stock torch
optimizer of each method (device_fused=False, the numerics cross-check) with the reference's parameter groups and
hyper-parameters, and the refusals."""
import pytest
import torch
import torch.nn as nn

from csts_amd.config import get_cfg
from csts_amd.train import construct_optimizer


class Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.pos_embed = nn.Parameter(torch.zeros(1, 4, 8))
        self.proj = nn.Linear(8, 8)
        self.norm = nn.LayerNorm(8)
        self.head = nn.Linear(8, 2, bias=False)
        self.frozen = nn.Parameter(torch.zeros(3), requires_grad=False)

    def no_weight_decay(self):
        return {"head"}


def _cfg(method, **solver):
    cfg = get_cfg()
    cfg.SOLVER.OPTIMIZING_METHOD = method
    cfg.SOLVER.BASE_LR = 0.01
    cfg.SOLVER.WEIGHT_DECAY = 1e-4
    cfg.SOLVER.ZERO_WD_1D_PARAM = True
    for k, v in solver.items():
        setattr(cfg.SOLVER, k, v)
    return cfg


def _groups(m):
    decay = [m.pos_embed, m.proj.weight]
    no_decay = [m.proj.bias, m.norm.weight, m.norm.bias, m.head.weight]
    return decay, no_decay


def _check_groups(opt, m, wd):
    decay, no_decay = _groups(m)
    assert len(opt.param_groups) == 2
    g0, g1 = opt.param_groups
    assert [id(p) for p in g0["params"]] == [id(p) for p in decay] and g0["weight_decay"] == wd
    assert [id(p) for p in g1["params"]] == [id(p) for p in no_decay] and g1["weight_decay"] == 0.0


def test_sgd_is_torch_sgd_with_reference_hyper_parameters():
    m = Tiny()
    cfg = _cfg("sgd", MOMENTUM=0.9, DAMPENING=0.0, NESTEROV=True)
    opt = construct_optimizer(m, cfg, device_fused=False)
    assert type(opt) is torch.optim.SGD
    _check_groups(opt, m, 1e-4)
    d = opt.defaults
    assert d["lr"] == 0.01 and d["momentum"] == 0.9 and d["dampening"] == 0.0 and d["nesterov"] is True and d["weight_decay"] == 1e-4
    cfg = _cfg("sgd", MOMENTUM=0.5, DAMPENING=0.2, NESTEROV=False)
    opt = construct_optimizer(m, cfg, device_fused=False)
    assert opt.defaults["momentum"] == 0.5 and opt.defaults["dampening"] == 0.2 and opt.defaults["nesterov"] is False


def test_default_method_is_sgd():
    cfg = get_cfg()
    assert cfg.SOLVER.OPTIMIZING_METHOD == "sgd"
    assert type(construct_optimizer(Tiny(), cfg, device_fused=False)) is torch.optim.SGD


def test_adam_is_torch_adam():
    m = Tiny()
    opt = construct_optimizer(m, _cfg("adam"), device_fused=False)
    assert type(opt) is torch.optim.Adam
    _check_groups(opt, m, 1e-4)
    assert opt.defaults["betas"] == (0.9, 0.999) and opt.defaults["lr"] == 0.01 and opt.defaults["amsgrad"] is False


def test_adamw_is_torch_adamw():
    m = Tiny()
    opt = construct_optimizer(m, _cfg("adamw"), device_fused=False)
    assert type(opt) is torch.optim.AdamW
    _check_groups(opt, m, 1e-4)
    assert opt.defaults["eps"] == 1e-8


def test_unknown_method_is_refused():
    with pytest.raises(NotImplementedError, match="Does not support lamb optimizer"):
        construct_optimizer(Tiny(), _cfg("lamb"), device_fused=False)


@pytest.mark.parametrize("momentum,dampening", [(0.9, 0.1), (0.0, 0.0)])
def test_nesterov_needs_momentum_and_zero_dampening(momentum, dampening):
    with pytest.raises(ValueError):
        construct_optimizer(Tiny(), _cfg("sgd", MOMENTUM=momentum, DAMPENING=dampening, NESTEROV=True), device_fused=False)


def test_cpu_steps_follow_the_value_clip():
    """device_fused=False keeps the reference's clip order in the harness: clip_grad_value_ (CLIP_GRAD_VAL) before the step, with
    precedence over CLIP_GRAD_L2NORM."""
    from csts_amd.train import _clip_and_step
    m = Tiny()
    cfg = _cfg("sgd", MOMENTUM=0.0, NESTEROV=False, CLIP_GRAD_VAL=0.01, CLIP_GRAD_L2NORM=1.0)
    opt = construct_optimizer(m, cfg, device_fused=False)
    w0 = m.proj.weight.detach().clone()
    for p in m.parameters():
        if p.requires_grad:
            p.grad = torch.full_like(p, 5.0)
    _clip_and_step(cfg, m, opt)
    assert torch.allclose(m.proj.weight.detach(), w0 - 0.01 * (0.01 + 1e-4 * w0))
