"""GPU parity tests of the device-fused optimizers for every SOLVER.OPTIMIZING_METHOD (slowfast/models/optimizer.py:82-108):
FusedSGD == torch.optim.SGD, FusedAdam == torch.optim.Adam, FusedAdamW with clip_value == clip_grad_value_ + torch.optim.AdamW
(tools/train_avgaze_net.py:101-109), through the chunk-table step, the 16-bit gradient buckets, the loss scaler and the factored
(fusion-conv) updates, plus the torch state_dict layouts both ways.  Tolerances of the AdamW tests in test_gpu_ops.py."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected everywhere, run only on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import lib as L                                      # noqa: E402
from csts_amd.optim import CHUNK, FusedAdam, FusedAdamW, FusedSGD  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(768, 300), (96,), (5,), (CHUNK + 1,), (1, 409, 96), (131, 7), (2 * CHUNK,), (33,)]
DECAY = [0, 4, 5, 6]
NOGRAD = 7
SGD_SETTINGS = {"nesterov": dict(momentum=0.9, dampening=0.0, nesterov=True),
                "damped": dict(momentum=0.9, dampening=0.1, nesterov=False),
                "plain": dict(momentum=0.0, dampening=0.0, nesterov=False)}
CLIPS = {"norm": dict(max_grad_norm=1.0), "value": dict(clip_value=0.01)}


def rnd(*shape, seed=0, scale=1.0, dt=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dt)


def _groups(ps, wd=0.05):
    return [{"params": [ps[i] for i in DECAY], "weight_decay": wd},
            {"params": [ps[i] for i in range(len(ps)) if i not in DECAY], "weight_decay": 0.0}]


def _make(method, groups, lr, clip, shadows=None, **kw):
    if method == "sgd":
        return FusedSGD(groups, lr=lr, shadows=shadows, **clip, **kw)
    cls = FusedAdam if method == "adam" else FusedAdamW
    return cls(groups, lr=lr, eps=1e-8, shadows=shadows, **clip, **kw)


def _torch(method, groups, lr, wd=0.05, **kw):
    if method == "sgd":
        return torch.optim.SGD(groups, lr=lr, weight_decay=wd, **kw)
    if method == "adam":
        return torch.optim.Adam(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    return torch.optim.AdamW(groups, lr=lr, eps=1e-8, weight_decay=wd)


def _torch_clip(ps, clip):
    if "clip_value" in clip:
        torch.nn.utils.clip_grad_value_(ps, clip["clip_value"])
        return None
    return torch.nn.utils.clip_grad_norm_(ps, clip["max_grad_norm"])


def _set_lr(fused, ref, lr):
    for grp in fused.param_groups:
        grp["lr"].fill_(lr)
    for grp in ref.param_groups:
        grp["lr"] = lr


CASES = [("sgd", s, c) for s in SGD_SETTINGS for c in CLIPS] + [("adam", None, c) for c in CLIPS] + [("adamw", None, "value")]


@pytest.mark.parametrize("method,setting,clip", CASES)
@pytest.mark.parametrize("grad16", [False, True])
def test_fused_method_matches_torch(method, setting, clip, grad16):
    """Ragged shapes (chunk boundaries, unaligned tails), a parameter that never has a gradient, two weight-decay groups, a
    changing learning rate, gradient scales on both sides of the clips.  grad16: the gradients arrive as 16-bit bucket views
    (set_external_grads); torch then steps on the same rounded gradients."""
    base_lr = 1e-2 if method == "sgd" else 1e-3
    kw = SGD_SETTINGS[setting] if method == "sgd" else {}
    pa = [rnd(*s, seed=10 + i, scale=0.5).requires_grad_() for i, s in enumerate(SHAPES)]
    pb = [p.detach().clone().requires_grad_() for p in pa]
    shadow = torch.empty(SHAPES[0], dtype=L.half_dtype(), device=DEV)
    fused = _make(method, _groups(pa), base_lr, CLIPS[clip], shadows={id(pa[0]): shadow}, **kw)
    ref = _torch(method, _groups(pb), base_lr, **kw)
    if method == "sgd" and kw["momentum"] == 0.0:
        assert fused.momentum_buffer is None and all(m is None for m in fused._m)      # no buffer at all
    for step, gscale in enumerate([1.0, 1e-4, 3.0, 0.02, 0.5, 2e-3]):
        ext = {}
        for i, (a, b) in enumerate(zip(pa, pb)):
            a.grad, b.grad = None, None
            if i == NOGRAD:
                continue
            g = rnd(*SHAPES[i], seed=100 * step + i, scale=gscale)
            if grad16:
                g16 = g.to(L.half_dtype())
                ext[id(a)] = g16
                b.grad = g16.float()
            else:
                a.grad, b.grad = g.clone(), g.clone()
        if grad16:
            fused.set_external_grads(ext, L.BF16)
        _set_lr(fused, ref, base_lr * (1 + step))
        norm_ref = _torch_clip(pb, CLIPS[clip])
        ref.step()
        fused.step()
        if norm_ref is not None:
            assert abs(float(fused.grad_norm) - float(norm_ref)) < 1e-5 * float(norm_ref)
        for i, (a, b) in enumerate(zip(pa, pb)):
            assert rel_l2(a.detach(), b.detach()) < 2e-6, (step, i)
    assert torch.equal(shadow, pa[0].detach().to(L.half_dtype()))
    assert torch.equal(pa[NOGRAD].detach(), pb[NOGRAD].detach())
    assert fused.step_count() == 6
    if method == "sgd" and kw["momentum"]:
        i3 = [id(p) for p in fused.params].index(id(pa[3]))
        assert rel_l2(fused._m[i3].view(SHAPES[3]), ref.state[pb[3]]["momentum_buffer"]) < 2e-6
        assert fused.state_dict()["state"][[id(p) for p in fused.params].index(id(pa[NOGRAD]))]["momentum_buffer"] is None


def test_value_clip_and_norm_clip_are_exclusive():
    p = rnd(64, seed=1).requires_grad_()
    with pytest.raises(ValueError):
        FusedSGD([{"params": [p], "weight_decay": 0.0}], lr=0.1, momentum=0.9, max_grad_norm=1.0, clip_value=0.5)
    with pytest.raises(ValueError):
        FusedSGD([{"params": [p], "weight_decay": 0.0}], lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)
    with pytest.raises(ValueError):
        FusedSGD([{"params": [p], "weight_decay": 0.0}], lr=0.1, momentum=0.0, nesterov=True)


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_loss_scaler_skip_matches_gradscaler(method):
    """fp16-style dynamic loss scaling inside the kernels against torch.cuda.amp.GradScaler + the torch optimizer: a non-finite
    gradient in step 2 leaves parameters, buffers and the momentum first-step state unchanged and backs the scale off; the
    sequence of parameters and scales matches.  Step 0 is the skipped one for a second run: the buffer must then be initialised by
    the first GOOD step (torch: buf = clone(d)), not continued from zeros."""
    kw = dict(momentum=0.9, dampening=0.1) if method == "sgd" else {}
    for bad_step in (2, 0):
        pa = [rnd(300, 40, seed=1, scale=0.5).requires_grad_(), rnd(77, seed=2, scale=0.5).requires_grad_()]
        pb = [p.detach().clone().requires_grad_() for p in pa]
        ga = [{"params": [pa[0]], "weight_decay": 0.05}, {"params": [pa[1]], "weight_decay": 0.0}]
        gb = [{"params": [pb[0]], "weight_decay": 0.05}, {"params": [pb[1]], "weight_decay": 0.0}]
        fused = _make(method, ga, 1e-2, {"max_grad_norm": 1.0}, loss_scaling=True, init_scale=1024.0, growth_interval=2, **kw)
        ref = _torch(method, gb, 1e-2, **kw)
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
        for step in range(5):
            grads = [rnd(*p.shape, seed=40 * step + i, scale=0.3) for i, p in enumerate(pa)]
            if step == bad_step:
                grads[0][3, 5] = float("inf")
            scale = float(fused.loss_scale)
            assert scale == float(scaler.scale(torch.ones((), device=DEV))), (bad_step, step)      # scaler.scale(loss)
            for a, b, g in zip(pa, pb, grads):
                a.grad, b.grad = g * scale, g * scale
            before = [t.clone() for t in fused.device_state()] + [p.detach().clone() for p in pa]
            steps_before = fused.step_count()
            scaler.unscale_(ref)
            torch.nn.utils.clip_grad_norm_(pb, 1.0)
            scaler.step(ref)
            scaler.update()
            fused.step()
            if step == bad_step:
                assert float(fused.state_t[3]) == 1.0 and float(fused.loss_scale) == scale * 0.5
                after = [t for t in fused.device_state()] + [p.detach() for p in pa]
                for k, (x, y) in enumerate(zip(before, after)):
                    if y.data_ptr() in (fused.scaler_t.data_ptr(), fused.state_t.data_ptr()):
                        continue
                    assert torch.equal(x, y), (bad_step, k)
                assert fused.step_count() == steps_before
            for a, b in zip(pa, pb):
                assert rel_l2(a.detach(), b.detach()) < 2e-6, (bad_step, step)
        assert fused.step_count() == 4
        assert float(fused.loss_scale) == scaler.get_scale()


@pytest.mark.parametrize("method", ["sgd", "adam"])
@pytest.mark.parametrize("a_dtype,T,clip", [(torch.float32, 32, "norm"), (torch.bfloat16, 128, "norm"), (torch.bfloat16, 128, "value"),
                                           (torch.float32, 32, "value")])
def test_factored_update_matches_dense_gradient(method, a_dtype, T, clip):
    """The fusion-conv weights updated from their factors (dW = dY^T A formed inside the update: the LDS form for fp32 A with
    T <= 64, the MFMA form for 16-bit A) == the same optimizer fed the materialised dW, for the sgd and adam rules."""
    if a_dtype != torch.float32 and L.half_dtype() != torch.bfloat16:
        pytest.skip("16-bit operands of this library are not bfloat16")
    kw = dict(momentum=0.9, nesterov=True) if method == "sgd" else {}
    N, K = 64, 2048
    shapes = [(N, 8, 16, 16), (300,), (96, 32)]
    dy16 = (lambda t: t.to(a_dtype).float()) if a_dtype != torch.float32 else (lambda t: t)
    pa = [rnd(*s, seed=10 + i, scale=0.5).requires_grad_() for i, s in enumerate(shapes)]
    pb = [p.detach().clone().requires_grad_() for p in pa]
    ga = [{"params": [pa[0], pa[2]], "weight_decay": 0.05}, {"params": [pa[1]], "weight_decay": 0.0}]
    gb = [{"params": [pb[0], pb[2]], "weight_decay": 0.05}, {"params": [pb[1]], "weight_decay": 0.0}]
    shadow = torch.empty(shapes[0], dtype=L.half_dtype(), device=DEV)
    lr = 1e-2 if method == "sgd" else 1e-3
    fused = _make(method, ga, lr, CLIPS[clip], shadows={id(pa[0]): shadow}, **kw)
    dense = _make(method, gb, lr, CLIPS[clip], **kw)
    for step, gscale in enumerate([1.0, 1e-3, 2.0]):
        dy = rnd(T, N, seed=50 * step, scale=gscale)
        a = rnd(T, K, seed=70 * step).to(a_dtype)
        pb[0].grad = (dy16(dy).t() @ a.float()).view(shapes[0])
        pa[0].grad = None
        for i in (1, 2):
            g = rnd(*shapes[i], seed=100 * step + i, scale=gscale)
            pa[i].grad, pb[i].grad = g.clone(), g.clone()
        fused.set_factored([(pa[0], dy, a)])
        dense.step()
        fused.step()
        if clip == "norm":
            tol = 2e-5 if T <= 64 else 1e-4
            assert abs(float(fused.grad_norm) - float(dense.grad_norm)) < tol * float(dense.grad_norm)
        for i, (x, y) in enumerate(zip(pa, pb)):
            assert rel_l2(x.detach(), y.detach()) < 3e-6, (step, i)
    assert torch.equal(shadow, pa[0].detach().to(L.half_dtype()))


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_state_dict_round_trips_through_torch(method):
    """Fused -> torch: the fused state loads into torch.optim.SGD / Adam and one more step of each agrees.  Torch -> fused: the
    loaded momentum buffer is USED by the next step (not re-initialised from the gradient), the moments and step count too."""
    kw = dict(momentum=0.9, dampening=0.1) if method == "sgd" else {}
    shapes = [(64, 40), (96,), (3, 5, 7)]

    def groups(ps):
        return [{"params": [ps[0], ps[2]], "weight_decay": 0.05}, {"params": [ps[1]], "weight_decay": 0.0}]

    def grads(seed):
        return [rnd(*s, seed=seed + i) for i, s in enumerate(shapes)]

    # fused -> torch
    pa = [rnd(*s, seed=20 + i, scale=0.5).requires_grad_() for i, s in enumerate(shapes)]
    pb = [p.detach().clone().requires_grad_() for p in pa]
    fused = _make(method, groups(pa), 2e-3, {"max_grad_norm": 0.0}, **kw)
    for step in range(3):
        for a, g in zip(pa, grads(300 + 10 * step)):
            a.grad = g
        fused.step()
    for a, b in zip(pa, pb):
        b.data.copy_(a.data)
    ref = _torch(method, groups(pb), 1.0, **kw)
    ref.load_state_dict(fused.state_dict())
    assert abs(ref.param_groups[0]["lr"] - 2e-3) < 1e-9
    for a, b, g in zip(pa, pb, grads(900)):
        a.grad, b.grad = g.clone(), g.clone()
    ref.step(); fused.step()
    for a, b in zip(pa, pb):
        assert rel_l2(a.detach(), b.detach()) < 2e-6

    # torch -> fused
    pc = [rnd(*s, seed=40 + i, scale=0.5).requires_grad_() for i, s in enumerate(shapes)]
    pd = [p.detach().clone().requires_grad_() for p in pc]
    ref2 = _torch(method, groups(pd), 2e-3, **kw)
    for step in range(2):
        for b, g in zip(pd, grads(500 + 10 * step)):
            b.grad = g
        ref2.step()
    for c, d in zip(pc, pd):
        c.data.copy_(d.data)
    fused2 = _make(method, groups(pc), 1e-5, {"max_grad_norm": 0.0}, **kw)
    fused2.load_state_dict(ref2.state_dict())
    assert fused2.step_count() == (0 if method == "sgd" else 2)       # torch.optim.SGD keeps no step counter
    for c, d, g in zip(pc, pd, grads(700)):
        c.grad, d.grad = g.clone(), g.clone()
    ref2.step(); fused2.step()
    for c, d in zip(pc, pd):
        assert rel_l2(c.detach(), d.detach()) < 2e-6
    if method == "sgd":
        assert rel_l2(fused2._m[0].view(shapes[0]), ref2.state[pd[0]]["momentum_buffer"]) < 2e-6
    # a state of another method, or of other parameters, is refused
    other = _torch("adamw", groups(pd), 1e-3) if method == "sgd" else _torch("sgd", groups(pd), 1e-3, momentum=0.9)
    for b, g in zip(pd, grads(800)):
        b.grad = g
    other.step()
    with pytest.raises(ValueError):
        fused2.load_state_dict(other.state_dict())
    bad = fused2.state_dict()
    key = "momentum_buffer" if method == "sgd" else "exp_avg"
    bad["state"][0][key] = torch.zeros(3)
    with pytest.raises(ValueError):
        fused2.load_state_dict(bad)
