"""MVIT.DROPOUT_RATE on the MI355X: the device dropout mask equals the host mask function, the dropout forms of ops.linear /
ops.mlp equal a plain-torch restatement that uses the exported mask, the fp32 model in train mode equals the oracle fed the same
drop-path and dropout masks, eval mode / rate 0 leave the default path untouched, and the HIP-graph training steps draw a fresh,
seed-reproducible key on every replay."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import lib as L                      # noqa: E402
from csts_amd.config import load_yaml              # noqa: E402
from csts_amd.build import build_model             # noqa: E402
from csts_amd.model import Block                   # noqa: E402
from csts_amd import ops, train as T               # noqa: E402
from oracle import csts_oracle as O                # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
TOL = {L.F32: 2e-5, L.BF16: 2e-2}          # tests/test_gpu_ops.py, the same ops without dropout


def key_tensor(k):
    return torch.tensor([np.int64(np.uint64(k).astype(np.int64))], dtype=torch.int64, device=DEV)


def keep_mult(key, site, shape, p):
    """(1 - mask) * scale of a site, shaped like the tensor it applies to (the exported device mask)."""
    cols = shape[-1]
    rows = int(np.prod(shape)) // cols
    _, scale = ops.dropout_params(p)
    m = ops.dropout_mask(key, site, rows, cols, p)
    return ((1 - m.float()) * scale).reshape(shape)


def make_model(compute="fp32", rate=0.1, loss="kldiv+egonce", extra=()):
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", loss, "DATA.NUM_FRAMES", 8, "CSTS_AMD.COMPUTE", compute,
                           "MVIT.DROPOUT_RATE", rate] + list(extra))
    m = build_model(cfg)
    m.load_state_dict(O.seeded_params(8, 256), strict=True)
    return m, cfg


def dev_batch(B, seed):
    return {k: v.to(DEV) for k, v in O.synthetic_batch(B, 8, 256, seed=seed).items()}


# ------------------------------------------------------------------------------------------------ G1: mask function
def test_device_mask_equals_host_mask_and_rate():
    for key, site, rows, cols in [(0x0123456789ABCDEF, 0, 1, 4096), (0xFFFFFFFFFFFFFFFF, 7, 13, 77), (0x5555AAAA3333CCCC, 79, 3, 1001),
                                  (0x0000000100000002, 2 ** 31 + 5, 17, 8)]:
        for p in (1e-3, 0.1, 0.5, 0.9):
            d = ops.dropout_mask(key_tensor(key), site, rows, cols, p).cpu().numpy().reshape(-1)
            h = ops.dropout_mask_host(key, site, 0, rows * cols, p)
            assert np.array_equal(d, h), (hex(key), site, rows, cols, p)
    n = 1 << 24
    for p in (0.1, 0.5):
        m = ops.dropout_mask(key_tensor(0x9ABCDEF012345678), 5, n // 1024, 1024, p)
        frac = float(m.double().mean())
        assert abs(frac - p) < 6 * np.sqrt(p * (1 - p) / n), (p, frac)
        head = ops.dropout_mask_host(0x9ABCDEF012345678, 5, 0, 1 << 16, p)
        assert np.array_equal(m.reshape(-1)[: 1 << 16].cpu().numpy(), head)


# ------------------------------------------------------------------------------------------------ G2: ops.linear / ops.mlp
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


@pytest.mark.parametrize("compute", [L.F32, L.BF16])
@pytest.mark.parametrize("with_rs_res", [False, True])
def test_linear_with_dropout(compute, with_rs_res):
    dt = torch.float32 if compute == L.F32 else L.half_dtype()
    B, N, K, Co, p = 2, 130, 96, 192, 0.1
    key = key_tensor(0x1234567890ABCDEF)
    x = rnd(B, N, K, seed=1).to(dt).requires_grad_(True)
    W, b = rnd(Co, K, seed=2, scale=0.1).requires_grad_(True), rnd(Co, seed=3, scale=0.1).requires_grad_(True)
    res = rnd(B, N, Co, seed=6).requires_grad_(True) if with_rs_res else None
    rs = torch.tensor([1.0 / 0.8, 0.0], device=DEV) if with_rs_res else None
    y = ops.linear(x, W, b, residual=res, row_scale=rs, rows_per_scale=N, out_dt=L.F32, compute=compute,
                   drop=ops.Dropout(key, 11, p))
    gy = rnd(B, N, Co, seed=9)
    y.backward(gy)
    got = [y.detach(), x.grad, W.grad, b.grad] + ([res.grad] if with_rs_res else [])
    km = keep_mult(key, 11, (B, N, Co), p)
    xr = x.detach().float().requires_grad_(True)
    P = [t.detach().clone().requires_grad_(True) for t in (W, b)] + ([res.detach().clone().requires_grad_(True)] if with_rs_res else [])
    yr = F.linear(xr, P[0], P[1]) * km
    if with_rs_res:
        yr = yr * rs[:, None, None] + P[2]
    yr.backward(gy)
    ref = [yr.detach(), xr.grad, P[0].grad, P[1].grad] + ([P[2].grad] if with_rs_res else [])
    tol = 1e-5 if compute == L.F32 else TOL[compute] * 2
    for i, (a, r) in enumerate(zip(got, ref)):
        assert rel_l2(a.float(), r) < tol, i
    assert (y.detach() == (res.detach() if with_rs_res else 0)).float().mean() > 0.05      # ~10 % of the branch dropped


@pytest.mark.parametrize("compute", [L.F32, L.BF16])
@pytest.mark.parametrize("with_rs_res", [False, True])
def test_mlp_with_dropout(compute, with_rs_res):
    dt = torch.float32 if compute == L.F32 else L.half_dtype()
    B, N, Cc, Hd, Co, p = 2, 130, 96, 384, 192, 0.1
    key = key_tensor(0x0FEDCBA987654321)
    x = rnd(B, N, Cc, seed=1).to(dt).requires_grad_(True)
    W1, b1 = rnd(Hd, Cc, seed=2, scale=0.1).requires_grad_(True), rnd(Hd, seed=3, scale=0.1).requires_grad_(True)
    W2, b2 = rnd(Co, Hd, seed=4, scale=0.1).requires_grad_(True), rnd(Co, seed=5, scale=0.1).requires_grad_(True)
    res = rnd(B, N, Co, seed=6).requires_grad_(True) if with_rs_res else None
    rs = torch.tensor([1.0 / 0.8, 0.0], device=DEV) if with_rs_res else None
    y = ops.mlp(x, W1, b1, W2, b2, residual=res, row_scale=rs, rows_per_scale=N, act_dt=compute, out_dt=L.F32, compute=compute,
                drop=ops.Dropout(key, 20, p))
    gy = rnd(B, N, Co, seed=9)
    y.backward(gy)
    got = [y.detach(), x.grad, W1.grad, b1.grad, W2.grad, b2.grad] + ([res.grad] if with_rs_res else [])
    k_hid, k_out = keep_mult(key, 20, (B, N, Hd), p), keep_mult(key, 21, (B, N, Co), p)
    xr = x.detach().float().requires_grad_(True)
    P = [t.detach().clone().requires_grad_(True) for t in (W1, b1, W2, b2)] + \
        ([res.detach().clone().requires_grad_(True)] if with_rs_res else [])
    yr = F.linear(F.gelu(F.linear(xr, P[0], P[1])) * k_hid, P[2], P[3]) * k_out
    if with_rs_res:
        yr = yr * rs[:, None, None] + P[4]
    yr.backward(gy)
    ref = [yr.detach(), xr.grad, P[0].grad, P[1].grad, P[2].grad, P[3].grad] + ([P[4].grad] if with_rs_res else [])
    tol = 1e-5 if compute == L.F32 else TOL[compute] * 2
    for i, (a, r) in enumerate(zip(got, ref)):
        assert rel_l2(a.float(), r) < tol, i


# ------------------------------------------------------------------------------------------------ G3: model vs oracle
def test_model_train_mode_with_dropout_vs_oracle(monkeypatch):
    """fp32 model, T=8, B=2, MVIT.DROPOUT_RATE 0.1, drop-path on, vs the oracle (run with torch on the GPU) fed the same
    drop-path keep masks and the dropout masks the model's key gives (test-local wrappers around the oracle's _drop / mlp /
    block_forward; the oracle file is not edited).  Tolerances of test_gpu_model.py at rate 0."""
    p = 0.1
    m, cfg = make_model("fp32", p)
    m.train()
    batch = dev_batch(2, 1000)
    G = O.derive_geometry()
    gen = torch.Generator().manual_seed(3)
    km = {}
    for s in G["video"]:
        if s.drop_path > 0:
            keep = 1.0 - s.drop_path
            km[s.prefix] = (torch.floor(keep + torch.rand(2, generator=gen)), torch.floor(keep + torch.rand(2, generator=gen)))
    assert any(float(a.min()) == 0.0 or float(b.min()) == 0.0 for a, b in km.values())   # some sample branch really dropped
    for q in m.parameters():
        q.grad = None
    loss, kld, nce, preds = T.compute_loss(cfg, m, batch["video"], batch["audio"], batch["labels_hm"], keep_masks=km)
    loss.backward()
    assert m._dropout_key is not None and m._dropout_key.dtype == torch.int64
    key = m._dropout_key.clone()
    sites = {n: mod.dropout_site for n, mod in m.named_modules() if isinstance(mod, Block)}

    P = {k: v.to(DEV).requires_grad_(True) for k, v in O.seeded_params(8, 256).items()}
    cur = {"prefix": None, "n": 0}
    orig_block, orig_drop = O.block_forward, O._drop

    def block_forward(x, thw, P_, spec, *a, **k):
        if spec.prefix in ("blocks.0", "blocks_audio.0"):       # pos_drop: in place, so that the recorded decoder tap sees it
            x.mul_(keep_mult(key, 0 if spec.prefix == "blocks.0" else 1, tuple(x.shape), p))
        cur["prefix"], cur["n"] = spec.prefix, 0
        return orig_block(x, thw, P_, spec, *a, **k)

    def drop(x_branch, keep_mask, drop_prob):
        site = sites[cur["prefix"]] + (0 if cur["n"] == 0 else 2)      # 1st call: attention proj, 2nd: MLP out
        cur["n"] += 1
        return orig_drop(x_branch * keep_mult(key, site, tuple(x_branch.shape), p), keep_mask, drop_prob)

    def mlp(x, P_, prefix):
        h = F.gelu(F.linear(x, P_[prefix + ".fc1.weight"], P_[prefix + ".fc1.bias"]))
        h = h * keep_mult(key, sites[cur["prefix"]] + 1, tuple(h.shape), p)
        return F.linear(h, P_[prefix + ".fc2.weight"], P_[prefix + ".fc2.bias"])

    monkeypatch.setattr(O, "block_forward", block_forward)
    monkeypatch.setattr(O, "_drop", drop)
    monkeypatch.setattr(O, "mlp", mlp)
    km_dev = {k: (a.to(DEV), b.to(DEV)) for k, (a, b) in km.items()}
    r_logits, r_v, r_a = O.csts_forward(P, batch["video"], batch["audio"], 8, 256, return_embed=True, keep_masks=km_dev)
    r_loss = O.csts_loss(r_logits, r_v, r_a, batch["labels_hm"])
    r_loss = r_loss[0] if isinstance(r_loss, (tuple, list)) else r_loss
    r_loss.backward()
    r_preds = O.frame_softmax(r_logits.detach(), 2.0)
    assert rel_l2(preds.detach(), r_preds) < 1e-4
    assert abs(float(loss) - float(r_loss.detach())) < 1e-4
    named = dict(m.named_parameters())
    total = float(torch.sqrt(sum((rp.grad.double() ** 2).sum() for rp in P.values() if rp.grad is not None)))
    for n, rp in P.items():
        if n == "classifier.bias" or rp.grad is None:
            continue
        ref_norm = float(rp.grad.double().norm())
        if ref_norm < 1e-6 * total:         # zero by softmax shift invariance (pool norm biases): rounding noise only
            continue
        gnorm = float(named[n].grad.double().norm())
        assert abs(gnorm - ref_norm) <= 2e-3 * ref_norm + 1e-12, (n, gnorm, ref_norm)


# ------------------------------------------------------------------------------------------------ G4: default path untouched
def test_eval_mode_and_rate_zero_leave_the_default_path():
    batch = dev_batch(2, 1000)
    m0, _ = make_model("fp32", 0.0)
    m0.eval()
    with torch.no_grad():
        l0 = m0([batch["video"]], batch["audio"], return_embed=True)
    m1, _ = make_model("fp32", 0.1)
    m1.eval()
    torch.manual_seed(5)
    st = torch.cuda.get_rng_state()
    with torch.no_grad():
        l1 = m1([batch["video"]], batch["audio"], return_embed=True)
    assert torch.equal(torch.cuda.get_rng_state(), st) and m1._dropout_key is None
    for a, b in zip(l0, l1):
        assert torch.equal(a, b)
    del m1
    # rate 0 in train mode: the drop-path draw only, exactly as without the feature
    m0.train()
    n_dp = 2 * sum(1 for b in m0.blocks if b.drop_prob > 0)
    torch.manual_seed(7)
    with torch.no_grad():
        m0([batch["video"]], batch["audio"])
    after = torch.cuda.get_rng_state()
    assert m0._dropout_key is None
    torch.manual_seed(7)
    torch.rand(n_dp, 2, dtype=torch.float32, device=DEV)
    assert torch.equal(torch.cuda.get_rng_state(), after)


# ------------------------------------------------------------------------------------------------ G5: graph replay
@pytest.mark.parametrize("kind", ["segmented", "graphed"])
def test_graph_steps_draw_a_fresh_reproducible_key(kind):
    import copy
    m, cfg = make_model("bf16", 0.1)
    m.train()
    m2 = copy.deepcopy(m)
    batch = T.synthetic_batch(2, 8, 256, 99, DEV)
    opt_e = T.construct_optimizer(m, cfg)
    opt_g = T.construct_optimizer(m2, cfg, capturable=True)
    state0 = copy.deepcopy(m2.state_dict())
    step = (T.SegmentedTrainStep if kind == "segmented" else T.GraphedTrainStep)(cfg, m2, opt_g, batch, warmup=1)
    m2.load_state_dict(state0)
    opt_g.reset_state()
    torch.manual_seed(11)
    le = float(T.train_step(cfg, m, batch, opt_e, lr=1e-4)[0])
    torch.manual_seed(11)
    lg = [float(step.run(batch, lr=0.0)[0]) for _ in range(3)]
    assert abs(le - lg[0]) < 1e-4, (le, lg)
    assert lg[0] != lg[1] and lg[1] != lg[2], lg           # lr 0: the weights stay, only the masks change
    torch.manual_seed(11)
    lg2 = [float(step.run(batch, lr=0.0)[0]) for _ in range(3)]
    assert lg2 == lg, (lg, lg2)
    ops.reset_deferred()


# ------------------------------------------------------------------------------------------------ G6: 16-bit modes
def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a * b).sum() / (a.norm() * b.norm()).clamp_min(1e-300))


def _grads_at(compute, seed, batch):
    m, cfg = make_model(compute, 0.1)
    m.train()
    torch.manual_seed(seed)
    loss, *_ = T.compute_loss(cfg, m, batch["video"], batch["audio"], batch["labels_hm"])
    loss.backward()
    torch.cuda.synchronize()
    out = {n: q.grad.double().flatten().cpu() for n, q in m.named_parameters()}
    return float(loss), out


def test_bf16_step_with_dropout_agrees_with_fp32():
    batch = dev_batch(2, 1000)
    l32, g32 = _grads_at("fp32", 21, batch)
    l16, g16 = _grads_at("bf16", 21, batch)
    assert np.isfinite(l16) and abs(l16 - l32) < 2e-2 * abs(l32)
    total = float(torch.sqrt(sum((v ** 2).sum() for v in g32.values())))
    bad = []
    for n, r in g32.items():
        if float(r.norm()) < 1e-6 * total:
            continue
        q = g16[n]
        assert torch.isfinite(q).all(), n
        c, ratio = _cos(q, r), float(q.norm() / r.norm())
        if c < 0.97 or not (0.95 < ratio < 1.05):
            bad.append(f"{n}: cosine {c:.5f}, ratio {ratio:.4f}")
    assert not bad, bad[:10]


def test_fp16_step_with_dropout_agrees_with_fp32(tmp_path):
    batch = dev_batch(2, 1000)
    l32, g32 = _grads_at("fp32", 21, batch)
    out = tmp_path / "fp16_dropout.pt"
    env = dict(os.environ, CSTS_HALF="fp16")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fp16_dropout_worker.py"), str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    res = torch.load(str(out))
    assert res["finite"] and abs(res["loss"] - l32) < 2e-2 * abs(l32), (res["loss"], l32)
    total = float(torch.sqrt(sum((v ** 2).sum() for v in g32.values())))
    bad = []
    for n, r in g32.items():
        if float(r.norm()) < 1e-6 * total:
            continue
        q = res["grads"][n]
        c, ratio = _cos(q, r), float(q.norm() / r.norm())
        if c < 0.97 or not (0.95 < ratio < 1.05):
            bad.append(f"{n}: cosine {c:.5f}, ratio {ratio:.4f}")
    assert not bad, bad[:10]
