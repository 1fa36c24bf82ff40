"""CPU tests of tests/layernorm_reference.py: the fp64 LayerNorm reference against torch's own float64 layer_norm and autograd, the
proof that the `offset` values of the GPU tests tell a one-pass variance from a two-pass one, and the exact-order emulations of the
row reducers inside their derived bars."""
import pytest
import torch

import layernorm_reference as LR

# The fp32-storage bars of tests/test_gpu_layernorm.py (which asserts that these copies equal its own constants).
RSTD_REL_F32 = 6.4e-7
K_Y_F32 = 44.0
EPS = 1e-6


@pytest.mark.parametrize("C", [8, 100, 768])
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "addend-dy2"])
def test_reference_matches_torch_float64(C, extras):
    rows = 37
    x = LR.values("offset", rows, C, 1).double()
    a = LR.values("plain", rows, C, 2).double() if extras else None
    dy = LR.values("plain", rows, C, 3).double()
    dy2 = LR.values("plain", rows, C, 4).double() if extras else None
    res = LR.values("plain", rows, C, 5).double() if extras else None
    gamma, beta = (t.double() for t in LR.params(C, 6))
    f = LR.forward(x, gamma, beta, EPS, addend=a)
    s = (x if a is None else x + a).clone().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(s, (C,), gt, bt, EPS)
    y.backward(dy if dy2 is None else dy + dy2)
    assert torch.allclose(f["y"], y.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(f["mean"], s.detach().mean(-1), rtol=1e-13, atol=0)
    assert torch.allclose(f["var"], s.detach().var(-1, unbiased=False), rtol=1e-10, atol=1e-13)
    b = LR.backward(dy, f["sum"], gamma, f["mean"], f["rstd"], dy2=dy2, addend=res)
    want_dx = s.grad if res is None else s.grad + res
    assert torch.allclose(b["dx"], want_dx, rtol=1e-10, atol=1e-11)
    assert torch.allclose(b["dgamma"], gt.grad, rtol=1e-10, atol=1e-10)
    assert torch.allclose(b["dbeta"], bt.grad, rtol=1e-12, atol=1e-12)
    # the scales dominate what they scale
    assert bool((f["S_y"] >= f["y"].abs() * (1 - 1e-12)).all()) and bool((b["S_dx"] >= b["dx"].abs() * (1 - 1e-12)).all())
    assert bool((b["S_dg"] >= b["dgamma"].abs()).all()) and bool((b["S_db"] >= b["dbeta"].abs()).all())


def test_copy16_rows_per_scale():
    dx = LR.values("plain", 14, 8, 7).double()
    scale = torch.tensor([0.0, 1.5], dtype=torch.float64)
    c = LR.copy16(dx, scale, 7, torch.bfloat16)
    assert bool((c[:7] == 0).all()) and torch.equal(c[7:], (dx[7:] * 1.5).to(torch.bfloat16))
    assert torch.equal(LR.copy16(dx, None, 1, torch.float16), dx.to(torch.float16))
    bar = LR.copy_bar(dx, scale, 7, torch.bfloat16)
    assert bool(((c.double() - dx * LR.row_scale(scale, 14, 7)).abs() <= bar).all())


def _forward_ratios(C, kind, one_pass):
    x = LR.values(kind, 257, C, 11 + C)
    gamma, beta = LR.params(C, 12 + C)
    f = LR.forward(x.double(), gamma.double(), beta.double(), EPS)
    e = LR.forward_f32(x, gamma, beta, EPS, one_pass=one_pass)
    mean_ratio = ((e["mean"].double() - f["mean"]).abs() / LR.mean_bar(x.double(), C)).max().item()
    rstd_rel = ((e["rstd"].double() - f["rstd"]).abs() / f["rstd"]).max().item()
    k_y = ((e["y"].double() - f["y"]).abs() / (LR.U * f["S_y"])).max().item()
    return mean_ratio, rstd_rel, k_y, f["var"].min().item()


@pytest.mark.parametrize("C", [8, 96, 100, 192, 384, 768])
def test_offset_values_separate_one_pass_from_two_pass(C):
    """x ~ N(64, 1): the fp32 two-pass forward stays inside the mean, rstd and y bars (so the path from the inputs to the fp64
    reference costs nothing the bars would notice); the one-pass E[x^2] - mean^2 misses the rstd bar by at least 10x.  On zero-mean
    data both forms pass: only the offset separates them."""
    mean_ratio, rstd_rel, k_y, min_var = _forward_ratios(C, "offset", False)
    print(f"\n[C {C} offset two-pass] mean ratio {mean_ratio:.3f}  rstd rel {rstd_rel:.3e}  K_y {k_y:.2f}  min var {min_var:.3f}")
    assert mean_ratio <= 1.0 and rstd_rel <= RSTD_REL_F32 and k_y <= K_Y_F32
    _, rstd1, k_y1, _ = _forward_ratios(C, "offset", True)
    print(f"[C {C} offset one-pass] rstd rel {rstd1:.3e}  K_y {k_y1:.2f}")
    assert rstd1 >= 10 * RSTD_REL_F32
    _, rstd0, _, _ = _forward_ratios(C, "plain", True)
    assert rstd0 <= RSTD_REL_F32, "on zero-mean data a one-pass variance is as good: the offset is what discriminates"


ROWS_SHAPES = [(n, c) for n in (1, 2, 3, 8, 9, 63, 64, 65, 129, 515) for c in (1, 31, 32, 33, 192, 1536)]
WIDE_SHAPES = [(n, c) for n in (1, 3, 4, 5, 8, 13) for c in (4, 1020, 36864)] + [(2, 4 * (4096 * 256 + 3))]


@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_row_reducer_emulations_within_derived_bar(scale):
    worst = 0.0
    for nrows, ncols in ROWS_SHAPES:
        ws = LR.mixed(nrows, ncols, 100 + nrows + ncols)
        ref, absum = LR.reduce_ref(ws, scale)
        for RL in {LR.reduce_rl(nrows), 32}:              # csts_reduce_rows' kernel for this height, and the batched kernel
            got = LR.reduce_rows_emulation(ws, scale, RL)
            r = ((got.double() - ref).abs() / LR.reduce_bar(absum, scale, nrows, RL)).max().item()
            worst = max(worst, r)
            assert r <= 1.0, (nrows, ncols, RL, r)
    print(f"\n[row reducer emulations, scale {scale}] worst ratio {worst:.3f}")


def test_row_reducer_emulation_order_shows_in_the_bits():
    """The three row-lane counts give different bits on the mixed-magnitude data: the bit-equality of the GPU tests is specific."""
    ws = LR.mixed(129, 192, 5)
    outs = [LR.reduce_rows_emulation(ws, 1.0, RL) for RL in (2, 8, 32)]
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    assert not torch.equal(outs[2], LR.reduce_wide_emulation(ws, 1.0))
    assert LR.reduce_rl(8) == 2 and LR.reduce_rl(9) == 8 and LR.reduce_rl(64) == 8 and LR.reduce_rl(65) == 32


def test_wide_reducer_emulation_within_derived_bar():
    worst = 0.0
    for nrows, ncols in WIDE_SHAPES:
        ws = LR.mixed(nrows, ncols, 200 + nrows)
        for scale in (1.0, 0.37):
            ref, absum = LR.reduce_ref(ws, scale)
            r = ((LR.reduce_wide_emulation(ws, scale).double() - ref).abs() / LR.reduce_bar(absum, scale, nrows)).max().item()
            worst = max(worst, r)
            assert r <= 1.0, (nrows, ncols, scale, r)
    print(f"\n[wide reducer emulation] worst ratio {worst:.3f}")
