"""The fp64 stencil reference of tests/stencil_reference.py against torch's own float64 operators on the CPU (no GPU needed):
F.conv3d(groups=C, padding=1, stride=s), F.conv_transpose3d with the output_padding that restores the fine grid, autograd's
weight gradient summed over the heads, and F.layer_norm -- on the ragged and degenerate geometries of tests/test_gpu_stencil.py
at a small channel count.  Agreement to 1e-12 (relative to the largest element)."""
import pytest
import torch
import torch.nn.functional as F

import stencil_reference as SR

GEOMS = [  # fine thw, stride: the table of tests/test_gpu_stencil.py
    ((3, 7, 5), (1, 2, 2)), ((4, 14, 14), (1, 8, 8)), ((3, 9, 13), (1, 4, 4)), ((3, 11, 8), (1, 3, 3)), ((5, 6, 6), (2, 2, 2)),
    ((4, 5, 5), (4, 1, 1)), ((1, 1, 6), (2, 2, 1)), ((2, 3, 3), (1, 8, 8)), ((2, 2, 2), (1, 1, 1)), ((5, 7, 6), (4, 3, 2)),
]
B, C, HD = 2, 16, 8
TOL = 1e-12


def _close(a, b):
    assert a.shape == b.shape
    return float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


def _ops(fthw, st, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, *fthw, C, generator=g, dtype=torch.float64)
    w = 0.3 * torch.randn(HD, 27, generator=g, dtype=torch.float64)
    y = torch.randn(B, *SR.coarse_grid(fthw, st), C, generator=g, dtype=torch.float64)
    wt = w.reshape(HD, 1, 3, 3, 3).repeat(C // HD, 1, 1, 1, 1)
    return x, w, y, wt


def _cl(t):       # (B, T, H, W, C) -> (B, C, T, H, W)
    return t.permute(0, 4, 1, 2, 3)


@pytest.mark.parametrize("fthw,st", GEOMS)
def test_coarse_grid(fthw, st):
    c = SR.coarse_grid(fthw, st)
    assert c == tuple((f - 1) // s + 1 for f, s in zip(fthw, st))
    x, w, y, wt = _ops(fthw, st)
    assert tuple(F.conv3d(_cl(x), wt, stride=st, padding=1, groups=C).shape[2:]) == c


@pytest.mark.parametrize("fthw,st", GEOMS)
def test_strided_equals_conv3d(fthw, st):
    x, w, y, wt = _ops(fthw, st, 1)
    got, A = SR.conv_strided(x, w, st)
    assert _close(got, F.conv3d(_cl(x), wt, stride=st, padding=1, groups=C).permute(0, 2, 3, 4, 1))
    assert _close(A, F.conv3d(_cl(x.abs()), wt.abs(), stride=st, padding=1, groups=C).permute(0, 2, 3, 4, 1))
    assert bool((A >= got.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("fthw,st", GEOMS)
def test_transposed_equals_conv_transpose3d(fthw, st):
    x, w, y, wt = _ops(fthw, st, 2)
    cthw = SR.coarse_grid(fthw, st)
    op = [f - ((c - 1) * s - 2 + 3) for f, c, s in zip(fthw, cthw, st)]      # output_padding that restores the fine grid
    got, A = SR.conv_transposed(y, w, fthw, st)
    if all(0 <= o < s for o, s in zip(op, st)):
        ref = F.conv_transpose3d(_cl(y), wt, stride=st, padding=1, output_padding=op, groups=C).permute(0, 2, 3, 4, 1)
        refA = F.conv_transpose3d(_cl(y.abs()), wt.abs(), stride=st, padding=1, output_padding=op, groups=C).permute(0, 2, 3, 4, 1)
    else:       # torch refuses output_padding >= stride (a grid smaller than its stride): the adjoint, through autograd
        xr = torch.zeros(B, *fthw, C, dtype=torch.float64, requires_grad=True)
        F.conv3d(_cl(xr), wt, stride=st, padding=1, groups=C).backward(_cl(y))
        ref = xr.grad
        xr = torch.zeros(B, *fthw, C, dtype=torch.float64, requires_grad=True)
        F.conv3d(_cl(xr), wt.abs(), stride=st, padding=1, groups=C).backward(_cl(y.abs()))
        refA = xr.grad
    assert _close(got, ref) and _close(A, refA)
    # and it is the adjoint of the strided form: <conv(x), y> == <x, conv^T(y)>
    fwd, _ = SR.conv_strided(x, w, st)
    assert abs(float((fwd * y).sum() - (x * got).sum())) <= 1e-10 * float((fwd.abs() * y.abs()).sum())


@pytest.mark.parametrize("fthw,st", GEOMS)
def test_wgrad_equals_autograd(fthw, st):
    x, w, y, wt = _ops(fthw, st, 3)
    wr = torch.zeros(C, 1, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv3d(_cl(x), wr, stride=st, padding=1, groups=C).backward(_cl(y))
    got, mag, n = SR.conv_wgrad(x, y, HD, st)
    assert _close(got, wr.grad.view(C // HD, HD, 27).sum(0))
    wr = torch.zeros(C, 1, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv3d(_cl(x.abs()), wr, stride=st, padding=1, groups=C).backward(_cl(y.abs()))
    assert _close(mag, wr.grad.view(C // HD, HD, 27).sum(0))
    cthw = SR.coarse_grid(fthw, st)
    assert n == B * cthw[0] * cthw[1] * cthw[2] * (C // HD)


@pytest.mark.parametrize("HDl,heads", [(8, 1), (8, 3), (104, 2), (96, 2)])
def test_layer_norm_heads_equals_layer_norm(HDl, heads):
    g = torch.Generator().manual_seed(4)
    c = torch.randn(3, 5, heads * HDl, generator=g, dtype=torch.float64) * 2 + 0.5
    gamma = 1 + 0.1 * torch.randn(HDl, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(HDl, generator=g, dtype=torch.float64)
    y, mean, rstd = SR.layer_norm_heads(c, HDl, gamma, beta)
    r = c.reshape(3, 5, heads, HDl)
    assert _close(y, F.layer_norm(r, (HDl,), gamma, beta, 1e-5).reshape(c.shape))
    assert _close(mean, r.mean(-1)) and _close(rstd, (r.var(-1, unbiased=False) + 1e-5).rsqrt())
    assert mean.shape == rstd.shape == (3, 5, heads)


def test_bars_shapes_and_values():
    ref, A = torch.tensor([1.0, -2.0]).double(), torch.tensor([3.0, 4.0]).double()
    b32 = SR.conv_bar(ref, A, torch.float32)
    assert torch.equal(b32, 28 * SR.U * A)
    b16 = SR.conv_bar(ref, A, torch.bfloat16)
    assert torch.allclose(b16, 28 * SR.U * A * (1 + 2.0 ** -8) + 2.0 ** -8 * ref.abs(), rtol=0, atol=0)
    b16 = SR.conv_bar(ref, A, torch.float16)
    assert torch.equal(b16, 28 * SR.U * A * (1 + 2.0 ** -11) + 2.0 ** -11 * ref.abs() + 2.0 ** -25)
    assert torch.equal(SR.wgrad_bar(A, 9), 10 * SR.U * A) and torch.equal(SR.mean_bar(A, 8), 36 * SR.U * A)
