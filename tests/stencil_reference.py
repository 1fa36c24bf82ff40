"""fp64 reference of the 3x3x3 depthwise stencil family (csts_amd/csrc/stencil.hip) and the error bars of tests/stencil_raw.py.
Not a test module.  Plain torch in float64, CPU or GPU, no convolution library call: the fine grid (B, T, H, W, C) is zero-padded
by 1 and the 27 strided slices  xp[:, kt + st * ot, kh + sh * oh, kw + sw * ow]  (all ot, oh, ow at once) are the taps of every
coarse position.  The strided form multiplies them by w[c % HD, k] and sums; the transposed form scatter-adds coarse * w into the
same slices of a zero padded grid and crops it; the weight gradient sums slice * coarse over batch, coarse positions and heads.
tests/test_stencil_reference_host.py holds all of this to torch's own float64 convolutions at 1e-12.

Operands come in already rounded to the type the kernel reads (16-bit tensors and fp32 weights upcast to float64), so that the
only error left in a kernel's result is fp32 accumulation plus the rounding of the output.  Next to every result the functions
return the magnitude the bars need: A = sum |x| |w| per output element, sum |fine| |coarse| per (channel of the head, tap)."""
import torch

U = 2.0 ** -24                                   # unit roundoff of the fp32 accumulation
U_OUT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HALF_SUBNORMAL = 2.0 ** -25                      # half the smallest fp16 subnormal: the absolute rounding error down there
LN_EPS = 1e-5


def coarse_grid(fine_thw, stride):
    """Output grid of a kernel-3, padding-1 convolution: floor((fine - 1) / stride) + 1 per axis."""
    return tuple((f - 1) // s + 1 for f, s in zip(fine_thw, stride))


def _pad1(x):
    B, T, H, W, C = x.shape
    xp = x.new_zeros(B, T + 2, H + 2, W + 2, C)
    xp[:, 1:T + 1, 1:H + 1, 1:W + 1] = x
    return xp


def tap_slices(xp, cthw, stride):
    """The 27 views of the padded fine grid xp (B, T+2, H+2, W+2, C): view k = kt * 9 + kh * 3 + kw holds, at coarse position o, the
    fine element o * stride - 1 + (kt, kh, kw).  (The last index, (c - 1) * s + 2, is inside the padded grid because
    (c - 1) * s <= fine - 1.)"""
    (Tc, Hc, Wc), (st, sh, sw) = cthw, stride
    out = []
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                out.append(xp[:, kt:kt + st * (Tc - 1) + 1:st, kh:kh + sh * (Hc - 1) + 1:sh, kw:kw + sw * (Wc - 1) + 1:sw])
    return out


def _wfull(w, C):
    HD = w.shape[0]
    assert w.shape == (HD, 27) and C % HD == 0 and w.dtype == torch.float64
    return w.repeat(C // HD, 1)                  # row c = w[c % HD]


def conv_strided(x, w, stride):
    """coarse[b, o, c] = sum_k fine[b, o * s - 1 + k, c] w[c % HD, k].  x (B, T, H, W, C), w (HD, 27), float64.
    Returns (y, A), both (B, Tc, Hc, Wc, C)."""
    assert x.dtype == torch.float64
    B, T, H, W, C = x.shape
    cthw = coarse_grid((T, H, W), stride)
    wf, wa = _wfull(w, C), _wfull(w, C).abs()
    y = x.new_zeros(B, *cthw, C)
    A = x.new_zeros(B, *cthw, C)
    for k, (s, sa) in enumerate(zip(tap_slices(_pad1(x), cthw, stride), tap_slices(_pad1(x.abs()), cthw, stride))):
        y += s * wf[:, k]
        A += sa * wa[:, k]
    return y, A


def conv_transposed(y, w, fine_thw, stride):
    """fine[b, f, c] = sum over (o, k) with o * s - 1 + k == f of coarse[b, o, c] w[c % HD, k]: the adjoint of conv_strided.
    y (B, Tc, Hc, Wc, C).  Returns (x, A), both (B, T, H, W, C)."""
    assert y.dtype == torch.float64
    B, C = y.shape[0], y.shape[-1]
    T, H, W = fine_thw
    cthw = coarse_grid(fine_thw, stride)
    assert tuple(y.shape[1:4]) == cthw
    wf, wa = _wfull(w, C), _wfull(w, C).abs()
    xp, Ap = y.new_zeros(B, T + 2, H + 2, W + 2, C), y.new_zeros(B, T + 2, H + 2, W + 2, C)
    ya = y.abs()
    for k, (s, sa) in enumerate(zip(tap_slices(xp, cthw, stride), tap_slices(Ap, cthw, stride))):
        s += y * wf[:, k]                        # in-place on the strided view: no two coarse positions share an element of one tap
        sa += ya * wa[:, k]
    crop = (slice(None), slice(1, T + 1), slice(1, H + 1), slice(1, W + 1))
    return xp[crop].clone(), Ap[crop].clone()


def conv_wgrad(fine, coarse, HD, stride):
    """dW[c, k] = sum over batch, coarse positions and heads of fine[b, o * s - 1 + k, h * HD + c] coarse[b, o, h * HD + c].
    Returns (dW, M, n): M = the same sum of absolute values, n = the number of addends of one element."""
    assert fine.dtype == torch.float64 and coarse.dtype == torch.float64
    B, T, H, W, C = fine.shape
    cthw = coarse_grid((T, H, W), stride)
    assert tuple(coarse.shape) == (B, *cthw, C) and C % HD == 0
    dw, mag = fine.new_zeros(HD, 27), fine.new_zeros(HD, 27)
    ca = coarse.abs()
    for k, (s, sa) in enumerate(zip(tap_slices(_pad1(fine), cthw, stride), tap_slices(_pad1(fine.abs()), cthw, stride))):
        dw[:, k] = (s * coarse).sum((0, 1, 2, 3)).view(C // HD, HD).sum(0)
        mag[:, k] = (sa * ca).sum((0, 1, 2, 3)).view(C // HD, HD).sum(0)
    return dw, mag, B * cthw[0] * cthw[1] * cthw[2] * (C // HD)


def layer_norm_heads(c, HD, gamma, beta, eps=LN_EPS):
    """LayerNorm over each head's HD-wide slice of the last axis.  c (..., C), gamma / beta (HD,), float64.
    Returns y (..., C), mean (..., heads), rstd (..., heads); the variance is the biased one, as in torch."""
    assert c.dtype == torch.float64
    r = c.reshape(*c.shape[:-1], c.shape[-1] // HD, HD)
    mean = r.mean(-1)
    d = r - mean[..., None]
    rstd = (d.pow(2).mean(-1) + eps).rsqrt()
    y = d * rstd[..., None] * gamma + beta
    return y.reshape(c.shape), mean, rstd


# ------------------------------------------------------------------------------------------------------------ the bars
def conv_bar(ref, A, out_dtype):
    """|got - ref| <= 28 u A (1 + u_out) + u_out |ref|: 27 rounded products and 27 additions in any order -- (1 + u)^28 - 1 is
    28 u in first order, FMA contraction only lowers it -- then one rounding to the output type of a value that is at most
    |ref| + 28 u A.  fp16 outputs: + half the smallest subnormal, the absolute rounding error of IEEE half below 2^-14 (a
    transposed convolution with one tap per axis produces such values from ordinary inputs: a product of two small normals)."""
    uo = U_OUT[out_dtype]
    return 28 * U * A * (1 + uo) + uo * ref.abs() + (HALF_SUBNORMAL if out_dtype == torch.float16 else 0.0)


def mean_bar(A_rows_mean, HD):
    """|mean - ref| <= (28 + HD) u x mean over the head's channels of A."""
    return (28 + HD) * U * A_rows_mean


def wgrad_bar(mag, n):
    """|dW - ref| <= (n + 1) u sum |fine| |coarse|: one rounding per product and at most n - 1 additions on the way of any addend,
    whatever the order of the sum."""
    return (n + 1) * U * mag
