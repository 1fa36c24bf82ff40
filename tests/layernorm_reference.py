"""fp64 reference of the LayerNorm kernels and the row reducers of csts_amd/csrc/norm.hip, the error scales the bars of
tests/layernorm_raw.py use, and exact-order fp32 emulations of the reducers.  Not a test module.  Plain torch in float64, CPU or
GPU, no autograd and no library LayerNorm inside: the formulas are written out.  tests/test_layernorm_reference_host.py holds
them to torch.nn.functional.layer_norm and its autograd in float64.

Operands come in already rounded to the type the kernel reads (16-bit tensors and fp32 parameters upcast to float64), so that the
only error left in a kernel's result is its fp32 arithmetic plus the rounding of the output.  The backward takes `mean` and `rstd`
as operands, like the kernel: the fp32 values the forward stored, upcast.

Forward    mean = mean_c(x), var = mean_c((x - mean)^2) (biased), rstd = (var + eps)^-1/2, y = (x - mean) rstd gamma + beta;
           with an addend, x + addend is what is normalised (and returned as `sum`).
Backward   g = (dy [+ dy2]) gamma, xhat = (x - mean) rstd,
           dx = rstd (g - mean_c(g) - xhat mean_c(g xhat)) [+ addend], dgamma = sum_rows dy xhat, dbeta = sum_rows dy,
           copy = round16(dx scale[row / rps]).
Scales     S_y  = |gamma_c| rstd (|x_c| + |mean|) + |beta_c|
           S_dx = rstd (|g_c| + mean_c|g| + |xhat_c| mean_c|g xhat|) + |addend_c|
           S_dg = sum_rows |dy xhat|,  S_db = sum_rows |dy|

Derived bars (u = 2^-24; u_out = 0 / 2^-8 / 2^-11 for fp32 / bf16 / fp16 storage):
  mean      |err| <= (C + 1) u mean_c|x|: every addend passes at most C - 1 additions, whatever their order (lanes, shuffles), and
            the product with 1 / C (itself rounded) adds two roundings: (1 + u)^(C + 1) - 1 = (C + 1) u in first order.
  copy      |copy - dx_stored scale| <= (u + u_out)(1 + u) |dx_stored scale| (+ 2^-25 for fp16: half its smallest subnormal):
            one fp32 product, one rounding to the 16-bit type.  dx_stored is the fp32 dx the kernel wrote.
  reducers  a column sum whose addends pass at most D additions, then one product with scale: |err| <= (D + 1) u |scale|
            sum_i |ws_ij|.  reduce_rows_kernel<RL> and the batched kernel (RL = 32): ceil(nrows / RL) additions in a row lane
            (the first, to 0.f, is exact) and RL in the fold of the lanes: D = ceil(nrows / RL) + RL.  Wide kernel: D = nrows.
The reducer emulations hold additions and one product only, in the kernel's order: they reproduce its bits."""
import torch

U = 2.0 ** -24                                   # unit roundoff of fp32
U_OUT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HALF_SUBNORMAL = 2.0 ** -25                      # half the smallest fp16 subnormal: the absolute rounding error down there
VALUE_SETS = ("plain", "offset", "flat", "big", "subnormal")


def sub_abs(dtype):
    return HALF_SUBNORMAL if dtype == torch.float16 else 0.0


# ------------------------------------------------------------------------------------------------------------ inputs
def values(kind, rows, C, seed, dev="cpu"):
    """fp32 test data (rows, C).  plain: 2 randn.  offset: randn + 64 -- the set that separates one-pass from two-pass statistics.
    flat: 3 + 1e-4 randn (variance 1e-8, far below eps) with row rows // 2 exactly constant.  big: 3e4 (1 + 0.1 randn), near the
    top of the fp16 range.  subnormal: 2e-5 randn, inside the fp16 subnormal range."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(rows, C, generator=g)
    if kind == "plain":
        x = r * 2
    elif kind == "offset":
        x = r + 64
    elif kind == "flat":
        x = 3 + 1e-4 * r
        x[rows // 2] = 3.0
    elif kind == "big":
        x = (3e4 * (1 + 0.1 * r)).clamp(-6e4, 6e4)
    elif kind == "subnormal":
        x = 2e-5 * r
    else:
        raise ValueError(kind)
    return x.to(dev)


def params(C, seed, dev="cpu"):
    """gamma = 1 + 0.3 randn, beta = 0.3 randn (fp32)."""
    g = torch.Generator().manual_seed(seed)
    return (1 + 0.3 * torch.randn(C, generator=g)).to(dev), (0.3 * torch.randn(C, generator=g)).to(dev)


def mixed(nrows, ncols, seed, dev="cpu"):
    """randn x 10^randint(-3, 3): mixed magnitudes, so that the order of a sum shows in its bits."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-3, 4, (nrows, ncols), generator=g).float()
    return (torch.randn(nrows, ncols, generator=g) * torch.pow(torch.tensor(10.0), e)).to(dev)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
def forward(x, gamma, beta, eps, addend=None):
    """x (rows, C), gamma / beta (C,), float64.  Returns a dict: y, mean, var, rstd, sum (x + addend, or x), S_y."""
    assert x.dtype == gamma.dtype == beta.dtype == torch.float64
    s = x if addend is None else x + addend
    mean = s.sum(-1) / s.shape[-1]
    d = s - mean[:, None]
    var = (d * d).sum(-1) / s.shape[-1]
    rstd = (var + eps).pow(-0.5)
    y = d * rstd[:, None] * gamma + beta
    S_y = gamma.abs() * rstd[:, None] * (s.abs() + mean.abs()[:, None]) + beta.abs()
    return {"y": y, "mean": mean, "var": var, "rstd": rstd, "sum": s, "S_y": S_y}


def backward(dy, x, gamma, mean, rstd, dy2=None, addend=None):
    """dy, x (rows, C), gamma (C,), mean / rstd (rows,), float64.  Returns a dict: dx, dgamma, dbeta, S_dx, S_dg, S_db."""
    assert dy.dtype == x.dtype == gamma.dtype == mean.dtype == rstd.dtype == torch.float64
    C = x.shape[-1]
    d = dy if dy2 is None else dy + dy2
    xh = (x - mean[:, None]) * rstd[:, None]
    g = d * gamma
    m1 = g.sum(-1, keepdim=True) / C
    m2 = (g * xh).sum(-1, keepdim=True) / C
    dx = rstd[:, None] * (g - m1 - xh * m2)
    S_dx = rstd[:, None] * (g.abs() + g.abs().sum(-1, keepdim=True) / C + xh.abs() * ((g * xh).abs().sum(-1, keepdim=True) / C))
    if addend is not None:
        dx = dx + addend
        S_dx = S_dx + addend.abs()
    return {"dx": dx, "dgamma": (d * xh).sum(0), "dbeta": d.sum(0), "S_dx": S_dx, "S_dg": (d * xh).abs().sum(0), "S_db": d.abs().sum(0)}


def row_scale(scale, rows, rps):
    """scale[row / rps] per row, (rows, 1)."""
    return scale[torch.arange(rows, device=scale.device) // rps][:, None]


def copy16(dx, scale, rps, dtype):
    """round16(dx scale[row / rps]): dx float64 (rows, C), scale float64 or None."""
    v = dx if scale is None else dx * row_scale(scale, dx.shape[0], rps)
    return v.to(dtype)


def mean_bar(s, C):
    return (C + 1) * U * s.abs().sum(-1) / C


def copy_bar(dx_stored, scale, rps, dtype):
    """dx_stored: the fp32 dx the kernel wrote, as float64."""
    v = dx_stored if scale is None else dx_stored * row_scale(scale, dx_stored.shape[0], rps)
    return (U + U_OUT[dtype]) * (1 + U) * v.abs() + sub_abs(dtype)


# ------------------------------------------------------------------------------------- fp32 emulations of the forward
def forward_f32(x, gamma, beta, eps, one_pass=False):
    """The forward in fp32 torch (x, gamma, beta float32): the two-pass statistics the kernels compute, or (one_pass) the variance as
    E[x^2] - mean^2.  Only the form matters, not the summation order: this is the CPU proof that the `offset` values tell the two
    apart (tests/test_layernorm_reference_host.py)."""
    C = x.shape[-1]
    invC = torch.tensor(1.0 / C, dtype=torch.float32)
    mean = x.sum(-1) * invC
    d = x - mean[:, None]
    if one_pass:
        var = ((x * x).sum(-1) * invC - mean * mean).clamp_min(0)
    else:
        var = (d * d).sum(-1) * invC
    rstd = torch.rsqrt(var + eps)
    return {"y": d * rstd[:, None] * gamma + beta, "mean": mean, "rstd": rstd}


# ------------------------------------------------------------------------------------------------------------ reducers
def reduce_rl(nrows):
    """Row lanes of the reduce_rows_kernel<RL> that csts_reduce_rows launches."""
    return 32 if nrows > 64 else (8 if nrows > 8 else 2)


def reduce_ref(ws, scale):
    """fp64: out[j] = scale sum_i ws[i][j]; and sum_i |ws[i][j]|."""
    w = ws.double()
    return w.sum(0) * float(torch.tensor(scale, dtype=torch.float32)), w.abs().sum(0)


def reduce_rows_emulation(ws, scale, RL):
    """reduce_rows_kernel<RL> / reduce_rows_batched_kernel (RL = 32) in their own order: rows i = ty (mod RL) are added in
    increasing i into RL running sums that start at 0.f, the sums are added in order r = 0 .. RL - 1 starting from 0.f, the result
    is multiplied by scale.  (A lane without a row keeps 0.f; adding 0.f to a running sum changes no bit, and a running sum that
    started at +0.f is never -0.f, so padding the rows with zeros up to a multiple of RL is exact.)"""
    assert ws.dtype == torch.float32 and ws.dim() == 2
    nrows, ncols = ws.shape
    k = -(-nrows // RL)
    p = torch.zeros(k * RL, ncols, dtype=torch.float32, device=ws.device)
    p[:nrows] = ws
    p = p.view(k, RL, ncols)
    s = torch.zeros(RL, ncols, dtype=torch.float32, device=ws.device)
    for i in range(k):
        s = s + p[i]
    t = torch.zeros(ncols, dtype=torch.float32, device=ws.device)
    for r in range(RL):
        t = t + s[r]
    return t * torch.tensor(scale, dtype=torch.float32, device=ws.device)


def reduce_wide_emulation(ws, scale):
    """reduce_rows_wide_kernel: the rows added in increasing order into one sum that starts at 0.f, then multiplied by scale."""
    assert ws.dtype == torch.float32 and ws.dim() == 2
    s = torch.zeros(ws.shape[1], dtype=torch.float32, device=ws.device)
    for i in range(ws.shape[0]):
        s = s + ws[i]
    return s * torch.tensor(scale, dtype=torch.float32, device=ws.device)


def reduce_bar(absum, scale, nrows, RL=None):
    """(ceil(nrows / RL) + RL + 1) u |scale| sum_i |ws_ij| (row / batched kernels), (nrows + 1) u |scale| sum_i |ws_ij| (RL None: wide)."""
    depth = nrows if RL is None else -(-nrows // RL) + RL
    return (depth + 1) * U * abs(float(torch.tensor(scale, dtype=torch.float32))) * absum
