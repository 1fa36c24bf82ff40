"""fp64 reference of csts_gemm (csts_amd/csrc/gemm.hip, gemm4.hip, gemm5.hip), its value sets, the per-element bars of
tests/gemm_raw.py and fp64 emulations of wrong kernels.  Not a test module.  Plain torch in float64, CPU or GPU, no GPU import.

Reference   C64 = epilogue(A64 . B64) for NT (A [M,K], B [N,K]), NN (A [M,K], B [K,N]) and TN (A [K,M], B [K,N]).  A64 and B64 are
            the operands AS THE MFMA READS THEM: rounded to the library's 16-bit type when `compute` is 16-bit (fp32 operands are
            rounded while staging), untouched in fp32 mode -- so the only error left in a kernel's C is its fp32 accumulation and
            its epilogue.  Epilogue, in the order of the kernels (gemm_kernel, gemm.hip):
              pre = acc + bias;  aux <- pre (GELU);  act = gelu(pre)  or  pre * gelu'(aux as stored)  or  pre;
              C = act * row_scale[m / rows_per_scale] + residual,  residual = row m, row m % res_row_mod, or the trilinear
              up-sampling (align_corners = False) of the coarse grid res_up.
            gelu is the exact-erf one.
Scales      S_pre = |A64| . |B64| + |bias|          (what every rounding up to the pre-activation is relative to)
            S     = S_pre |slope| |scale| + |residual|, slope = 1 without an activation, |gelu'(pre64)| with GELU, |gelu'(aux)| with
                    DGELU.
            P     = |act| |scale| with GELU / DGELU, 0 otherwise: what the two roundings BEHIND the activation (the product with the
                    scale, the residual add) are relative to.  Where the slope vanishes S no longer covers them.
            up-sampled residual: |residual| = sum_taps |w| |r|.
Bars        u = 2^-24; u_out = 0 / 2^-8 / 2^-11 for fp32 / bf16 / fp16 storage; + 2^-25 for fp16 storage.
            |C - C64| <= k u S + 2 u P + F + u_out |C64|,   k = min(c_derived, measured constant); 2 u P is DERIVED (two roundings)
                                                            and is not scaled by the measured constant
            |aux - pre64| <= k u S_pre + u_out_aux |pre64|
  c_derived (DERIVED).  The K products of 16-bit operands are exact in fp32 (8 + 8 or 11 + 11 significand bits); in fp32 mode
            each is rounded once (<= u, relative to |a b|).  Summing K terms in ANY order -- MFMA blocks, k-tiles, lanes, the
            butterfly of the tiny kernel -- takes at most K additions per addend path (the first, to 0.f, included), each
            committing at most one ulp = 2 u of its partial sum (2 u rather than u: the matrix cores' adder is not documented to
            round to nearest), and every partial sum is bounded by |A| . |B| in first order: 2 K u |A|.|B|.  Split-K adds
            nsplit more additions per element (slab sums in the finishing pass, or fp32 atomics): 2 nsplit u.  The epilogue
            adds the bias (1), multiplies by the scale (1), adds the residual (1), each <= u of a quantity bounded by S: 3 u S.
            An up-sampled residual is 8 products w r (w itself a product of three rounded fp32 weights) and 8 additions:
            <= 14 u sum |w| |r|.  Together c_derived = 2 (K + nsplit) + 3 (+ 1 in fp32 mode, + 14 with res_up), first order in u.
  F         the function-error term, ABSOLUTE (1 - poly e cancels for large negative x, so it cannot be relative to the result):
            gelu_fast   0.5 |x| E |scale|                      E = 1.5e-7 + c_f u: the Abramowitz-Stegun bound common.h states
            dgelu_fast  (0.5 E + |h| pdf(h) c_f u) |pre| |scale|  plus the rounding of the device exp / rcp
            libm forms  c_f u |scale|   resp.   c_f u |pre| |scale|
            c_f is measured (tests/test_gpu_gemm.py BARS).
Which fn    fn_kind(): gemm2 / gemm3 / gemm4 / gemm5 take gelu_fast / dgelu_fast when aux_dt is 16-bit and the libm forms
            otherwise; gemm_kernel and the finishing pass of deterministic split-K always take the libm forms.
Value sets  plain: randn.  offset: randn + 1.5 for A and B, so that a dropped k-chunk moves every output (each product has mean
            2.25).  exact: integers in [-3, 3] for A and B, [-8, 8] for the bias, [-16, 16] for the residual, row_scale in
            {0.5, 1, 2} and, where the case sets scale_zero, 0 (a single scale: 0.5 or 2); res_up only with dyadic weights.
            Every product and partial sum is then an integer (or a small dyadic fraction) below 2^24 in any order: the fp32 result is exact and the expected C is C64 rounded ONCE to the storage
            type, bit for bit; reference() asserts the 2^24 condition on S itself.
            big / subnormal (fp16 library): plain values, A and B scaled by powers of two so that max |C64| lies in (1.5e4, 3e4]
            resp. (2^-16, 2^-15]."""
import math

import torch

U = 2.0 ** -24
U_OUT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HALF_SUBNORMAL = 2.0 ** -25
AS_BOUND = 1.5e-7                                 # |erf error| of Abramowitz-Stegun 7.1.26, as common.h states it
F32, F64 = torch.float32, torch.float64
VALUE_SETS = ("plain", "offset", "exact", "big", "subnormal")
MUTANTS = ("k16", "slab", "bias_n1", "res_before_scale", "scale_m1", "res_row_m", "tanh")


def sub_abs(dtype):
    return HALF_SUBNORMAL if dtype == torch.float16 else 0.0


def dt(name, half):
    """'f32' | 'h16' (the 16-bit type of the library under test) -> torch dtype."""
    return F32 if name == "f32" else half


def cdiv(a, b):
    return -(-a // b)


DEFAULTS = dict(a="h16", b="h16", c="h16", compute="h16", epi="none", bias=False, aux=None, gelu_dt=None, res=None, res_row_mod=0,
                rps=0, scale_zero=False, split=1, det=False, colsum=False, tile_rows=0, algo=0, res_up=None, pad=8, mis=None,
                kind="plain", seed=1, zero_c=False)


def case(layout, M, N, K, **kw):
    """One problem.  a / b / c / aux / res: 'f32' | 'h16' (aux / res None: absent); gelu_dt: the aux_dt handed over when GELU keeps
    no pre-activation (default: c); rps > 0: a row scale for every rps rows (scale_zero: one of them is 0); split / det: split_k
    and whether the workspace of deterministic split-K is given; res_up = (Ti, Hi, Wi, To, Ho, Wo); pad: elements added to every
    leading dimension; mis = {operand: elements} moves an operand's pointer; zero_c: C is pre-zeroed (atomic split-K)."""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    c = dict(DEFAULTS, layout=layout, M=M, N=N, K=K, **kw)
    if c["epi"] == "gelu" and c["aux"] is None and c["gelu_dt"] is None:
        c["gelu_dt"] = c["c"]
    if c["split"] > 1 and not c["det"]:
        c["zero_c"] = True
    return c


def aux_flavour(c):
    return c["aux"] if c["aux"] is not None else c["gelu_dt"]


def fn_kind(c, kernel_name):
    """None, 'fast' or 'libm': which GELU functions the kernel named `kernel_name` applies to this case."""
    if c["epi"] == "none":
        return None
    if (c["split"] > 1 and c["det"]) or kernel_name.startswith("gemm_kernel"):
        return "libm"
    return "fast" if aux_flavour(c) == "h16" else "libm"


def split_plan(c, kernel_name):
    """(k_chunk, nsplit) of route() in gemm.hip: k-tiles of 64 in gemm2, 32 in gemm_kernel, dealt over split_k slabs."""
    bk = 32 if kernel_name.startswith("gemm_kernel") else 64
    k_chunk = cdiv(cdiv(c["K"], bk), max(c["split"], 1)) * bk
    return k_chunk, cdiv(c["K"], k_chunk)


def finish_form(c, nsplit, ws_aligned=True):
    """(VEC, SL) launch_finish / launch_finish_v of gemm.hip choose."""
    vec = 4 if c["N"] % 4 == 0 and ws_aligned else 1
    nvec = cdiv(c["M"] * c["N"], vec)
    return vec, (16 if nsplit >= 16 and nvec < 16384 else (4 if nsplit >= 4 and nvec < 131072 else 1))


def c_derived(c, nsplit=1):
    return 2 * (c["K"] + (nsplit if nsplit > 1 else 0)) + 3 + (1 if c["compute"] == "f32" else 0) + (14 if c["res_up"] else 0)


# ------------------------------------------------------------------------------------------------------------ functions
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def pdf64(x):
    return 0.3989422804014327 * torch.exp(-0.5 * x * x)


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * pdf64(x)


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


# ------------------------------------------------------------------------------------------------------------ up-sampled residual
def up_axis(o_n, i_n, dev="cpu"):
    """Source cells and weights of one axis, torch's area_pixel_compute_source_index with align_corners = False."""
    o = torch.arange(o_n, dtype=F64, device=dev)
    s = ((o + 0.5) * (i_n / o_n) - 0.5).clamp_min(0)
    i0 = s.floor().long()
    i1 = i0 + (i0 < i_n - 1).long()
    l1 = s - i0
    return i0, i1, 1 - l1, l1


def res_up64(r64, grids, M):
    """r64 (B Ti Hi Wi, N) -> (up-sampled residual (M, N), sum |w| |r|), M = B To Ho Wo, rows ordered (b, t, h, w)."""
    Ti, Hi, Wi, To, Ho, Wo = grids
    B = M // (To * Ho * Wo)
    N = r64.shape[1]
    r = r64.view(B, Ti, Hi, Wi, N)
    out, ab = torch.zeros(B, To, Ho, Wo, N, dtype=F64, device=r64.device), torch.zeros(B, To, Ho, Wo, N, dtype=F64, device=r64.device)
    ta, ha, wa = up_axis(To, Ti, r64.device), up_axis(Ho, Hi, r64.device), up_axis(Wo, Wi, r64.device)
    for a in range(2):
        for e in range(2):
            for f in range(2):
                w = ta[2 + a].view(To, 1, 1) * ha[2 + e].view(1, Ho, 1) * wa[2 + f].view(1, 1, Wo)
                g = r[:, ta[a]][:, :, ha[e]][:, :, :, wa[f]]
                out += w.view(1, To, Ho, Wo, 1) * g
                ab += w.view(1, To, Ho, Wo, 1) * g.abs()
    return out.view(M, N), ab.view(M, N)


def dyadic_up(grids):
    """Every axis weight a multiple of 1/8 (the fine size a power-of-two multiple of the coarse one, at most 4x)."""
    return all(o % i == 0 and o // i in (1, 2, 4) for i, o in zip(grids[:3], grids[3:]))


# ------------------------------------------------------------------------------------------------------------ operands
def operands(c, half, dev="cpu"):
    """The operands of a case in their storage types, from one seeded CPU generator (so that the host test and the GPU test see the
    same numbers), moved to `dev`: A, B, bias, aux_in (DGELU), residual, res_full (M rows: what a kernel that forgets res_row_mod
    would read), row_scale."""
    g = torch.Generator().manual_seed(1000 * c["seed"] + 7)
    M, N, K, kind = c["M"], c["N"], c["K"], c["kind"]
    a_shape = (K, M) if c["layout"] == "TN" else (M, K)
    b_shape = (N, K) if c["layout"] == "NT" else (K, N)
    exact = kind == "exact"

    def ints(shape, lim):
        return torch.randint(-lim, lim + 1, shape, generator=g).float()

    if exact:
        A, B = ints(a_shape, 3), ints(b_shape, 3)
    else:
        A, B = torch.randn(a_shape, generator=g), torch.randn(b_shape, generator=g)
        if kind == "offset":
            A, B = A + 1.5, B + 1.5
    o = {}
    # (offset values: every |C| is near 2.25 K, and so is the 16-bit rounding of C; the bias and the residual are scaled with it so that a wrong one shows)
    wide = 1 + 0.1 * K if kind == "offset" else 1.0
    o["bias"] = (ints((N,), 8) if exact else torch.randn(N, generator=g) * wide) if c["bias"] else None
    o["aux_in"] = (1.5 * torch.randn(M, N, generator=g)).to(dt(c["aux"], half)) if c["epi"] == "dgelu" else None
    o["residual"] = o["res_full"] = None
    if c["res"] is not None:
        rd = dt(c["res"], half)
        if c["res_up"]:
            Ti, Hi, Wi, To, Ho, Wo = c["res_up"]
            assert M % (To * Ho * Wo) == 0 and (not exact or dyadic_up(c["res_up"]))
            rows = M // (To * Ho * Wo) * Ti * Hi * Wi
            o["residual"] = (ints((rows, N), 16) if exact else torch.randn(rows, N, generator=g) * wide).to(rd)
        else:
            full = (ints((M, N), 16) if exact else torch.randn(M, N, generator=g) * wide).to(rd)
            o["res_full"] = full
            o["residual"] = full[:c["res_row_mod"]].contiguous() if c["res_row_mod"] > 0 else full
    o["row_scale"] = None
    if c["rps"] > 0:
        ns = cdiv(M, c["rps"])
        # neighbouring scales always differ (by 0.5 at least): a kernel that takes the scale of row m - 1 at a boundary must show
        if exact:
            sc = torch.tensor([0.5, 2.0, 1.0])[(torch.arange(ns) + int(torch.randint(0, 3 if ns > 1 else 2, (1,), generator=g))) % 3]
        else:
            sc = 0.5 + torch.rand(ns, generator=g)
            sc[1::2] += 1.5
        if c["scale_zero"] and ns > 1:
            sc[ns // 2] = 0.0
            for j in (ns // 2 - 1, ns // 2 + 1):
                if 0 <= j < ns and sc[j] == 0:
                    sc[j] = 2.0
        o["row_scale"] = sc
    if kind in ("big", "subnormal"):
        rnd = (lambda t, n: t.to(dt(n, half)).double()) if c["compute"] != "f32" else (lambda t, n: t.double())
        a64, b64 = rnd(A, "h16"), rnd(B, "h16")
        p = (a64.t() if c["layout"] == "TN" else a64) @ (b64.t() if c["layout"] == "NT" else b64)
        top = 3e4 if kind == "big" else 2.0 ** -15
        e = math.floor(math.log2(top / float(p.abs().max())))
        A, B = A * 2.0 ** (e // 2), B * 2.0 ** (e - e // 2)
    o["A"], o["B"] = A.to(dt(c["a"], half)), B.to(dt(c["b"], half))
    return {k: (v.to(dev) if v is not None else None) for k, v in o.items()}


# ------------------------------------------------------------------------------------------------------------ reference
def reference(c, o, half, fn=None, plan=None, mutant=None):
    """fp64 result and error scales of case c on operands o.  fn: fn_kind() of the kernel; plan: split_plan() (the `slab` mutant
    and c_derived need it).  mutant: one of MUTANTS -- the same computation with one thing wrong.
    Returns C64, pre64, S, S_pre, P, fn_base, fn_coef (F = fn_base + c_f u fn_coef), c_derived, colsum64, colsum_abs."""
    M, N, K = c["M"], c["N"], c["K"]
    k_chunk, nsplit = plan if plan is not None else (K, 1)

    def mma(t):                                   # as the MFMA reads it
        return (t.to(half) if c["compute"] != "f32" else t).double()

    A64, B64 = mma(o["A"]), mma(o["B"])
    At = A64.t() if c["layout"] == "TN" else A64              # [M, K]
    Bt = B64 if c["layout"] == "NT" else B64.t()              # [N, K]
    k_hi = K
    if mutant == "k16":
        k_hi = K - 16
    elif mutant == "slab":
        k_hi = (nsplit - 1) * k_chunk
    P = At[:, :k_hi] @ Bt[:, :k_hi].t()
    S_pre = At.abs() @ Bt.abs().t()
    r = {"colsum64": None, "colsum_abs": None}
    if c["colsum"]:
        r["colsum64"], r["colsum_abs"] = At.sum(1), At.abs().sum(1)
    pre = P
    if o["bias"] is not None:
        b64 = o["bias"].double()
        if mutant == "bias_n1":
            b64 = b64[(torch.arange(N, device=b64.device) ^ 1).clamp_max(N - 1)]
        pre = pre + b64
        S_pre = S_pre + o["bias"].double().abs()
    one = torch.ones((), dtype=F64, device=P.device)
    slope, act_abs, fn_base, fn_coef = one, 0 * one, 0 * one, 0 * one
    if c["epi"] == "gelu":
        act = gelu_tanh64(pre) if mutant == "tanh" else gelu64(pre)
        slope, act_abs = dgelu64(pre).abs(), gelu64(pre).abs()
        if fn == "fast":
            fn_base, fn_coef = 0.5 * pre.abs() * AS_BOUND, 0.5 * pre.abs()
        else:
            fn_coef = torch.ones_like(pre)
    elif c["epi"] == "dgelu":
        h = o["aux_in"].double()
        act = pre * dgelu64(h)
        slope, act_abs = dgelu64(h).abs(), act.abs()
        if fn == "fast":
            fn_base, fn_coef = 0.5 * AS_BOUND * pre.abs(), (0.5 + h.abs() * pdf64(h)) * pre.abs()
        else:
            fn_coef = pre.abs()
    else:
        act = pre
    sc = one
    if o["row_scale"] is not None:
        rows = torch.arange(M, device=P.device)
        if mutant == "scale_m1":
            rows = (rows - 1).clamp_min(0)
        sc = o["row_scale"].double()[rows // c["rps"]].view(M, 1)
    res = res_abs = 0 * one
    if o["residual"] is not None:
        if c["res_up"]:
            res, res_abs = res_up64(o["residual"].double(), c["res_up"], M)
        elif c["res_row_mod"] > 0 and mutant != "res_row_m":
            res = o["residual"].double()[torch.arange(M, device=P.device) % c["res_row_mod"]]
            res_abs = res.abs()
        else:
            res = (o["res_full"] if c["res_row_mod"] > 0 else o["residual"]).double()
            res_abs = res.abs()
    C64 = (act + res) * sc if mutant == "res_before_scale" else act * sc + res
    S = S_pre * slope * sc.abs() + res_abs
    r.update(C64=C64, pre64=pre, S=S.expand(M, N), S_pre=S_pre, P=(act_abs * sc.abs()).expand(M, N), fn_base=(fn_base * sc.abs()).expand(M, N),
             fn_coef=(fn_coef * sc.abs()).expand(M, N), c_derived=c_derived(c, nsplit))
    if c["kind"] == "exact" and mutant is None:
        lim = 2.0 ** 24 / (64 if c["res_up"] else 2)          # partial sums are integers (halves with a 0.5 scale, 64ths with res_up)
        assert float((S_pre * torch.maximum(sc.abs(), one) + res_abs).max()) < lim, "exact value set: a partial sum may pass 2^24"
    return r


def bar(r, k, c_f, out_dtype):
    """Per-element bar of C."""
    return k * U * r["S"] + 2 * U * r["P"] + r["fn_base"] + c_f * U * r["fn_coef"] + U_OUT[out_dtype] * r["C64"].abs() + sub_abs(out_dtype)


def aux_bar(r, k, aux_dtype):
    return k * U * r["S_pre"] + U_OUT[aux_dtype] * r["pre64"].abs() + sub_abs(aux_dtype)


def applies(mutant, c, plan):
    """Whether a wrong kernel of this kind would compute something else on this case."""
    if mutant == "k16":
        return c["K"] >= 32
    if mutant == "slab":
        return plan[1] > 1
    if mutant == "bias_n1":
        return c["bias"] and c["N"] > 1
    if mutant == "res_before_scale":
        return c["rps"] > 0 and c["res"] is not None
    if mutant == "scale_m1":
        return 0 < c["rps"] < c["M"]
    if mutant == "res_row_m":
        return 0 < c["res_row_mod"] < c["M"]
    if mutant == "tanh":
        return c["epi"] == "gelu" and c["c"] == "f32"
    raise ValueError(mutant)


def finish_emulation(ws, nsplit, SL, bias, out_dtype):
    """splitk_finish_kernel<VEC, SL> without an activation, in its order, in fp32: lane l sums slabs l, l + SL, ... from 0.f, the
    lanes are folded in order, then the bias.  ws (nsplit, M, N) fp32.  Additions only: reproduces the kernel's bits."""
    lanes = []
    for l in range(SL):
        v = torch.zeros_like(ws[0])
        for s in range(l, nsplit, SL):
            v = v + ws[s]
        lanes.append(v)
    v = lanes[0]
    for l in range(1, SL):
        v = v + lanes[l]
    if bias is not None:
        v = v + bias
    else:
        v = v + 0.0
    return v.to(out_dtype)
