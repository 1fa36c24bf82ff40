"""Raw C-ABI harness for the depthwise stencil family of csts_amd/csrc/stencil.hip (csts_dwconv_strided, csts_dwconv_transposed /
_transposed2, csts_pool_ln_fwd, csts_dwconv_wgrad / _wgrad2, csts_dwconv_wgrad_grouped) against the fp64 reference and the bars of
tests/stencil_reference.py.  Shared by tests/test_gpu_stencil.py (bf16 library) and tests/stencil_worker.py (child processes: the
fp16 library, environment variants); not a test module itself.

Every tensor of a call is a Region: (B, N, C) elements inside a wider buffer -- GUARD elements, B batch elements of N rows of
`ts` >= C elements plus a batch pad, GUARD elements -- the way ops.py hands the kernels a slot of a (B, N, 3C) qkv buffer.  Every
base is 16-byte aligned and every stride a multiple of 8 elements, as the C-ABI demands.
  inputs : the whole buffer is NaN except the region itself.  A kernel that reads a foreign slot, a row gap or a guard band ends
           with a non-finite output (taps outside the grid read CLAMPED addresses of the region itself and a zero weight).
  outputs: the region is pre-filled with one NaN bit pattern, everything else with another (the sentinel).  After the call every
           element of the region must be finite and every other element of the buffer still the sentinel, bit for bit.
The error of every element is then held to the derived bars of stencil_reference (ratio = |err| / bar <= 1 for the convolutions
and the mean), or reported as a ratio / per-row relative error for the caller's measured bars (weight gradient, rstd, y)."""
import ctypes as C

import torch

from csts_amd import lib as L
import stencil_reference as SR

GUARD = 64                                       # elements in front of and behind every buffer (keeps 16-byte alignment)
SENT = {4: 0x7FC0DEAD, 2: 0x7FDE}                # the sentinel: a quiet NaN (fp32 / bf16 / fp16) no kernel produces
PREFILL = {4: 0x7FC00001, 2: 0x7FFF}             # what an output region holds before the call: another NaN
_IV = {4: torch.int32, 2: torch.int16}


def _sx(v, es):                                  # the bit pattern as a signed integer of the view's width
    return v - (1 << (8 * es)) if v >= 1 << (8 * es - 1) else v


def stream():
    return torch.cuda.current_stream().cuda_stream


def dt_code(dtype):
    return L.F32 if dtype == torch.float32 else L.BF16


class Region:
    """(B, N, C) elements of `dtype`: element (b, n, c) at GUARD + b * bs + n * ts + off + c of one flat buffer, bs = N * ts + pad."""

    def __init__(self, B, N, Cc, dtype, dev, ts=None, off=0, pad=0):
        ts = Cc if ts is None else ts
        assert ts % 8 == 0 and off % 8 == 0 and pad % 8 == 0 and off + Cc <= ts
        self.B, self.N, self.C, self.ts, self.off, self.bs, self.dtype = B, N, Cc, ts, off, N * ts + pad, dtype
        self.es = torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.empty(2 * GUARD + B * self.bs, dtype=dtype, device=dev)
        self.ibuf = self.buf.view(_IV[self.es])
        self.ibuf.fill_(_sx(SENT[self.es], self.es))
        self.mask = torch.zeros(self.buf.numel(), dtype=torch.bool, device=dev)
        self._strided(self.mask).fill_(True)
        assert self.ptr() % 16 == 0

    def _strided(self, flat):
        return flat.as_strided((self.B, self.N, self.C), (self.bs, self.ts, 1), GUARD + self.off)

    def view(self):
        return self._strided(self.buf)

    def ptr(self):
        return self.buf.data_ptr() + (GUARD + self.off) * self.es

    def load(self, data):
        """Input: NaN everywhere (the sentinel), the data in the region."""
        self.view().copy_(data.to(self.dtype))
        return self

    def arm(self):
        """Output: the sentinel everywhere, the other NaN in the region."""
        self.ibuf.fill_(_sx(SENT[self.es], self.es))
        self._strided(self.ibuf).fill_(_sx(PREFILL[self.es], self.es))
        return self

    def guards_ok(self):
        return bool((self.ibuf[~self.mask] == _sx(SENT[self.es], self.es)).all())

    def finite(self):
        return bool(torch.isfinite(self.view()).all())


class Spec:
    """One geometry: B, C, HD, fine (T, H, W), stride; N fine / coarse tokens per batch element."""

    def __init__(self, B, Cc, HD, fthw, stride):
        self.B, self.C, self.HD, self.fthw, self.stride = B, Cc, HD, tuple(fthw), tuple(stride)
        self.cthw = SR.coarse_grid(fthw, stride)
        self.Nf = fthw[0] * fthw[1] * fthw[2]
        self.Nc = self.cthw[0] * self.cthw[1] * self.cthw[2]
        self.heads = Cc // HD

    def geom(self, fine, coarse):
        g = L.DwconvGeom()
        g.B, g.C, g.HD = self.B, self.C, self.HD
        g.Tf, g.Hf, g.Wf = self.fthw
        g.Tc, g.Hc, g.Wc = self.cthw
        g.st, g.sh, g.sw = self.stride
        g.fine_batch_stride, g.fine_token_stride = fine.bs, fine.ts
        g.coarse_batch_stride, g.coarse_token_stride = coarse.bs, coarse.ts
        return g

    def fine_region(self, dtype, dev, layout):
        return _region(self.B, self.Nf, self.C, dtype, dev, layout)

    def coarse_region(self, dtype, dev, layout):
        return _region(self.B, self.Nc, self.C, dtype, dev, layout)

    def f5(self, t):
        return t.reshape(self.B, *self.fthw, self.C)

    def c5(self, t):
        return t.reshape(self.B, *self.cthw, self.C)

    def __repr__(self):
        return f"B{self.B} C{self.C} HD{self.HD} fine{self.fthw} stride{self.stride}"


def _region(B, N, Cc, dtype, dev, layout):
    """layout: ("slot", i) -- slot i of a (B, N, 3C) buffer, batch stride padded by 24 elements; ("rows", gap) -- rows of C + gap
    elements, batch stride padded by 8; "dense"."""
    if layout == "dense":
        return Region(B, N, Cc, dtype, dev)
    kind, v = layout
    if kind == "slot":
        return Region(B, N, Cc, dtype, dev, ts=3 * Cc, off=v * Cc, pad=24)
    return Region(B, N, Cc, dtype, dev, ts=Cc + v, off=0, pad=8)


def rand(shape, seed, dev, scale=1.0, big=False, subnormal=False):
    """Random normal data.  big: sigma 4e3, so |x| reaches ~1.6e4 and a 27-tap sum with weights of 0.25 (sigma ~5e3) ~2.3e4, near
    the top of the fp16 range (65504 is 12 sigma of the sum away: the outputs must stay finite); subnormal: every 5th channel in
    the fp16 subnormal range (|x| < 6.1e-5)."""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale
    if big:
        x = (x * 4e3).clamp(-3.2e4, 3.2e4)
    if subnormal:
        x[..., ::5] *= 1e-5
    return x.to(dev)


def weights(HD, seed, dev, scale=0.25):
    return (torch.randn(HD, 27, generator=torch.Generator().manual_seed(seed)) * scale).to(dev).contiguous()


OUTPUTS = None                                   # a list (tools/stencil_digest.py): every run_* appends (name, output Region)


def _record(name, *regions):
    if OUTPUTS is not None:
        OUTPUTS.extend((f"{name}[{i}]", r) for i, r in enumerate(regions))


def _ratio(err, bar):
    """Worst |err| / bar; an error where the bar is zero counts as infinite."""
    r = torch.where(bar > 0, err / bar, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = r.nan_to_num(nan=float("inf"), posinf=float("inf"))
    i = int(r.argmax())
    return float(r.flatten()[i]), i


def _conv_result(name, out, ref, A, extra_guards=()):
    got = out.view().double()
    ref = ref.reshape(got.shape)
    err = (got - ref).abs()
    ratio, at = _ratio(err, SR.conv_bar(ref, A.reshape(got.shape), out.dtype))
    return {"name": name, "finite": out.finite(), "guards": out.guards_ok() and all(g.guards_ok() for g in extra_guards),
            "ratio": ratio, "at": list(_unravel(at, got.shape)), "got": float(got.flatten()[at]), "ref": float(ref.flatten()[at])}


def _unravel(i, shape):
    idx = []
    for s in reversed(shape):
        idx.append(i % s)
        i //= s
    return tuple(reversed(idx))


# -------------------------------------------------------------------------------------------------------- the kernels
def run_strided(sp, f_dt, c_dt, dev, seed=1, fine_layout=("slot", 1), out_layout=("slot", 2), **kw):
    """csts_dwconv_strided: fine read in place from a slot, coarse written into a slot of a 3C-wide buffer."""
    fine = sp.fine_region(f_dt, dev, fine_layout).load(rand((sp.B, sp.Nf, sp.C), seed, dev, **kw))
    w = weights(sp.HD, seed + 100, dev)
    out = sp.coarse_region(c_dt, dev, out_layout).arm()
    g = sp.geom(fine, out)
    L.check(L.load().csts_dwconv_strided(C.byref(g), fine.ptr(), dt_code(f_dt), w.data_ptr(), out.ptr(), dt_code(c_dt), stream()),
            "csts_dwconv_strided")
    torch.cuda.synchronize()
    _record("strided", out)
    ref, A = SR.conv_strided(sp.f5(fine.view().double()), w.double(), sp.stride)
    return [_conv_result(f"strided {sp}", out, ref, A)]


def run_transposed(sp, dt, dev, nslots=1, seed=2, coarse_layout=("slot", 1), out_layout=("rows", 8), **kw):
    """csts_dwconv_transposed (nslots == 1) / csts_dwconv_transposed2: the coarse tensors read in place from slots of 3C-wide
    buffers, two different weight tables, two different destinations."""
    lib = L.load()
    s0 = 0 if coarse_layout == "dense" else coarse_layout[1]
    srcs = [sp.coarse_region(dt, dev, "dense" if coarse_layout == "dense" else ("slot", (s0 + i) % 3)).load(rand((sp.B, sp.Nc, sp.C), seed + i, dev, **kw)) for i in range(nslots)]
    ws = [weights(sp.HD, seed + 100 + i, dev) for i in range(nslots)]
    outs = [sp.fine_region(dt, dev, out_layout).arm() for i in range(nslots)]     # one geometry: the same strides for both slots
    g = sp.geom(outs[0], srcs[0])
    code = dt_code(dt)
    if nslots == 1:
        rc = lib.csts_dwconv_transposed(C.byref(g), srcs[0].ptr(), code, ws[0].data_ptr(), outs[0].ptr(), code, stream())
    else:
        vp2 = C.c_void_p * 2
        rc = lib.csts_dwconv_transposed2(C.byref(g), vp2(srcs[0].ptr(), srcs[1].ptr()), code, vp2(ws[0].data_ptr(), ws[1].data_ptr()),
                                         vp2(outs[0].ptr(), outs[1].ptr()), code, stream())
    L.check(rc, "csts_dwconv_transposed")
    torch.cuda.synchronize()
    _record("transposed", *outs)
    res = []
    for i in range(nslots):
        ref, A = SR.conv_transposed(sp.c5(srcs[i].view().double()), ws[i].double(), sp.fthw, sp.stride)
        res.append(_conv_result(f"transposed[{i}] {sp}", outs[i], ref, A))
    return res


def ln_params(HD, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (1 + 0.1 * torch.randn(HD, generator=g)).to(dev), (0.1 * torch.randn(HD, generator=g)).to(dev)


def run_pool_ln(sp, dt, dev, nslots=1, seed=3, fine_slots=True, **kw):
    """csts_pool_ln_fwd: conv_out and y element-wise / per row, mean and rstd per (token, head) row.  The fine tensors are slots 1
    and 2 of 3C-wide buffers; conv_out and y are rows of C + 8 elements with a padded batch stride (one geometry describes both)."""
    lib = L.load()
    rows = sp.B * sp.Nc * sp.heads
    fines = [sp.fine_region(dt, dev, ("slot", 1 + i) if fine_slots else ("rows", 8)).load(rand((sp.B, sp.Nf, sp.C), seed + i, dev, **kw)) for i in range(nslots)]
    ws = [weights(sp.HD, seed + 100 + i, dev) for i in range(nslots)]
    gbs = [ln_params(sp.HD, seed + 200 + i, dev) for i in range(nslots)]
    convs = [sp.coarse_region(dt, dev, ("rows", 8)).arm() for _ in range(nslots)]
    ys = [sp.coarse_region(dt, dev, ("rows", 8)).arm() for _ in range(nslots)]
    means = [Region(1, 1, rows, torch.float32, dev, ts=(rows + 7) // 8 * 8).arm() for _ in range(nslots)]
    rstds = [Region(1, 1, rows, torch.float32, dev, ts=(rows + 7) // 8 * 8).arm() for _ in range(nslots)]
    pa = L.PoolLnArgs()
    pa.geom, pa.nslots, pa.dt, pa.eps = sp.geom(fines[0], convs[0]), nslots, dt_code(dt), SR.LN_EPS
    for i in range(nslots):
        pa.fine[i], pa.weight[i], pa.gamma[i], pa.beta[i] = fines[i].ptr(), ws[i].data_ptr(), gbs[i][0].data_ptr(), gbs[i][1].data_ptr()
        pa.conv_out[i], pa.y[i], pa.mean[i], pa.rstd[i] = convs[i].ptr(), ys[i].ptr(), means[i].ptr(), rstds[i].ptr()
    L.check(lib.csts_pool_ln_fwd(C.byref(pa), stream()), "csts_pool_ln_fwd")
    torch.cuda.synchronize()
    for name, regions in (("conv_out", convs), ("y", ys), ("mean", means), ("rstd", rstds)):
        _record(f"pool_ln {name}", *regions)
    res = []
    for i in range(nslots):
        ref, A = SR.conv_strided(sp.f5(fines[i].view().double()), ws[i].double(), sp.stride)
        r = _conv_result(f"pool_ln[{i}] {sp} conv_out", convs[i], ref, A, (ys[i], means[i], rstds[i]))
        r["finite"] = r["finite"] and ys[i].finite() and means[i].finite() and rstds[i].finite()
        # The statistics are those of the STORED row (the kernel rounds the row to the activation type first, as the two-kernel
        # path does).  fp32: the stored row is the fp32 accumulator, so the reference is LayerNorm64 of the fp64 convolution and
        # the mean carries the convolution's 28 u A plus HD u of its own sum.  16-bit: a row rounded to 2^-8 / 2^-11 moves its mean
        # by far more than that bar, so the reference is LayerNorm64 of the row the kernel stored (which the conv_out check above
        # has just held to fp64 element by element); the same bar covers it: (HD + 1) u |stored| and |stored| <= A (1 + 2^-8 + 28 u).
        src = ref.reshape(sp.B, sp.Nc, sp.C) if dt == torch.float32 else convs[i].view().double()
        yref, mref, rref = SR.layer_norm_heads(src, sp.HD, gbs[i][0].double(), gbs[i][1].double())
        Arow = A.reshape(sp.B, sp.Nc, sp.heads, sp.HD).mean(-1)
        mean = means[i].view().double().reshape(sp.B, sp.Nc, sp.heads)
        rstd = rstds[i].view().double().reshape(sp.B, sp.Nc, sp.heads)
        r["mean_ratio"], _ = _ratio((mean - mref).abs(), SR.mean_bar(Arow, sp.HD))
        r["rstd_rel"] = float(((rstd - rref).abs() / rref).max())                                  # per row, every row
        yg = ys[i].view().double().reshape(sp.B, sp.Nc, sp.heads, sp.HD)
        yr = yref.reshape(sp.B, sp.Nc, sp.heads, sp.HD)
        r["y_rel"] = float(((yg - yr).norm(dim=-1) / yr.norm(dim=-1)).max())                       # per row rel-L2, every row
        r["min_var"] = float((1 / rref.pow(2) - SR.LN_EPS).min())
        res.append(r)
    return res


class WgradProblem:
    """fine / coarse of one stencil weight gradient and its fp64 reference.  roles "pool": fine = a qkv slot, coarse = the dense
    gradient with a padded batch stride; "upsample": fine = the gradient (rows with a gap), coarse = a qkv slot."""

    def __init__(self, sp, dt, dev, seed=4, roles="pool", **kw):
        self.sp, self.dt = sp, dt
        fl, cl = (("slot", 1), ("rows", 0)) if roles == "pool" else (("rows", 8), ("slot", 2))
        self.fine = sp.fine_region(dt, dev, fl).load(rand((sp.B, sp.Nf, sp.C), seed, dev, **kw))
        self.coarse = sp.coarse_region(dt, dev, cl).load(rand((sp.B, sp.Nc, sp.C), seed + 1, dev, **kw))
        self.g = sp.geom(self.fine, self.coarse)
        self.ref, self.mag, self.n = SR.conv_wgrad(sp.f5(self.fine.view().double()), sp.c5(self.coarse.view().double()), sp.HD, sp.stride)

    def result(self, name, dw, ok):
        err = (dw.double().reshape(self.sp.HD, 27) - self.ref).abs()
        ratio, at = _ratio(err, SR.U * self.mag)                  # in units of u x sum |fine| |coarse|
        return {"name": f"{name} {self.sp}", "finite": bool(torch.isfinite(dw).all()), "guards": ok, "ratio": ratio,
                "derived": self.n + 1, "n": self.n, "at": list(_unravel(at, (self.sp.HD, 27)))}


def _f32_out(n, dev):
    return Region(1, 1, n, torch.float32, dev, ts=(n + 7) // 8 * 8).arm()


def run_wgrad(probs, mode, dev):
    """mode "dweight": csts_dwconv_wgrad with the second stage inside the call; "null": dweight NULL, the partial rows of the
    workspace summed here (in fp64); "two": csts_dwconv_wgrad2 on pairs of problems that share a geometry (probs: list of pairs),
    dweight given for the first and NULL for the second."""
    lib = L.load()
    code = dt_code(probs[0][0].dt if mode == "two" else probs[0].dt)
    res = []
    for p in probs:
        pair = p if mode == "two" else (p,)
        sp, g = pair[0].sp, pair[0].g
        wsz = lib.csts_dwconv_wgrad_workspace(C.byref(g))
        per = wsz // 4
        assert wsz > 0 and per % (sp.HD * 27) == 0
        ws = _f32_out(per * len(pair), dev)
        dws = [_f32_out(sp.HD * 27, dev) for _ in pair]
        if mode == "two":
            vp2 = C.c_void_p * 2
            rc = lib.csts_dwconv_wgrad2(C.byref(g), vp2(pair[0].fine.ptr(), pair[1].fine.ptr()), code,
                                        vp2(pair[0].coarse.ptr(), pair[1].coarse.ptr()), code, vp2(dws[0].ptr(), None), ws.ptr(), wsz * 2, stream())
        else:
            rc = lib.csts_dwconv_wgrad(C.byref(g), pair[0].fine.ptr(), code, pair[0].coarse.ptr(), code,
                                       dws[0].ptr() if mode == "dweight" else None, ws.ptr(), wsz, stream())
        L.check(rc, "csts_dwconv_wgrad")
        torch.cuda.synchronize()
        _record(f"wgrad/{mode} workspace", ws)
        _record(f"wgrad/{mode} dweight", *dws)
        for i, q in enumerate(pair):
            given = mode == "dweight" or (mode == "two" and i == 0)
            ok = ws.finite() and ws.guards_ok() and dws[i].guards_ok()
            if given:
                dw = dws[i].view().flatten()
            else:                                                                   # a NULL dweight: nothing written anywhere
                ok = ok and bool((dws[i].ibuf[dws[i].mask] == _sx(PREFILL[4], 4)).all())
                dw = ws.view().flatten()[i * per:(i + 1) * per].double().view(-1, sp.HD * 27).sum(0)
            res.append(q.result(f"wgrad/{mode}[{i}]", dw, ok))
    return res


def run_wgrad_grouped(probs, dev, keep=None):
    """csts_dwconv_wgrad_grouped: every problem of the list in ONE launch; the partial rows summed here (in fp64).  keep (a list):
    receives the raw workspaces for bit comparisons."""
    lib = L.load()
    code = dt_code(probs[0].dt)
    items = (L.DwconvWgradItem * len(probs))()
    wss = []
    for i, p in enumerate(probs):
        gsz = lib.csts_dwconv_wgrad_grouped_workspace(C.byref(p.g))
        assert 0 < gsz <= lib.csts_dwconv_wgrad_workspace(C.byref(p.g)) and gsz % (p.sp.HD * 27 * 4) == 0
        wss.append(_f32_out(gsz // 4, dev))
        items[i].geom, items[i].fine, items[i].coarse, items[i].workspace = p.g, p.fine.ptr(), p.coarse.ptr(), wss[i].ptr()
    image = (C.c_uint8 * (L.DWCONV_WGRAD_TABLE_ENTRY * len(probs)))()
    nblocks = C.c_int(0)
    L.check(lib.csts_dwconv_wgrad_grouped_plan(items, len(probs), image, len(image), C.byref(nblocks)), "plan")
    table = torch.frombuffer(bytearray(bytes(image)), dtype=torch.uint8).to(dev)
    L.check(lib.csts_dwconv_wgrad_grouped(table.data_ptr(), len(probs), nblocks.value, code, stream()), "csts_dwconv_wgrad_grouped")
    torch.cuda.synchronize()
    _record("wgrad/grouped workspace", *wss)
    if keep is not None:
        keep.extend(wss)
    return [p.result("wgrad/grouped", ws.view().flatten().double().view(-1, p.sp.HD * 27).sum(0), ws.finite() and ws.guards_ok())
            for p, ws in zip(probs, wss)]


# ------------------------------------------------------------------------------------------------------------ verdicts
def worst(results, key="ratio"):
    return max((r[key] for r in results if key in r), default=0.0)


def conv_violations(results):
    """Every result that misses a derived bar (ratio <= 1), wrote a non-finite element or touched a guard / foreign slot."""
    return [r for r in results if not (r["finite"] and r["guards"] and r["ratio"] <= 1.0 and r.get("mean_ratio", 0.0) <= 1.0)]


def ln_violations(results, rstd_bar, y_bar):
    return [r for r in results if "rstd_rel" in r and not (r["rstd_rel"] <= rstd_bar and r["y_rel"] <= y_bar)]


def wgrad_violations(results, c_measured):
    """|err| <= min(n + 1, c_measured) u sum |fine| |coarse|."""
    return [r for r in results if not (r["finite"] and r["guards"] and r["ratio"] <= min(r["derived"], c_measured))]


# ----------------------------------------------------------------------------------------------- shared problem sets
RAGGED = [  # fine thw, stride
    ((3, 7, 5), (1, 2, 2)), ((4, 14, 14), (1, 8, 8)), ((3, 9, 13), (1, 4, 4)), ((3, 11, 8), (1, 3, 3)), ((5, 6, 6), (2, 2, 2)),
    ((4, 5, 5), (4, 1, 1)), ((1, 1, 6), (2, 2, 1)), ((2, 3, 3), (1, 8, 8)), ((2, 2, 2), (1, 1, 1)),
]
S22 = [((3, 8, 12), 1), ((4, 6, 4), 1), ((3, 8, 12), 2), ((4, 6, 4), 2), ((3, 8, 12), 4), ((4, 6, 4), 4)]   # even grids x st: NT = 3, 2, 1
POOL_HEADS = {8: (1, 2, 8), 64: (1, 2, 8), 104: (1, 2, 8), 128: (1, 2, 8), 160: (1, 2), 184: (1, 2), 96: (1, 2, 8), 192: (1, 2)}   # C <= 1024


def ragged_all(dt, dev, idx, **kw):
    """One row of the ragged table through strided, transposed, pool_ln_fwd (one slot) and the weight gradient (dweight given)."""
    fthw, st = RAGGED[idx]
    sp = Spec(2, 192, 96, fthw, st)
    res = run_strided(sp, dt, dt, dev, **kw) + run_transposed(sp, dt, dev, **kw) + run_pool_ln(sp, dt, dev, **kw)
    return res, run_wgrad([WgradProblem(sp, dt, dev, **kw)], "dweight", dev)


def s22_all(dt, dev, idx, **kw):
    """dwconv_transposed_s22_kernel (16-bit, sh = sw = 2, even grid): one and two slots, coarse read in place from a 3C buffer."""
    fthw, st = S22[idx]
    sp = Spec(2, 192, 96, fthw, (st, 2, 2))
    return run_transposed(sp, dt, dev, nslots=1, **kw) + run_transposed(sp, dt, dev, nslots=2, **kw)


def pool_cases(dt, dev, HD, **kw):
    """csts_pool_ln_fwd at one head_dim: heads in {1, 2, 8} (C <= 1024), one slot and two slots, on a ragged grid."""
    res = []
    for heads in POOL_HEADS[HD]:
        for ns in (1, 2):
            res += run_pool_ln(Spec(2, HD * heads, HD, (3, 7, 5), (1, 2, 2)), dt, dev, nslots=ns, **kw)
    return res


def wgrad_specs():
    """HD 8 / 32 / 64 / 64 / 96 / 160 / 192: the 192-channel slab holds 24 / 6 / 3 / 2 / 2 / 1 / 1 heads.  (3, 7, 5) by (1, 2, 2), B = 2:
    72 coarse tokens in 5 chunks of 15 (the last holds 12); one coarse token in total and two (lanes == 1); the (1, 3, 3) stride."""
    g = ((3, 7, 5), (1, 2, 2))
    return [Spec(2, 192, 8, *g), Spec(2, 192, 32, *g), Spec(2, 192, 64, *g), Spec(2, 128, 64, *g), Spec(2, 192, 96, *g),
            Spec(2, 320, 160, *g), Spec(2, 384, 192, *g), Spec(1, 192, 96, (1, 1, 1), (1, 1, 1)), Spec(1, 96, 96, (2, 3, 3), (1, 8, 8)),
            Spec(2, 64, 32, (3, 11, 8), (1, 3, 3))]


def pool_tiny(dt, dev, HD, **kw):
    """csts_pool_ln_fwd on one almost-empty workgroup (B = 1, one head, stride 1): a single item -- one token with 26 of its 27
    taps outside the grid, one slot -- and six (fine (1, 1, 3), two slots), against 8 to 32 lane groups per workgroup: most
    groups have no item at all."""
    return (run_pool_ln(Spec(1, HD, HD, (1, 1, 1), (1, 1, 1)), dt, dev, nslots=1, **kw)
            + run_pool_ln(Spec(1, HD, HD, (1, 1, 3), (1, 1, 1)), dt, dev, nslots=2, **kw))
